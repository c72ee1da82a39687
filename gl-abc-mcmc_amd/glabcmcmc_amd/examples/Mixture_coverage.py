"""Is epsilon small enough?  The coverage check of Mixture_set's ABC posterior at three tolerances, under both kernels.

``coverage.check`` takes 512 test pairs (theta*, y*) from the prior predictive, runs ABC against each y* on one table of 2^17 prior
draws that is never stored, and ranks theta*_j in the resulting posterior sample.  A sound tolerance gives uniform ranks -- a flat
histogram, a chi^2(9) statistic near 9 and intervals that cover at their nominal level; a loose one gives an over-wide posterior, the
ranks pile up on both sides of the middle and the intervals cover too often.  Printed per epsilon in (0.05, 0.3, 1.0) and kernel: the
10-bin rank histogram pooled over the two coordinates, its chi^2, and the coverage of the central 50 / 90 / 95 % intervals.

Then the local variant of Prangle et al.: the test pairs are the 512 draws of a rejection sample nearest to y_obs -- drawn under
ANOTHER seed than the table's, or each test would meet itself in the table at distance 0 --, which asks the question where it
matters, near the data, with each test's own 1 % tolerance (``quantile=0.01``).

    python -m glabcmcmc_amd.examples.Mixture_coverage          (needs an MI355X)
"""
from .. import coverage, rejection
from .Mixture import Mixture_set

BOUND = 27.88                              # the 99.9 % point of chi^2(9)


def report(name, c):
    chi, cov = c.chi2(10), c.coverage((0.5, 0.9, 0.95))
    print("%-28s ranks %s  chi2(%d) %7.2f %s  coverage %s  empty %d  median ess %.0f"
          % (name, c.rank_histogram(10).sum(dim=0).tolist(), chi.dof, chi.value, "ok  " if chi.value < BOUND else "LOOSE",
             ["%.3f" % v for v in cov.pooled.tolist()], c.n_empty, float(c.ess.nanmedian())))
    return {"chi2": chi.value, "coverage": cov.pooled.tolist(), "n_empty": c.n_empty}


def main(n_tests=512, n_draws=1 << 17, seed=2026, verbose=True):
    """-> {(kernel, epsilon) | "local": dict(chi2, coverage, n_empty)}"""
    Model = Mixture_set(0.05)
    out = {}
    for kernel in ("hard", "model"):
        for eps in (0.05, 0.3, 1.0):
            c = coverage.check(Model, n_tests, n_draws, kernel=kernel, epsilon=eps, seed=seed)
            out[(kernel, eps)] = report("%s, epsilon = %g" % (kernel, eps), c) if verbose else \
                {"chi2": c.chi2(10).value, "coverage": c.coverage().pooled.tolist(), "n_empty": c.n_empty}
    near = rejection.sample(Model, 1 << 20, kernel="hard", n_accept=n_tests, seed=seed + 1)          # NOT the table's seed
    c = coverage.check(Model, n_tests, n_draws, kernel="hard", quantile=0.01, tests=near, seed=seed)
    out["local"] = report("local (near y_obs), q = 0.01", c) if verbose else \
        {"chi2": c.chi2(10).value, "coverage": c.coverage().pooled.tolist(), "n_empty": c.n_empty}
    return out


if __name__ == "__main__":
    main()
