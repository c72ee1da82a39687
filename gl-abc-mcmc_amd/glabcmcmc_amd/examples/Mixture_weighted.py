"""Summaries of weighted posterior samples next to those of a chain history of the same target.

1. ``smc.sample`` on Mixture_set -> a weighted population; ``weighted.summary``, ``weighted.interval`` and a 64 x 64
   ``weighted.histogram2d`` with its 50 / 90 / 95 % highest-density levels (``diagnostics.hpd_levels`` reads a weighted grid as it
   is), printed next to ``diagnostics.quantile`` / ``interval`` / ``histogram2d`` of a GLMCMC history of the same target.  The
   target is |theta| + noise, four symmetric modes: the intervals of both samplers must agree to their Monte-Carlo error, and the
   share of the bins inside a highest-density region too.
2. ``rejection.sample`` on the g-and-k Model at a loose tolerance, corrected by ``regression.adjust`` -> adjusted draws with kernel
   weights; their ``weighted.summary`` next to the unweighted summary of the kept draws (``weighted`` on a ``Rejection``: unit
   weights).

Nothing is resampled: a weight is quantised to an integer multiplicity and the summaries are exact order statistics and counts of
that multiset (glabcmcmc_amd/weighted.py).

    python -m glabcmcmc_amd.examples.Mixture_weighted          (needs an MI355X)
"""
import numpy as np
import torch

from .. import diagnostics, distribution, regression, rejection, smc, weighted
from ..GLMCMC import GLMCMC
from .GK import GK_set
from .Mixture import Mixture_set

PROBS = (0.5, 0.9, 0.95)
QUANTILES = (0.025, 0.25, 0.75, 0.975)          # not the median: it lies between the modes, where the distribution function is flat


def _levels(counts):
    level, mass, inside = diagnostics.hpd_levels(counts, PROBS)
    return [(int(inside[i]), int(mass[i]) / float(counts.sum())) for i in range(len(PROBS))]


def main(n_particles=4096, n_chains=4096, num_ite=500, epsilon=0.05, gk_draws=1 << 20, seed=2026, half_width=4.0, verbose=True):
    """-> dict(smc, chains, adjusted, kept): per sample the summary (or quantiles), the 95 % interval and, for the Mixture target,
    the (bins inside, share of the mass) of each highest-density region"""
    Model = Mixture_set(epsilon)
    pop = smc.sample(Model, n_particles, kernel="model", seed=seed)
    s = weighted.summary(pop, QUANTILES)
    lower, upper = weighted.interval(pop, 0.95)
    grid = weighted.histogram2d(pop, bins=64, range=(-half_width, half_width))
    res = {"smc": {"summary": s, "interval": (lower, upper), "hpd": _levels(grid.counts[0]), "outside": int(grid.outside[0])}}

    gen = torch.Generator().manual_seed(seed)
    theta0 = torch.randn(n_chains, 2, generator=gen)
    y0 = theta0.abs() + (0.05 ** 0.5) * torch.randn(n_chains, 2, generator=gen)
    lp = distribution.DiagGaussian(2, loc=torch.zeros(1, 2), log_scale=torch.log(torch.tensor([0.35, 0.35])))
    ip = distribution.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.log(torch.tensor([1.6, 1.6])))
    hist = GLMCMC(Model, num_ite, theta0, y0, lp, None, 0.9, ip, 5, seed=seed + 1, verbose=False, return_device=True)
    c_lower, c_upper = diagnostics.interval(hist, 0.95)
    c_grid = diagnostics.histogram2d(hist, bins=64, range=(-half_width, half_width))
    res["chains"] = {"quantiles": diagnostics.quantile(hist, s["probs"]), "interval": (c_lower, c_upper), "hpd": _levels(c_grid.counts[0]),
                     "outside": int(c_grid.outside[0])}

    gk = GK_set(0.5)
    kept = rejection.sample(gk, gk_draws, kernel="hard", quantile=0.05, seed=seed + 2)
    adjusted = regression.adjust(gk, kept)
    res["kept"] = {"summary": weighted.summary(kept), "interval": weighted.interval(kept, 0.95)}
    res["adjusted"] = {"summary": weighted.summary(adjusted), "interval": weighted.interval(adjusted, 0.95), "outside_prior": adjusted.outside_prior}

    if verbose:
        fmt = lambda v: "[" + ", ".join("%.4f" % x for x in np.ravel(v)) + "]"          # noqa: E731
        print("Mixture_set(%g): %d particles (ess %.0f, M = %d at scale 2^%d) against %d chains x %d iterations"
              % (epsilon, n_particles, s["ess"], s["M"], int(np.log2(s["scale"])), n_chains, num_ite))
        print("  mean %s, sd %s" % (fmt(s["mean"]), fmt(s["sd"])))
        for i, p in enumerate(s["probs"]):
            print("  quantile %.3f   weighted %s   chains %s" % (p, fmt(s["quantiles"][i]), fmt(res["chains"]["quantiles"][i])))
        print("  95 %% interval    weighted %s .. %s   chains %s .. %s" % (fmt(lower), fmt(upper), fmt(c_lower), fmt(c_upper)))
        for i, p in enumerate(PROBS):
            a, b = res["smc"]["hpd"][i], res["chains"]["hpd"][i]
            print("  %2.0f %% highest-density region: weighted %d bins holding %.4f, chains %d bins holding %.4f" % (100 * p, a[0], a[1], b[0], b[1]))
        for name in ("kept", "adjusted"):
            t = res[name]["summary"]
            print("g-and-k, %s draws (ess %.0f): mean %s, sd %s" % (name, t["ess"], fmt(t["mean"]), fmt(t["sd"])))
            print("  95 %% interval %s .. %s" % (fmt(res[name]["interval"][0]), fmt(res[name]["interval"][1])))
        print("  adjusted weight outside the prior: %.4f" % adjusted.outside_prior)
    return res


if __name__ == "__main__":
    main()
