"""Can a loose tolerance be corrected?  Regression adjustment of rejection ABC on the g-and-k Model (GK_set).

Rejection at the 5 % quantile of the prior-predictive distances, raw and regression-adjusted (``regression.adjust``: local-linear,
Epanechnikov weights, Beaumont, Zhang and Balding 2002), next to plain rejection at the 0.1 % quantile of the same draws.  Per
parameter the posterior mean +- standard deviation (the true values are A, B, g, k = 3, 1, 2, 0.5), and the weighted share of the
adjusted draws that left the Uniform(0, 10)^4 prior's support -- the adjustment knows nothing of the bounds, so that share is
reported, not hidden.  A and B gain most; g and k are barely identified by 8 order statistics and move little.

    python -m glabcmcmc_amd.examples.GK_adjusted          (needs an MI355X)
"""
import numpy as np
import torch

from .. import regression, rejection
from .GK import GK_set

NAMES = ("A", "B", "g", "k")


def weighted_mean_sd(theta, w):
    t = theta.double()
    m = (w[:, None] * t).sum(0)
    return m.cpu().numpy(), torch.sqrt((w[:, None] * (t - m) ** 2).sum(0)).cpu().numpy()


def main(n_draws=1 << 21, loose=0.05, tight=0.001, seed=2026, verbose=True):
    """-> dict(raw, adjusted, tight: (mean, sd) per parameter; outside_prior, ess, delta, kept)"""
    model = GK_set(0.5)
    kept = rejection.sample(model, n_draws, kernel="hard", quantile=loose, seed=seed)
    a = regression.adjust(model, kept)
    near = rejection.sample(model, n_draws, kernel="hard", quantile=tight, seed=seed)
    uniform = torch.full((near.theta.shape[0],), 1.0 / near.theta.shape[0], dtype=torch.float64, device=near.theta.device)
    out = {"raw": weighted_mean_sd(kept.theta, a.weights), "adjusted": (a.mean, np.sqrt(np.diag(a.covariance))),
           "tight": weighted_mean_sd(near.theta, uniform), "outside_prior": a.outside_prior, "ess": a.ess, "delta": a.delta,
           "kept": (int(kept.ids.numel()), int(near.ids.numel()))}
    if verbose:
        print("%d prior draws; %d kept at the %g quantile (delta = %.3f, effective sample size %.0f), %d at the %g quantile"
              % (n_draws, out["kept"][0], loose, a.delta, a.ess, out["kept"][1], tight))
        for title, key in (("rejection at %g" % loose, "raw"), ("adjusted at %g" % loose, "adjusted"), ("rejection at %g" % tight, "tight")):
            m, s = out[key]
            print("%-22s %s" % (title, "   ".join("%s %.2f +- %.2f" % (NAMES[j], m[j], s[j]) for j in range(4))))
        print("share of the adjusted draws outside the prior's support: %.3f" % a.outside_prior)
    return out


if __name__ == "__main__":
    main()
