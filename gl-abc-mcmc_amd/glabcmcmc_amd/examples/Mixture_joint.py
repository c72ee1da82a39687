"""The joint posterior of Mixture_set from a history that stays on the GPU: what a filled density contour of (theta_1, theta_2)
shows, without pandas and seaborn.

The target is |theta| + noise, four symmetric modes in two dimensions: every marginal is a symmetric bimodal curve with mean 0,
and whether the chains hold all four modes or only two of them shows in the joint alone.

1. GLMCMC with ``return_device=True``; ``diagnostics.covariance`` / ``correlation`` of all pooled draws.
2. The mass of each quadrant: a 2 x 2 ``diagnostics.histogram2d`` over a symmetric range.
3. A 64 x 64 grid over the draws' exact range and its 50 / 90 / 95 % highest-density levels (``diagnostics.hpd_levels``): the
   count thresholds whose regions a contour plot fills; level / (N bin area) is the density at the contour.
4. The grid saved as ``.npy`` (uint64 [64][64], axis 0 along theta_1) for any plotting tool: with the printed levels,
   ``contourf(counts.T, levels=...)``.

    python -m glabcmcmc_amd.examples.Mixture_joint [Mixture_joint_grid.npy]          (needs an MI355X)
"""
import sys

import numpy as np
import torch

from .. import diagnostics, distribution
from ..GLMCMC import GLMCMC
from .Mixture import Mixture_set

PROBS = (0.5, 0.9, 0.95)


def main(n_chains=4096, num_ite=500, epsilon=0.05, seed=2026, half_width=4.0, out=None, verbose=True):
    """-> dict(covariance, correlation, quadrants [2][2] fractions, outside, levels, mass, n_bins_inside, density, grid, edges)"""
    Model = Mixture_set(epsilon)
    gen = torch.Generator().manual_seed(seed)
    theta0 = torch.randn(n_chains, 2, generator=gen)
    y0 = theta0.abs() + (0.05 ** 0.5) * torch.randn(n_chains, 2, generator=gen)
    lp = distribution.DiagGaussian(2, loc=torch.zeros(1, 2), log_scale=torch.log(torch.tensor([0.35, 0.35])))
    ip = distribution.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.log(torch.tensor([1.6, 1.6])))
    hist = GLMCMC(Model, num_ite, theta0, y0, lp, None, 0.9, ip, 5, seed=seed + 1, verbose=False, return_device=True)
    n = hist.shape[0] * hist.shape[1]
    terms = diagnostics.joint_terms(hist)
    cov, corr = diagnostics.covariance(terms), diagnostics.correlation(terms)
    quad = diagnostics.histogram2d(hist, bins=2, range=(-half_width, half_width))
    grid = diagnostics.histogram2d(hist, bins=64)
    counts, edges = grid.counts[0], grid.edges
    level, mass, inside = diagnostics.hpd_levels(counts, PROBS)
    area = (edges[0, 1] - edges[0, 0]) * (edges[1, 1] - edges[1, 0])
    res = {"covariance": cov, "correlation": corr, "quadrants": quad.counts[0] / float(n), "outside": int(quad.outside[0]),
           "levels": level, "mass": mass, "n_bins_inside": inside, "density": level / (float(counts.sum()) * area), "grid": counts,
           "edges": edges}
    if out:
        np.save(out, counts)
    if verbose:
        print("%d chains x %d iterations, epsilon = %g" % (n_chains, num_ite, epsilon))
        print("covariance   [[%.4f, %.4f], [%.4f, %.4f]]" % tuple(cov.reshape(-1)))
        print("correlation  [[%.4f, %.4f], [%.4f, %.4f]]" % tuple(corr.reshape(-1)))
        q = res["quadrants"]
        print("mass per quadrant (theta_1 < 0 | >= 0 down, theta_2 < 0 | >= 0 across)  [[%.4f, %.4f], [%.4f, %.4f]], %d draws outside +-%g"
              % (q[0, 0], q[0, 1], q[1, 0], q[1, 1], res["outside"], half_width))
        for i, p in enumerate(PROBS):
            print("%2.0f %% highest-density region: count level %d (density %.4f), %d of %d bins, %.4f of the draws"
                  % (100 * p, int(level[i]), res["density"][i], int(inside[i]), counts.size, int(mass[i]) / float(counts.sum())))
        if out:
            print("grid saved to", out)
    return res


if __name__ == "__main__":
    main(out=sys.argv[1] if len(sys.argv) > 1 else "Mixture_joint_grid.npy")
