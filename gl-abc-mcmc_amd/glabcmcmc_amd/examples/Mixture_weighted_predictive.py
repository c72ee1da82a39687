"""The posterior predictive check of weighted draws next to that of a chain history of the same target.

``smc.sample`` on Mixture_set -> a weighted population, checked by ``predictive.check_weighted`` (every draw counts with its quantised
weight; nothing is resampled); a GLMCMC history of the same target, checked by ``predictive.check``.  Both posteriors are the same
up to the samplers' Monte-Carlo error, so the predictive p-values and the share of fresh simulations within epsilon of the data
should agree to that error.  Both are printed; nothing is asserted.

    python -m glabcmcmc_amd.examples.Mixture_weighted_predictive          (needs an MI355X)
"""
import torch

from .. import distribution, predictive, smc
from ..GLMCMC import GLMCMC
from .Mixture import Mixture_set


def main(n_particles=4096, n_chains=4096, num_ite=500, epsilon=0.05, seed=2026, verbose=True):
    """-> (Check of the population, Check of the history)"""
    Model = Mixture_set(epsilon)
    pop = smc.sample(Model, n_particles, kernel="model", seed=seed)
    lim = [(-1.0, 4.0), (-1.0, 4.0), (0.0, 3.0)]
    weighted_check = predictive.check_weighted(Model, pop, bins=64, range=lim, seed=seed + 1)

    gen = torch.Generator().manual_seed(seed)
    theta0 = torch.randn(n_chains, 2, generator=gen)
    y0 = theta0.abs() + (0.05 ** 0.5) * torch.randn(n_chains, 2, generator=gen)
    lp = distribution.DiagGaussian(2, loc=torch.zeros(1, 2), log_scale=torch.log(torch.tensor([0.35, 0.35])))
    ip = distribution.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.log(torch.tensor([1.6, 1.6])))
    hist = GLMCMC(Model, num_ite, theta0, y0, lp, None, 0.9, ip, 5, seed=seed + 2, verbose=False, return_device=True)
    chain_check = predictive.check(Model, hist[num_ite // 2:], bins=64, range=lim, seed=seed + 3)

    if verbose:
        fmt = lambda v: "[" + ", ".join("%.4f" % x for x in v) + "]"          # noqa: E731
        print("Mixture_set(%g): %d particles (ess %.0f, M = %d) against %d chains x %d iterations (N = %d)"
              % (epsilon, n_particles, pop.ess, weighted_check.n, n_chains, num_ite - num_ite // 2, chain_check.n))
        print("  p-values P(y_rep >= y_obs)     weighted %s   chains %s" % (fmt(weighted_check.p_upper), fmt(chain_check.p_upper)))
        print("  within epsilon of the data     weighted %.4f   chains %.4f" % (weighted_check.within_epsilon, chain_check.within_epsilon))
        share = lambda c: c.distance_counts[:8].sum() / float(c.n)          # noqa: E731
        print("  distance below %.3f            weighted %.4f   chains %.4f" % (chain_check.distance_edges[8], share(weighted_check), share(chain_check)))
    return weighted_check, chain_check


if __name__ == "__main__":
    main()
