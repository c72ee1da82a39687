"""Does the fitted model reproduce the data?  The posterior predictive check of Mixture_set from a history that stays on the GPU.

The ``y`` a chain carries was accepted because it lay near ``y_obs``; a posterior predictive check simulates afresh for every
posterior draw and asks where ``y_obs`` lies among the replicated data.

1. GLMCMC with ``return_device=True``; ``predictive.check`` of the history: the predictive p-values ``P(y_rep_j >= y_obs_j)`` -- near
   1/2 for a model that fits, near 0 or 1 for one that does not --, the share of fresh distances within epsilon, and the histograms of
   ``y_rep`` and of the distance.
2. The same check of a deliberately misfitted history: the same draws shifted by +1.  The target's modes at theta_j = +-1.5 move to
   2.5 and -0.5, so the replicated |theta| + noise lies near 2.5 or near 0.5, never near ``y_obs`` = 1.5: the share of distances within
   epsilon collapses and the distance histogram moves away from 0, while a p-value can stay near 1/2 when both modes are held (half
   the replicates lie above, half below) -- a p-value alone does not certify a fit.

    python -m glabcmcmc_amd.examples.Mixture_predictive          (needs an MI355X)
"""
import torch

from .. import distribution, predictive
from ..GLMCMC import GLMCMC
from .Mixture import Mixture_set


def main(n_chains=4096, num_ite=500, epsilon=0.05, seed=2026, shift=1.0, verbose=True):
    """-> dict(fitted, shifted): the two ``predictive.Check`` tuples"""
    Model = Mixture_set(epsilon)
    gen = torch.Generator().manual_seed(seed)
    theta0 = torch.randn(n_chains, 2, generator=gen)
    y0 = theta0.abs() + (0.05 ** 0.5) * torch.randn(n_chains, 2, generator=gen)
    lp = distribution.DiagGaussian(2, loc=torch.zeros(1, 2), log_scale=torch.log(torch.tensor([0.35, 0.35])))
    ip = distribution.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.log(torch.tensor([1.6, 1.6])))
    hist = GLMCMC(Model, num_ite, theta0, y0, lp, None, 0.9, ip, 5, seed=seed + 1, verbose=False, return_device=True)
    lim = [(0.0, 4.0), (0.0, 4.0), (0.0, 3.0)]                    # one range for both, so the histograms can be laid over each other
    res = {"fitted": predictive.check(Model, hist, bins=32, range=lim, seed=seed + 2),
           "shifted": predictive.check(Model, hist + shift, bins=32, range=lim, seed=seed + 2)}
    if verbose:
        print("%d chains x %d iterations, epsilon = %g, y_obs = %r" % (n_chains, num_ite, epsilon, Model.y_obs.reshape(-1).tolist()))
        for name, c in res.items():
            print("%-8s P(y_rep >= y_obs) = [%.4f, %.4f]   distances within epsilon: %.4f   mode of the distance histogram: %.3f   (%d draws)"
                  % (name, c.p_upper[0], c.p_upper[1], c.within_epsilon, c.distance_edges[int(c.distance_counts.argmax())], c.n))
    return res


if __name__ == "__main__":
    main()
