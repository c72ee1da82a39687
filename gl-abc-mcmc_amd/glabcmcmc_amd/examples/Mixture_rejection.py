"""Where epsilon and the starting states come from: rejection ABC in front of GLMCMC, on Mixture_set.

1. ``rejection.calibrate_epsilon``: the tolerance as a quantile of the prior-predictive distances (instead of a hard-coded 0.05).
2. ``rejection.initial_state(kernel="model")``: every chain starts at an exact draw from the target (instead of theta = 0).
3. 4096 GLMCMC chains; ``diagnostics.summary`` of theta_j^2 over the chains next to the independent rejection draws' mean of
   theta_j^2 and the analytic value (per coordinate the posterior is proportional to N(theta; 0, 1) N(y_obs; |theta|, 0.05 + eps^2)).

    python -m glabcmcmc_amd.examples.Mixture_rejection          (needs an MI355X)
"""
import numpy as np
import torch

from .. import diagnostics, distribution, rejection
from ..GLMCMC import GLMCMC
from .Mixture import Mixture_set


def analytic_second_moment(epsilon, y_obs=1.5, s2=0.05):
    """E theta_j^2 under the ABC posterior of Mixture_set, by quadrature"""
    t = np.linspace(-12.0, 12.0, 2400001)
    w = np.exp(-0.5 * t * t - (y_obs - np.abs(t)) ** 2 / (2.0 * (s2 + epsilon * epsilon)))
    return float(np.sum(w * t * t) / np.sum(w))


def main(n_chains=4096, num_ite=500, calibration_draws=1 << 22, quantile=2e-4, seed=2026, verbose=True):
    """-> dict(epsilon, chains, rejection, analytic): E theta_j^2 three ways"""
    epsilon = rejection.calibrate_epsilon(Mixture_set(1.0), calibration_draws, quantile, seed=seed)
    Model = Mixture_set(epsilon)
    # the acceptance rate of the Model's kernel at this epsilon is unknown beforehand: four times the draws until enough are kept
    n_draws = 1024 * n_chains
    while True:
        exact = rejection.sample(Model, n_draws, kernel="model", seed=seed + 1)
        if exact.ids.numel() >= n_chains:
            break
        n_draws *= 4
    theta0, y0 = rejection.initial_state(Model, n_chains, n_draws=n_draws, kernel="model", seed=seed + 1)
    lp = distribution.DiagGaussian(2, loc=torch.zeros(1, 2), log_scale=torch.log(torch.tensor([0.35, 0.35])))
    ip = distribution.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.tensor([0.0, 0.0]))
    hist = GLMCMC(Model, num_ite, theta0, y0, lp, None, 0.9, ip, 5, seed=seed + 2, verbose=False, return_device=True)
    s = diagnostics.summary(hist * hist)                           # the chains' theta_j^2: mean, Monte Carlo standard error, split-R-hat
    sq = exact.theta.double() ** 2
    out = {"epsilon": epsilon, "n_draws": n_draws, "accepted": int(exact.ids.numel()),
           "chains": s["mean"], "chains_mcse": s["mcse"], "chains_rhat": s["rhat"],
           "rejection": sq.mean(dim=0).cpu().numpy(), "rejection_se": (sq.std(dim=0) / exact.ids.numel() ** 0.5).cpu().numpy(),
           "analytic": analytic_second_moment(epsilon)}
    if verbose:
        print("epsilon = %.5f (quantile %g of %d prior-predictive distances); %d of %d draws accepted by the Model's kernel"
              % (epsilon, quantile, calibration_draws, out["accepted"], n_draws))
        for j in range(2):
            print("E theta_%d^2   GLMCMC %.4f +- %.4f (split-R-hat %.3f)   rejection %.4f +- %.4f   analytic %.4f"
                  % (j, out["chains"][j], out["chains_mcse"][j], out["chains_rhat"][j], out["rejection"][j], out["rejection_se"][j],
                     out["analytic"]))
    return out


if __name__ == "__main__":
    main()
