"""ABC-SMC next to plain rejection ABC on Mixture_set(0.05): the same target, a fraction of the simulations.

1. ``smc.sample(kernel="model")``: hard generations down a ladder of tolerances, each the median distance of the one before, then
   one generation accepted by the Model's own kernel -- weighted particles of the posterior the MCMC samplers target.
2. ``rejection.sample(kernel="model")`` sized to accept about as many draws: independent unweighted draws of the same posterior.
3. The ladder, the simulations both used, and E theta_j^2 three ways: weighted particles, rejection draws, analytic (per coordinate
   the posterior is proportional to N(theta; 0, 1) N(y_obs; |theta|, 0.05 + eps^2)).

    python -m glabcmcmc_amd.examples.Mixture_smc          (needs an MI355X)
"""
import numpy as np

from .. import rejection, smc
from .Mixture import Mixture_set
from .Mixture_rejection import analytic_second_moment


def main(n_particles=4096, epsilon=0.05, seed=2026, verbose=True):
    """-> dict(ladder, simulations, rejection_simulations, smc, smc_se, rejection, rejection_se, analytic, ess)"""
    Model = Mixture_set(epsilon)
    p = smc.sample(Model, n_particles, kernel="model", seed=seed)
    sims = sum(g["n_draws"] for g in p.generations)
    # plain rejection for the same count: N / rate draws, the rate from a pilot
    pilot = rejection.sample(Model, 1 << 22, kernel="model", seed=seed + 1)
    rate = pilot.ids.numel() / float(1 << 22)
    n_draws = int(np.ceil(n_particles / rate))
    exact = rejection.sample(Model, n_draws, kernel="model", seed=seed + 2)
    w, f = p.weights, p.theta.double() ** 2
    mean = (w.unsqueeze(1) * f).sum(dim=0)
    se = ((w * w).unsqueeze(1) * (f - mean) ** 2).sum(dim=0).sqrt()
    sq = exact.theta.double() ** 2
    out = {"ladder": [g["epsilon"] for g in p.generations], "simulations": sims, "rejection_simulations": n_draws,
           "rejection_accepted": int(exact.ids.numel()), "ess": p.ess, "smc": mean.cpu().numpy(), "smc_se": se.cpu().numpy(),
           "rejection": sq.mean(dim=0).cpu().numpy(), "rejection_se": (sq.std(dim=0) / exact.ids.numel() ** 0.5).cpu().numpy(),
           "analytic": analytic_second_moment(epsilon)}
    if verbose:
        for t, g in enumerate(p.generations):
            print("generation %d: %-5s epsilon %.4f  %8d draws  acceptance %.4f  ess %.0f" % (t, g["kernel"], g["epsilon"], g["n_draws"], g["rate"], g["ess"]))
        print("%d particles (ess %.0f) from %d simulations; plain rejection accepted %d of %d (N / rate): %.1f times as many"
              % (n_particles, p.ess, sims, out["rejection_accepted"], n_draws, n_draws / sims))
        for j in range(2):
            print("E theta_%d^2   SMC %.4f +- %.4f   rejection %.4f +- %.4f   analytic %.4f"
                  % (j, out["smc"][j], out["smc_se"][j], out["rejection"][j], out["rejection_se"][j], out["analytic"]))
    return out


if __name__ == "__main__":
    main()
