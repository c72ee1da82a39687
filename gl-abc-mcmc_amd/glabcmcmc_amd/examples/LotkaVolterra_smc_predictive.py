"""The posterior predictive check of an ABC-SMC population: does the fitted predator-prey model reproduce the data?

``smc.sample`` on the compiled Lotka-Volterra Model of ``LotkaVolterra_smc`` returns 4096 weighted particles.  ``predictive.check_weighted``
simulates afresh from every particle -- ``weighted_predictive_kernel`` compiled around the simulator source
(``CompiledModel.weighted_predictive_program``) -- and counts every draw with its quantised weight: nothing is resampled, the weights
are not dropped.  Printed: the weighted posterior predictive p-value P(y_rep_j >= y_obs_j) of each of the eight observations, and the
weighted share of fresh simulations that land within epsilon of the data.

    python -m glabcmcmc_amd.examples.LotkaVolterra_smc_predictive        (needs an MI355X)
"""
import time

import torch

from . import LotkaVolterra_smc


def main(n_particles=4096, seed=1, verbose=True):
    from .. import predictive, smc
    model = LotkaVolterra_smc.build()
    pop = smc.sample(model, n_particles, kernel="model", seed=seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    check = predictive.check_weighted(model, pop, bins=64, seed=seed + 1)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    if verbose:
        print("ABC-SMC: %d particles, ESS %.0f, final tolerance %.3g" % (n_particles, pop.ess, pop.generations[-1]["epsilon"]))
        print("weighted predictive check: M = %d (sum of the quantised weights), %.3f s including the program's compilation" % (check.n, t1 - t0))
        print("  p-values P(y_rep >= y_obs): " + ", ".join("%.3f" % p for p in check.p_upper))
        print("  fresh simulations within epsilon = %g of the data: %.4f" % (float(model.epsilon), check.within_epsilon))
    return pop, check


if __name__ == "__main__":
    main()
