"""Does the fitted predator-prey model reproduce the data?  The ABC-SMC fit of examples/LotkaVolterra_smc.py, then a posterior
predictive check of it.

The weighted particles are resampled (multinomial, by their weights) to an equally weighted history of one row, one chain per
draw, which stays on the GPU; ``predictive.check`` simulates the model afresh for every draw and counts.  The Model is a
``CompiledModel``, so the check runs in the predictive kernel compiled around its simulator (``CompiledModel.predictive_program``):
the 3000 RK4 steps of a draw run in registers, and the result is a function of (Model, theta, seed, id).

    python -m glabcmcmc_amd.examples.LotkaVolterra_predictive
"""
import time

import torch

from . import LotkaVolterra_smc


def main(n_particles=4096, n_draws=65536, seed=1):
    from .. import predictive
    pop = LotkaVolterra_smc.main(n_particles, seed)
    model = LotkaVolterra_smc.build()
    g = torch.Generator(device=pop.theta.device).manual_seed(seed)
    pick = torch.multinomial(pop.weights.to(device=pop.theta.device, dtype=torch.float32), n_draws, replacement=True, generator=g)
    history = pop.theta[pick].to(torch.float32).reshape(1, n_draws, 2)          # (T, C, D) = (1, draws, 2), on the GPU
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c = predictive.check(model, history, bins=32, seed=seed)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    print("posterior predictive check: %d fresh simulations in %.3f s (the first call compiles and checks the kernel)" % (c.n, t1 - t0))
    print("p-values P(y_rep >= y_obs): %s" % ", ".join("%.3f" % p for p in c.p_upper))
    print("share of fresh distances within epsilon = %.3g: %.3f" % (model.epsilon, c.within_epsilon))
    return c


if __name__ == "__main__":
    main()
