"""ABC-SMC on a predator-prey model: the textbook case of Toni et al. (2009, J. R. Soc. Interface 6:187), restated.

    dx/dt = a x - x y        dy/dt = b x y - y        x(0) = 1, y(0) = 0.5        theta = (a, b),  prior Uniform(0, 3)^2

The simulator integrates the deterministic equations with 3000 fixed RK4 steps over t in [0, 15], records prey and predator at
t = 3.75, 7.5, 11.25 and 15 (y_dim 8) and adds Gaussian observation noise of standard deviation 0.3 (noise_dim 8).  The data are the
trajectory of a = b = 1 with one such noise draw.  It is written with + - * / fmaf only, so a CPU build of the same source gives
the same bits; parameters for which the integration overflows give a NaN distance, which no acceptance rule keeps.

About 10^5 instructions per simulation: the expensive simulator for which DESIGN.md 4.7 expects ABC-SMC to beat plain rejection on
wall time.  Both run fused here -- the draw kernels of ``glabc_abc_draws`` / ``glabc_smc_draws`` compiled around the source
(``CompiledModel.draws_program``).

    python -m glabcmcmc_amd.examples.LotkaVolterra_smc        # 4096 weighted particles of the posterior
"""
import time

import torch

N_STEPS = 3000
Y_OBS = [0.90, 0.84, 1.93, 0.48, 0.13, 0.99, 1.52, 1.47]

SOURCE = """
GLABC_SIMULATOR void glabc_user_simulate(const float* theta, const float* eps, float* y)
{   /* theta = (a, b), eps[8] standard normals -> y = (x, y) at four times + 0.3 eps */
    const float a = theta[0], b = theta[1], h = 0.005f;
    float u = 1.0f, v = 0.5f;
    for (int k = 0; k < 4; ++k) {
        for (int s = 0; s < %d; ++s) {
            const float u1 = a * u - u * v, v1 = b * (u * v) - v;
            const float ua = fmaf(0.5f * h, u1, u), va = fmaf(0.5f * h, v1, v);
            const float u2 = a * ua - ua * va, v2 = b * (ua * va) - va;
            const float ub = fmaf(0.5f * h, u2, u), vb = fmaf(0.5f * h, v2, v);
            const float u3 = a * ub - ub * vb, v3 = b * (ub * vb) - vb;
            const float uc = fmaf(h, u3, u), vc = fmaf(h, v3, v);
            const float u4 = a * uc - uc * vc, v4 = b * (uc * vc) - vc;
            u = fmaf(h / 6.0f, (u1 + 2.0f * u2) + (2.0f * u3 + u4), u);
            v = fmaf(h / 6.0f, (v1 + 2.0f * v2) + (2.0f * v3 + v4), v);
        }
        y[2 * k] = fmaf(0.3f, eps[2 * k], u);
        y[2 * k + 1] = fmaf(0.3f, eps[2 * k + 1], v);
    }
}
""" % (N_STEPS // 4)


def build(epsilon=0.5):
    from .. import distribution
    from ..compiled import CompiledModel
    return CompiledModel(theta_dim=2, y_dim=8, simulator_source=SOURCE, prior=distribution.Uniform(2, torch.zeros(2), torch.full((2,), 3.0)),
                         y_obs=Y_OBS, epsilon=epsilon, noise_dim=8)


def main(n_particles=4096, seed=1):
    from .. import smc
    model = build()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pop = smc.sample(model, n_particles, kernel="model", seed=seed)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    mean = (pop.weights.unsqueeze(1) * pop.theta.double()).sum(0).tolist()
    draws = sum(g["n_draws"] for g in pop.generations)
    print("ABC-SMC: %d particles, ESS %.0f, %d generations, %d simulations, %.3f s; E(a, b) = (%.3f, %.3f)"
          % (n_particles, pop.ess, len(pop.generations), draws, t1 - t0, mean[0], mean[1]))
    rate = pop.generations[-1]["rate"]
    print("tolerances: %s; last acceptance rate %.3g" % (", ".join("%.3g" % g["epsilon"] for g in pop.generations), rate))
    return pop


if __name__ == "__main__":
    main()
