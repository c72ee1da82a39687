"""ABC-SMC with a full-covariance perturbation kernel on a posterior with strongly correlated parameters.

    theta in R^2,  prior N(0, 3^2 I),  y = (theta_1 + theta_2, 0.1 (theta_1 - theta_2)) + 0.05 z,  y_obs = (1, 0)

with the Euclidean distance and the Gaussian ABC kernel at epsilon = 0.05.  The sum of the parameters is observed ten times more
sharply than their difference, so the ABC posterior -- Gaussian, known in closed form (``analytic``) -- has correlation -0.980.  A
product of marginals as wide as the population in every coordinate (the diagonal perturbation kernel of ``smc.sample``) puts most
proposals off that ridge; the multivariate normal kernel with a multiple of the weighted population covariance
(``perturbation="full"``; Filippi et al. 2013) follows it.

The Model is defined twice: ``build()`` is a ``CompiledModel`` (the simulator as C source, run fused on the GPU) and ``Callback`` its
twin in plain torch for ``path="generic"``, CPU tensors included.

    python -m glabcmcmc_amd.examples.Correlated_smc        # diagonal against full, next to the analytic values
"""
import math

import numpy as np
import torch

NOISE, EPSILON, PRIOR_SCALE = 0.05, 0.05, 3.0
Y_OBS = [1.0, 0.0]

SOURCE = """
GLABC_SIMULATOR void glabc_user_simulate(const float* theta, const float* eps, float* y)
{   /* y = (theta_1 + theta_2, 0.1 (theta_1 - theta_2)) + 0.05 eps */
    y[0] = (theta[0] + theta[1]) + 0.05f * eps[0];
    y[1] = 0.1f * (theta[0] - theta[1]) + 0.05f * eps[1];
}
"""


def prior():
    from .. import distribution
    return distribution.DiagGaussian(2, torch.zeros(2), torch.full((2,), math.log(PRIOR_SCALE)))


def build(epsilon=EPSILON):
    from ..compiled import CompiledModel
    return CompiledModel(theta_dim=2, y_dim=2, simulator_source=SOURCE, prior=prior(), y_obs=Y_OBS, epsilon=epsilon, noise_dim=2)


class Callback:
    """the same Model through the callbacks of the Model protocol, in plain torch on the device of its arguments"""

    def __init__(self, epsilon=EPSILON):
        self.epsilon, self.theta_dim, self.y_dim = epsilon, 2, 2
        self.y_obs = torch.tensor([Y_OBS])

    def generate_samples(self, theta, num_samples=1):
        theta = theta.reshape(-1, 2)
        mean = torch.stack([theta[:, 0] + theta[:, 1], 0.1 * (theta[:, 0] - theta[:, 1])], dim=1)
        return mean + NOISE * torch.randn(mean.shape, device=theta.device)

    def discrepancy(self, y):
        y = y.reshape(-1, 2)
        return torch.sqrt(((y - self.y_obs.to(y.device)) ** 2).sum(dim=1))

    def calculate_log_kernel_dis(self, dis, epsilon=None):
        eps = self.epsilon if epsilon is None else epsilon
        return -0.5 * (dis / eps) ** 2 - math.log(eps) - 0.5 * math.log(2.0 * math.pi)


def analytic(epsilon=EPSILON):
    """mean (2,) and covariance (2, 2) of the ABC posterior: y_obs | theta ~ N(A theta, (0.05^2 + epsilon^2) I) under the prior"""
    A = np.array([[1.0, 1.0], [0.1, -0.1]])
    s2 = NOISE ** 2 + epsilon ** 2
    cov = np.linalg.inv(np.eye(2) / PRIOR_SCALE ** 2 + A.T @ A / s2)
    return cov @ (A.T @ np.asarray(Y_OBS) / s2), cov


def moments(pop):
    """weighted mean and covariance of a Population, float64 numpy"""
    w, x = pop.weights.double().cpu().numpy(), pop.theta.double().cpu().numpy()
    mean = w @ x
    return mean, (w[:, None] * (x - mean)).T @ (x - mean)


def main(n_particles=2000, seed=1, bandwidth="beaumont"):
    from .. import smc
    fused = torch.cuda.is_available()
    model = build() if fused else Callback()
    kw = dict(kernel="model", bandwidth=bandwidth, seed=seed) if fused else dict(kernel="model", bandwidth=bandwidth, path="generic", prior=prior())
    mean, cov = analytic()
    print("analytic: mean (%.4f, %.4f), variances (%.5f, %.5f), correlation %.3f"
          % (mean[0], mean[1], cov[0, 0], cov[1, 1], cov[0, 1] / math.sqrt(cov[0, 0] * cov[1, 1])))
    out = {}
    for perturbation in ("diagonal", "full"):
        if not fused:
            torch.manual_seed(seed)
        pop = smc.sample(model, n_particles, perturbation=perturbation, **kw)
        m, c = moments(pop)
        sims = sum(g["n_draws"] for g in pop.generations)
        print("%-8s (%s, %s): %d simulations, %d generations, ESS %.0f; mean (%.4f, %.4f), variances (%.5f, %.5f), correlation %.3f"
              % (perturbation, bandwidth, "fused" if fused else "generic", sims, len(pop.generations), pop.ess, m[0], m[1], c[0, 0], c[1, 1],
                 c[0, 1] / math.sqrt(c[0, 0] * c[1, 1])))
        out[perturbation] = pop
    return out


if __name__ == "__main__":
    main()
