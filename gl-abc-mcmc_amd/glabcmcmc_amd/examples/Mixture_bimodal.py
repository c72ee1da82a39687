"""Mixture_set with a mixture proposal: the Model simulates y = |theta| + noise, so its posterior has 2^d symmetric modes --
four at (+-1.5, +-1.5) for the observation (1.5, 1.5).  An importance proposal with one Gaussian component per mode is the
textbook choice for the iSIR move; as a ``distribution.GaussianMixture`` (reference distribution.py:206-293) it runs inside
the fused GLMCMC kernel.

    python -m glabcmcmc_amd.examples.Mixture_bimodal [chains] [iterations]
"""
import sys

import torch

from .. import DiagGaussian, GaussianMixture, MCMCRunner
from .Mixture import Mixture_set


def main(chains=4096, iterations=500, batch_size=5, output_dir="./"):
    model = Mixture_set(0.05)
    local = DiagGaussian(2, torch.zeros(1, 2), torch.log(torch.tensor([0.35, 0.35])))
    importance = GaussianMixture(4, 2, loc=[[1.5, 1.5], [1.5, -1.5], [-1.5, 1.5], [-1.5, -1.5]], scale=[[0.5, 0.5]] * 4)
    theta0 = torch.randn(chains, 2)
    y0 = model.generate_samples(theta0)
    runner = MCMCRunner(model, output_dir)
    hist = runner.run_glmcmc(iterations, theta0, y0, 0.9, local, importance, batch_size, output_file=None, verbose=False)
    last = hist[-1]                                        # (chains, 2)
    for sx in (1, -1):
        for sy in (1, -1):
            share = ((torch.sign(last[:, 0]) == sx) & (torch.sign(last[:, 1]) == sy)).float().mean().item()
            print("mode (%+.1f, %+.1f): %.3f of the chains" % (1.5 * sx, 1.5 * sy, share))
    print("mean |theta| = (%.3f, %.3f)" % tuple(last.abs().mean(0).tolist()))
    return hist


if __name__ == "__main__":
    main(*[int(v) for v in sys.argv[1:3]])
