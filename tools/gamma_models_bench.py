"""Gamma priors and proposals on the two Models that need positive parameters: GLMCMC through the fused kernels (path="fused")
against the split-phase path (path="generic") on the same chains and seed.  The split-phase path is what these calls ran before
the fused kernels took a Gamma on g-and-k and on a CompiledModel, so the ratio is the gain of that change.

Whole-call wall time ending in a device synchronise; every shape is warmed up first (compile, self-check, graphs); fused and
split-phase alternate in one process; one JSON line per configuration with every repeat's time, and the two histories are
compared bit for bit.

    python tools/gamma_models_bench.py [--batch 5 64] [--chains 16384] [--iters 50] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-abc-mcmc_amd"))
import glabcmcmc_amd as g  # noqa: E402
from glabcmcmc_amd.examples.GK import GK_set  # noqa: E402

# theta[2] (a rate and a scale), eps[3] -> y[3]
SIM = """
GLABC_SIMULATOR void glabc_user_simulate(const float* theta, const float* eps, float* y)
{
    y[0] = theta[1] / (theta[0] + 0.5f) + 0.2f*eps[0];
    y[1] = sqrtf(fabsf(theta[0]*theta[1])) + 0.2f*eps[1];
    y[2] = glabc_logf(1.0f + theta[0]*theta[0]) * glabc_expf(0.1f*eps[2]);
}
"""


def gamma(shape, rate):
    return g.Gamma(torch.tensor(shape), torch.tensor(rate))


def configurations(chains):
    gen = torch.Generator().manual_seed(1234)
    gk = GK_set(1.0, prior=gamma([3.0, 2.0, 2.0, 1.5], [1.0, 2.0, 1.0, 3.0]))
    th0 = torch.tensor([3.0, 1.0, 2.0, 0.5]) * torch.exp(0.2 * torch.randn(chains, 4, generator=gen))
    y0 = torch.sort(3.0 + 2.0 * torch.randn(chains, 8, generator=gen), dim=1).values
    yield ("gk", gk, th0, y0, g.DiagGaussian(4, torch.zeros(1, 4), torch.log(torch.full((4,), 0.15))),
           gamma([9.0, 4.0, 4.0, 2.0], [3.0, 4.0, 2.0, 4.0]))
    cm = g.CompiledModel(2, 3, SIM, gamma([2.0, 3.0], [1.0, 2.0]), [1.0, 1.5, 1.2], 0.4, noise_dim=3)
    th0 = torch.randn(chains, 2, generator=gen).abs() + 0.5
    y0 = cm.simulate_from_noise(th0, torch.randn(chains, 3, generator=gen)).cpu()
    yield ("user", cm, th0, y0, g.DiagGaussian(2, torch.zeros(1, 2), torch.log(torch.full((2,), 0.3))), gamma([4.0, 4.0], [2.5, 2.5]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[5, 64])
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    ok = True
    for name, model, th0, y0, lp, ip in configurations(a.chains):
        for N in a.batch:
            kw = dict(seed=20261018, verbose=False, return_device=True)
            runs = {"fused": lambda: g.GLMCMC(model, a.iters + 1, th0, y0, lp, None, 0.8, ip, N, path="fused", **kw),
                    "split_phase": lambda: g.GLMCMC(model, a.iters + 1, th0, y0, lp, None, 0.8, ip, N, path="generic", **kw)}
            out, times = {}, {"fused": [], "split_phase": []}
            for which, fn in runs.items():                       # warm-up of every shape
                fn()
                torch.cuda.synchronize()
            for _ in range(a.repeats):                           # alternating
                for which, fn in runs.items():
                    t0 = time.perf_counter()
                    out[which] = fn()
                    torch.cuda.synchronize()
                    times[which].append(time.perf_counter() - t0)
            same = torch.equal(out["fused"].contiguous().view(torch.int32), out["split_phase"].contiguous().view(torch.int32))
            ok = ok and same
            steps = float(a.chains) * a.iters
            tf, ts = times["fused"], times["split_phase"]
            print(json.dumps({"model": name, "batch_size": N, "chains": a.chains, "iterations": a.iters,
                              "fused_s": tf, "split_phase_s": ts,
                              "fused_chain_steps_per_s": steps / min(tf), "split_phase_chain_steps_per_s": steps / min(ts),
                              "fused_over_split_phase": min(ts) / min(tf),
                              # the least and the largest ratio any pairing of the repeats gives: the spread of the measurement
                              "ratio_low": min(ts) / max(tf), "ratio_high": max(ts) / min(tf),
                              "bit_identical": bool(same)}), flush=True)
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
