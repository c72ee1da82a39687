"""A CompiledModel at batch sizes beyond 16: GLMCMC through the run-time compiled lane-group kernel (path="fused") against the
split-phase path (path="generic", sentinel_redraw=False) on the same chains and seed -- both rates, and the two histories
compared bit for bit.  bench.py --workload callback always runs N = 5, so this is the split-phase comparison at large N.

    python tools/rtc_wide_bench.py [--batch 32 64 256] [--chains 16384] [--iters 50] [--repeats 3]
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

# bench.py's RTC_MIXTURE: examples/Mixture.py:19-23 as user source (the Mixture Model, noise scale sqrt(0.05))
SIM = """
GLABC_SIMULATOR void glabc_user_simulate(const float* theta, const float* eps, float* y)
{
    for (int j = 0; j < GLABC_Y_DIM; ++j) y[j] = fabsf(theta[j]) + 0.2236068f * eps[j];
}
"""


def timed(fn, repeats):
    fn()                                                     # warm-up: compile, self-check, graphs, caches
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[32, 64, 256])
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    prior = g.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.tensor([0.0, 0.0]))
    cm = g.CompiledModel(2, 2, SIM, prior, [1.5, 1.5], 0.05)
    lp = g.DiagGaussian(2, torch.zeros(1, 2), torch.log(torch.tensor([0.35, 0.35])))
    ip = g.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.tensor([0.0, 0.0]))
    gen = torch.Generator().manual_seed(1234)
    th0 = torch.randn(a.chains, 2, generator=gen)
    y0 = th0.abs() + (0.05 ** 0.5) * torch.randn(a.chains, 2, generator=gen)
    for N in a.batch:
        kw = dict(seed=20261003, verbose=False, return_device=True)
        tf, hf = timed(lambda: g.GLMCMC(cm, a.iters + 1, th0, y0, lp, None, 0.9, ip, N, path="fused", **kw), a.repeats)
        ts, hs = timed(lambda: g.GLMCMC(cm, a.iters + 1, th0, y0, lp, None, 0.9, ip, N, path="generic", sentinel_redraw=False, **kw),
                       a.repeats)
        same = torch.equal(hf.contiguous().view(torch.int32), hs.contiguous().view(torch.int32))
        steps = float(a.chains) * a.iters
        print(json.dumps({"batch_size": N, "chains": a.chains, "iterations": a.iters,
                          "fused_chain_steps_per_s": steps / tf, "split_phase_chain_steps_per_s": steps / ts,
                          "fused_over_split_phase": ts / tf, "fused_s": tf, "split_phase_s": ts, "bit_identical": bool(same)}),
              flush=True)
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
