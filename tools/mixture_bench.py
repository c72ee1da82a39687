"""GLMCMC on Mixture_set with a four-mode GaussianMixture importance proposal: whole calls of
  (a) path="auto"     the fused mixture kernel (glabc_glmcmc_mix_steps up to 16 proposals, glabc_glmcmc_mix_wide_steps above),
  (b) path="generic"  the split-phase path with the mixture as a callback -- what such a call ran before the kernel existed,
  (c) the fused kernel with a DiagGaussian importance proposal, as context,
timed with a host clock that ends in a device synchronise.  After a warm-up of each, (a) and (b) alternate in one process;
the median and the spread (max - min) of the repeats are reported, and (a) beats (b) only if the medians differ by more than
both spreads.  --split-iters gives (b) a shorter call of its own (it is three orders of magnitude slower); the comparison is then
one of seconds per iteration, and each entry names its own iteration count.

--compiled runs the same calls on a CompiledModel whose source is the |theta| + noise simulator: (a) is then the run-time compiled
mixture program (glabc_rtc_mix_steps), (b) the callback path such a call took before those programs existed.

--glmala runs whole GLMALA calls instead (bench.py's glmala workload: gf 0.8, tau 0.3, num_grad 100): (a) is glabc_glmala_mix_steps,
(b) generic.run_glmala with the mixture as a callback and the MALA gradient as float64 torch operations -- what path="auto" ran before
the kernel variant existed --, (c) glabc_glmala_steps with a DiagGaussian importance proposal: the price of the K-mode density.

    python tools/mixture_bench.py [--chains 65536] [--iters 2000] [--split-iters ITERS] [--batch 5] [--repeats 3] [--compiled]
                                  [--glmala] [--out profiles/mixture_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-abc-mcmc_amd"))
import glabcmcmc_amd as g  # noqa: E402
from glabcmcmc_amd.examples.Mixture import Mixture_set  # noqa: E402


# examples/Mixture.py:19-23 as user source: y = |theta| + sqrt(0.05) eps
COMPILED_SOURCE = """
GLABC_SIMULATOR void glabc_user_simulate(const float* theta, const float* eps, float* y)
{
    for (int j = 0; j < GLABC_Y_DIM; ++j) y[j] = fabsf(theta[j]) + 0.2236068f * eps[j];
}
"""


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--split-iters", type=int, default=None, help="iterations of a split-phase call (default: --iters)")
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup-iters", type=int, default=20)
    ap.add_argument("--compiled", action="store_true", help="a CompiledModel with the |theta| + noise simulator as C source")
    ap.add_argument("--glmala", action="store_true", help="whole GLMALA calls (gf 0.8, tau 0.3, num_grad 100) instead of GLMCMC")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    model = Mixture_set(0.05)
    if a.compiled:
        model = g.CompiledModel(2, 2, COMPILED_SOURCE, g.DiagGaussian(2, torch.zeros(2), torch.zeros(2)), [1.5, 1.5], 0.05)
    lp = g.DiagGaussian(2, torch.zeros(1, 2), torch.log(torch.tensor([0.35, 0.35])))
    mix = g.GaussianMixture(4, 2, loc=[[1.5, 1.5], [1.5, -1.5], [-1.5, 1.5], [-1.5, -1.5]], scale=[[0.5, 0.5]] * 4)
    gauss = g.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.log(torch.tensor([1.6, 1.6])))
    gen = torch.Generator().manual_seed(1234)
    th0 = torch.randn(a.chains, 2, generator=gen)
    y0 = th0.abs() + (0.05 ** 0.5) * torch.randn(a.chains, 2, generator=gen)
    kw = dict(seed=20261019, verbose=False, record_history=False)

    if a.glmala and a.compiled:
        ap.error("--glmala runs on Mixture_set: GLMALA has no run-time compiled kernels")

    def call(ip, path, iters):
        if a.glmala:
            return lambda: g.GLMALA(model, iters + 1, th0, y0, 0.3, 100, None, 0.8, ip, a.batch, path=path, **kw)
        return lambda: g.GLMCMC(model, iters + 1, th0, y0, lp, None, 0.9, ip, a.batch, path=path, **kw)

    iters = {"fused_mixture": a.iters, "split_phase_mixture": a.split_iters or a.iters, "fused_diag_gaussian": a.iters}
    runs = {"fused_mixture": call(mix, "auto", a.iters), "split_phase_mixture": call(mix, "generic", iters["split_phase_mixture"]),
            "fused_diag_gaussian": call(gauss, "auto", a.iters)}
    for name, (ip, path) in {"fused_mixture": (mix, "auto"), "split_phase_mixture": (mix, "generic"),
                             "fused_diag_gaussian": (gauss, "auto")}.items():
        clocked(call(ip, path, a.warmup_iters))              # warm-up: library load, graphs, caches
    times = {k: [] for k in runs}
    for _ in range(a.repeats):                               # (a) and (b) alternate; (c) rides along
        for name in ("fused_mixture", "split_phase_mixture", "fused_diag_gaussian"):
            times[name].append(clocked(runs[name]))
    res = {"workload": "%s on %s, theta_dim 2, 4-mode GaussianMixture importance proposal"
                       % ("GLMALA (gf 0.8, tau 0.3, num_grad 100)" if a.glmala else "GLMCMC",
                          "a CompiledModel (|theta| + noise as C source)" if a.compiled else "Mixture_set"), "chains": a.chains,
           "iterations": a.iters, "batch_size": a.batch, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    for name, ts in times.items():
        k = float(iters[name])
        res[name] = {"iterations": iters[name], "seconds": ts, "median_s": statistics.median(ts), "spread_s": max(ts) - min(ts),
                     "median_s_per_iteration": statistics.median(ts) / k, "spread_s_per_iteration": (max(ts) - min(ts)) / k,
                     "chain_steps_per_s": a.chains * k / statistics.median(ts)}
    fa, sb, dg = res["fused_mixture"], res["split_phase_mixture"], res["fused_diag_gaussian"]
    res["fused_over_split_phase"] = sb["median_s_per_iteration"] / fa["median_s_per_iteration"]
    res["fused_beats_split_phase_by_more_than_the_spread"] = bool(
        sb["median_s_per_iteration"] - fa["median_s_per_iteration"] > max(fa["spread_s_per_iteration"], sb["spread_s_per_iteration"]))
    res["fused_mixture_over_fused_diag_gaussian_time"] = fa["median_s"] / dg["median_s"]
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
