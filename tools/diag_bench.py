"""Effective sample size of a many-chain history that stays on the GPU: whole calls of
  (a) diagnostics.ess(history, max_lag)     the float64 autocovariance kernels behind glabc_autocov, the chains' sums, the formulas,
  (b) the same pooled autocovariances through torch.fft on the same device (centre, rfft along time zero-padded to a power of two
      >= 2 T, |F|^2 summed over chains, one irfft of the pooled spectrum) and the same formulas, in float64 and in float32,
timed with a host clock that ends in a device synchronise.  The history is what GLMCMC on Mixture_set returns with
return_device=True.  After a warm-up of each, the three alternate in one process; the median and the spread (max - min) of the
repeats are reported, and (a) beats (b) only if the medians differ by more than both spreads.  The torch paths' peak extra device
memory is torch.cuda.max_memory_allocated over a call; glabc_autocov alone is timed with device events, and its bytes are counted
from the shapes: `unique` is the history read by each of the two kernels plus the outputs, `requested` what the load instructions
ask the caches for (every lag block of 20 reads a leading and a trailing row per time step).

    python tools/diag_bench.py [--chains 65536] [--iters 2000] [--max-lag 128] [--repeats 7] [--out profiles/diag_bench.json]
"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-abc-mcmc_amd"))
import glabcmcmc_amd as g  # noqa: E402
from glabcmcmc_amd import diagnostics as D  # noqa: E402
from glabcmcmc_amd.examples.Mixture import Mixture_set  # noqa: E402

HBM_SUSTAINED = 6.29e12           # bytes per second the part sustains on a copy
LAGS_PER_ITEM = 20                # csrc/glabc_diag.hip LAGS


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fft_ess(history, max_lag, dtype):
    """diagnostics.ess from torch.fft: history (T, C, D) on the device -> Ess"""
    x = history.permute(0, 2, 1).to(dtype)                            # [T][D][C]
    n, d, c = x.shape
    mean = x.mean(dim=0)
    size = 1 << int(np.ceil(np.log2(2 * n)))
    f = torch.fft.rfft(x - mean, n=size, dim=0)
    power = (f.real * f.real + f.imag * f.imag).sum(dim=2)            # pooled over chains: the transform is linear
    acov = torch.fft.irfft(power.to(f.dtype), n=size, dim=0)[:max_lag + 1] / n
    mean = mean.double()
    z = np.zeros((2, d))
    t = D.Terms(c, n, mean.sum(dim=1).cpu().numpy(), (mean * mean).sum(dim=1).cpu().numpy(), acov.double().cpu().numpy(), 0, z, z, z)
    return D.ess(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--max-lag", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lp = g.DiagGaussian(2, torch.zeros(1, 2), torch.log(torch.tensor([0.35, 0.35])))
    ip = g.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.log(torch.tensor([1.6, 1.6])))
    gen = torch.Generator().manual_seed(1234)
    th0 = torch.randn(a.chains, 2, generator=gen)
    y0 = th0.abs() + (0.05 ** 0.5) * torch.randn(a.chains, 2, generator=gen)
    hist = g.GLMCMC(Mixture_set(0.05), a.iters, th0, y0, lp, None, 0.9, ip, 5, seed=20261019, verbose=False, return_device=True)
    n, c, d = hist.shape
    history_bytes = hist.numel() * 4

    runs = {"kernel": lambda: D.ess(hist, a.max_lag), "torch_fft_float64": lambda: fft_ess(hist, a.max_lag, torch.float64),
            "torch_fft_float32": lambda: fft_ess(hist, a.max_lag, torch.float32)}
    results, peak = {}, {}
    for name, fn in runs.items():
        for _ in range(a.warmup):
            clocked(fn)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        _, results[name] = clocked(fn)
        peak[name] = torch.cuda.max_memory_allocated() - before
    times = {k: [] for k in runs}
    for _ in range(a.repeats):
        for name, fn in runs.items():
            times[name].append(clocked(fn)[0])

    # glabc_autocov alone, device events around the two kernels
    cm = hist.permute(0, 2, 1)
    mean = torch.empty(d, c, dtype=torch.float64, device=hist.device)
    acov = torch.empty(a.max_lag + 1, d, c, dtype=torch.float64, device=hist.device)
    kernel_ms = []
    for i in range(a.warmup + a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        D._autocov(cm, 0, c, a.max_lag, mean, acov)
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            kernel_ms.append(e0.elapsed_time(e1))
    lag_blocks = -(-(a.max_lag + 1) // LAGS_PER_ITEM)
    out_bytes = (a.max_lag + 2) * d * c * 8
    unique = 2 * history_bytes + out_bytes + d * c * 8
    requested = (1 + 2 * lag_blocks) * history_bytes + out_bytes + d * c * 8
    k_med = statistics.median(kernel_ms) * 1e-3

    res = {"workload": "diagnostics.ess of a GLMCMC history on Mixture_set (return_device=True)", "date": datetime.date.today().isoformat(),
           "device": torch.cuda.get_device_name(0), "chains": c, "rows": n, "theta_dim": d, "max_lag": a.max_lag, "repeats": a.repeats,
           "history_bytes": history_bytes}
    for name, ts in times.items():
        res[name] = {"seconds": ts, "median_s": statistics.median(ts), "spread_s": max(ts) - min(ts), "peak_extra_device_bytes": peak[name],
                     "tau": results[name].tau.tolist(), "ess": results[name].ess.tolist()}
    res["glabc_autocov"] = {"milliseconds": kernel_ms, "median_ms": statistics.median(kernel_ms), "spread_ms": max(kernel_ms) - min(kernel_ms),
                            "unique_bytes": unique, "requested_bytes": requested, "unique_bytes_per_s": unique / k_med,
                            "requested_bytes_per_s": requested / k_med, "unique_over_hbm_sustained": unique / k_med / HBM_SUSTAINED,
                            "lag_products_per_s": c * d * n * lag_blocks * LAGS_PER_ITEM / k_med}
    k = res["kernel"]
    for other in ("torch_fft_float64", "torch_fft_float32"):
        o = res[other]
        res["kernel_over_" + other] = o["median_s"] / k["median_s"]
        res["kernel_beats_%s_by_more_than_the_spread" % other] = bool(o["median_s"] - k["median_s"] > max(o["spread_s"], k["spread_s"]))
        res["tau_relative_difference_to_" + other] = float(np.max(np.abs(np.array(o["tau"]) / np.array(k["tau"]) - 1.0)))
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
