"""Joint summaries of a many-chain history that stays on the GPU: whole calls of
  (a) diagnostics.histogram2d(history, bins=64)                     one glabc_histogram2d launch behind the exact range,
  (b) the best torch composition on the device: float64 bin indices of both coordinates and torch.bincount, per pair, over the
      same range (the range itself is not timed for torch: it is handed the one (a) found),
  (c) diagnostics.covariance(history)                               glabc_cross_moments in slabs and the pooled formula,
  (d) torch.cov of the float64 reshaped history,
timed with a host clock that ends in a device synchronise, on two histories of the same byte size: what GLMCMC on Mixture_set
returns with return_device=True (65 536 chains x 2000 iterations, theta_dim 2, one pair) and a synthetic theta_dim 8 history
(65 536 chains x 500 rows of correlated normal draws, all 28 pairs).  After the warm-ups the paths alternate in one process; the
median and the spread (max - min) of the repeats are reported, and one path beats another only if the medians differ by more than
both spreads.  A path that raises (out of memory) is recorded with its message and left out.  Peak extra device memory is
torch.cuda.max_memory_allocated over a call.  Each kernel is timed alone with device events and set against one read of the
history at the sustained HBM rate (the 28 pairs of theta_dim 8 read every coordinate seven times, the cross moments read the
history twice: the fraction says what the call costs in units of one read, not what the kernel achieves per byte it touches).

    python tools/joint_bench.py [--chains 65536] [--iters 2000] [--repeats 7] [--out profiles/joint_bench.json]
"""
import argparse
import ctypes as C
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
from glabcmcmc_amd import _capi  # noqa: E402
from glabcmcmc_amd import diagnostics as D  # noqa: E402
from glabcmcmc_amd.examples.Mixture import Mixture_set  # noqa: E402

HBM_SUSTAINED = 6.29e12           # bytes per second the part sustains on a copy
BINS = 64


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def torch_histogram2d(hist, pairs, lo, hi):
    """(T, C, D) device tensor -> int64 [P][BINS][BINS]: glabc_histogram's bin arithmetic in torch float64, draws with a value
    outside or a NaN dropped"""
    out = []
    for a, b in pairs:
        idx, keep = [], None
        for j in (a, b):
            x = hist[:, :, j].reshape(-1).double()
            ok = (x >= lo[j]) & (x <= hi[j])
            u = torch.floor((x - lo[j]) * (BINS / (hi[j] - lo[j]))).clamp_(0, BINS - 1).long()
            idx.append(u)
            keep = ok if keep is None else keep & ok
            del x, ok, u
        flat = (idx[0] * BINS + idx[1])[keep]
        out.append(torch.bincount(flat, minlength=BINS * BINS).view(BINS, BINS))
        del idx, keep, flat
    return torch.stack(out)


def torch_cov(hist):
    return torch.cov(hist.reshape(-1, hist.shape[2]).double().T)


def event_ms(launch, warmup, repeats):
    out = []
    for i in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(e0.elapsed_time(e1))
    return out


def stats(ts, unit):
    return {unit: ts, "median_" + unit: statistics.median(ts), "spread_" + unit: max(ts) - min(ts)}


def measure(hist, a):
    n, c, d = hist.shape
    history_bytes = hist.numel() * 4
    pairs = [(i, j) for i in range(d) for j in range(i + 1, d)]
    res = {"rows": n, "chains": c, "theta_dim": d, "pairs": len(pairs), "history_bytes": history_bytes,
           "one_read_at_hbm_sustained_ms": history_bytes / HBM_SUSTAINED * 1e3}
    first = D.histogram2d(hist, bins=BINS)
    lo, hi = first.edges[:, 0].copy(), first.edges[:, -1].copy()
    runs = {"histogram2d": lambda: D.histogram2d(hist, bins=BINS).counts,
            "torch_bincount": lambda: torch_histogram2d(hist, pairs, lo, hi).cpu().numpy(),
            "covariance": lambda: D.covariance(hist), "torch_cov": lambda: torch_cov(hist).cpu().numpy()}
    results, peak, refused = {}, {}, {}
    for name, fn in list(runs.items()):
        try:
            for _ in range(a.warmup - 1):
                clocked(fn)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            first_s, results[name] = clocked(fn)
            peak[name] = torch.cuda.max_memory_allocated() - before
            print("# d = %d %s: %.4f s" % (d, name, first_s), file=sys.stderr, flush=True)
        except Exception as e:          # noqa: BLE001 -- an out-of-memory error is a result here
            refused[name] = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:300])
            del runs[name]
            torch.cuda.empty_cache()
    times = {k: [] for k in runs}
    for _ in range(a.repeats):
        for name, fn in runs.items():
            times[name].append(clocked(fn)[0])
    for name, ts in times.items():
        res[name] = dict(stats(ts, "s"), peak_extra_device_bytes=peak[name])
    res["refused"] = refused
    for ours, other in (("histogram2d", "torch_bincount"), ("covariance", "torch_cov")):
        if ours in times and other in times:
            k, o = res[ours], res[other]
            res["%s_over_%s" % (other, ours)] = o["median_s"] / k["median_s"]
            res["%s_beats_%s_by_more_than_the_spread" % (ours, other)] = bool(o["median_s"] - k["median_s"] > max(o["spread_s"], k["spread_s"]))
            res["%s_beats_%s_by_more_than_the_spread" % (other, ours)] = bool(k["median_s"] - o["median_s"] > max(o["spread_s"], k["spread_s"]))
    if "torch_bincount" in results:
        res["counts_equal_torch"] = bool(np.array_equal(results["histogram2d"].astype(np.int64), results["torch_bincount"]))
    if "torch_cov" in results:
        sd = np.sqrt(np.diag(results["torch_cov"]))
        res["covariance_minus_torch_in_eps_sd_sd"] = float((np.abs(results["covariance"] - results["torch_cov"]) /
                                                            (np.finfo(np.float64).eps * np.outer(sd, sd))).max())
    res["covariance_value"] = np.asarray(results["covariance"]).tolist() if "covariance" in results else None

    # each kernel alone, device events around the entry point
    cm = D._chain_major(hist, "rows")
    lib = _capi.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = np.ascontiguousarray(pairs, np.int32)
    counts = torch.zeros(len(pairs), BINS * BINS + 2, dtype=torch.int64, device=hist.device)

    def launch():
        counts.zero_()
        _capi.check(lib.glabc_histogram2d(cm.data_ptr(), n, d, c, c, len(pairs), table.ctypes.data, BINS, lo.ctypes.data, hi.ctypes.data,
                                          counts.data_ptr(), stream), "glabc_histogram2d")
    zero_ms = statistics.median(event_ms(counts.zero_, a.warmup, a.repeats))
    ms = event_ms(launch, a.warmup, a.repeats)
    want = counts.cpu().numpy().copy()
    med = statistics.median(ms)
    entry = dict(stats(ms, "ms"), lds_bytes=4 * (BINS * BINS + 2), cells_hit_per_pair=(want[:, :-2] > 0).sum(axis=1).tolist(),
                 zeroing_the_counts_ms=zero_ms, one_read_of_the_history_over_kernel_time_as_a_fraction_of_hbm_sustained=history_bytes /
                 ((med - zero_ms) * 1e-3) / HBM_SUSTAINED)
    res["glabc_histogram2d"] = entry
    mean = torch.empty(d, c, dtype=torch.float64, device=hist.device)
    cov = torch.empty(d * (d + 1) // 2, c, dtype=torch.float64, device=hist.device)
    ms = event_ms(lambda: _capi.check(lib.glabc_cross_moments(cm.data_ptr(), n, d, c, c, mean.data_ptr(), cov.data_ptr(), stream),
                                      "glabc_cross_moments"), a.warmup, a.repeats)
    res["glabc_cross_moments"] = dict(stats(ms, "ms"), one_read_of_the_history_over_kernel_time_as_a_fraction_of_hbm_sustained=history_bytes /
                                      (statistics.median(ms) * 1e-3) / HBM_SUSTAINED)
    print("# d = %d kernels: histogram2d %.3f ms, cross_moments %.3f ms" % (d, med, statistics.median(ms)), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"workload": "diagnostics.histogram2d(history, bins=%d) and diagnostics.covariance(history) of histories on the device" % BINS,
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup,
           "hbm_sustained_bytes_per_s": HBM_SUSTAINED}
    lp = g.DiagGaussian(2, torch.zeros(1, 2), torch.log(torch.tensor([0.35, 0.35])))
    ip = g.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.log(torch.tensor([1.6, 1.6])))
    gen = torch.Generator().manual_seed(1234)
    th0 = torch.randn(a.chains, 2, generator=gen)
    y0 = th0.abs() + (0.05 ** 0.5) * torch.randn(a.chains, 2, generator=gen)
    hist = g.GLMCMC(Mixture_set(0.05), a.iters, th0, y0, lp, None, 0.9, ip, 5, seed=20261019, verbose=False, return_device=True)
    res["d2_glmcmc_mixture"] = measure(hist, a)
    del hist
    torch.cuda.empty_cache()
    dgen = torch.Generator(device="cuda").manual_seed(5678)
    rows = max(1, a.iters // 4)
    z = torch.randn(rows, 8, a.chains, generator=dgen, device="cuda")                 # chain-major, correlated through a running sum
    hist8 = torch.cumsum(z, dim=1).mul_(0.5).permute(0, 2, 1)
    del z
    res["d8_synthetic"] = measure(hist8, a)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
