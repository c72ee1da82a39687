"""Summaries of weighted draws that stay on the GPU: whole calls of
  (a) weighted.quantile(draws, (0.025, 0.5, 0.975))          three glabc_weighted_key_counts passes and the host's walk of the counts,
  (b) the torch composition a user would write today: torch.sort per coordinate, a gather of the weights, cumsum, searchsorted,
  (c) weighted.histogram2d(draws, bins=64) under an explicit range, one glabc_weighted_histogram2d launch,
  (d) torch: the bins of both coordinates, then torch.bincount with the weights,
timed with a host clock that ends in a device synchronise, on two inputs: the rows regression.adjust keeps of
rejection.sample(GK_set, 2^24 draws, kernel="hard", quantile=0.1) with its kernel weights (1.7e6 rows x 4 coordinates), and a
65 536-particle population with Dirichlet-like weights (2 coordinates).  After the warm-ups the paths alternate in one process; the median
and the spread (max - min) of the repeats are reported, and one path beats the other only if the medians differ by more than both
spreads.  No ratio is expected: the inputs are small and both sides are near launch and synchronisation latency.  The torch paths
weight with float64 sums, so their results are neither exact nor reproducible to the bit; the largest difference to (a) / (c) is
recorded.  Peak extra device memory is torch.cuda.max_memory_allocated over a call.  Each kernel is timed alone with device
events, on the prefixes the selection walked.

    python tools/weighted_bench.py [--draws 16777216] [--particles 65536] [--repeats 7] [--out profiles/weighted_bench.json]
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
from glabcmcmc_amd import _capi, regression, rejection, weighted  # noqa: E402
from glabcmcmc_amd import diagnostics as D  # noqa: E402
from glabcmcmc_amd.examples.GK import GK_set  # noqa: E402

QS = (0.025, 0.5, 0.975)
BINS = 64


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def torch_quantile(theta, w):
    """the inverted weighted distribution function by a sort: float64 cumulative weights, so a rank at a tie of the sums may differ"""
    out = np.empty((len(QS), theta.shape[1]))
    q = torch.tensor(QS, dtype=torch.float64, device=theta.device)
    for j in range(theta.shape[1]):
        s, order = torch.sort(theta[:, j])
        cum = torch.cumsum(w[order].double(), 0)
        at = torch.searchsorted(cum, q * cum[-1]).clamp(max=theta.shape[0] - 1)
        out[:, j] = s[at].double().cpu().numpy()
    return out


def torch_histogram2d(theta, w, pairs, lo, hi):
    """numpy.histogram2d's bins in torch float64 and a weighted bincount; draws outside the range are dropped"""
    grids = []
    for a, b in pairs:
        idx = []
        for j in (a, b):
            x = theta[:, j].double()
            k = torch.floor((x - lo[j]) * (BINS / (hi[j] - lo[j]))).long().clamp(max=BINS - 1)
            idx.append(torch.where((x >= lo[j]) & (x <= hi[j]), k, torch.full_like(k, -1)))
        keep = (idx[0] >= 0) & (idx[1] >= 0)
        grids.append(torch.bincount((idx[0] * BINS + idx[1])[keep], weights=w[keep].double(), minlength=BINS * BINS))
    return torch.stack(grids).cpu().numpy().reshape(len(pairs), BINS, BINS)


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


def measure(name, theta, w, a):
    n, d = theta.shape
    draws = (theta, w)
    m, scale = weighted.quantize(w)
    lim = weighted._exact_range(weighted._Prepared(draws, None, "fused"))
    lo, hi = lim[:, 0].tolist(), lim[:, 1].tolist()
    pairs = [(i, j) for i in range(d) for j in range(i + 1, d)]
    res = {"draws": n, "dim": d, "scale": scale, "M": int(m.sum()), "ess": weighted.summary(draws)["ess"], "pairs": len(pairs)}
    runs = {"weighted_quantile": lambda: weighted.quantile(draws, QS), "torch_sort_cumsum": lambda: torch_quantile(theta, w),
            "weighted_histogram2d": lambda: weighted.histogram2d(draws, pairs, BINS, lim).counts,
            "torch_bincount": lambda: torch_histogram2d(theta, w, pairs, lo, hi)}
    results, peak = {}, {}
    for key, fn in runs.items():
        for _ in range(a.warmup - 1):
            clocked(fn)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        _, results[key] = clocked(fn)
        peak[key] = torch.cuda.max_memory_allocated() - before
    times = {k: [] for k in runs}
    for _ in range(a.repeats):
        for key, fn in runs.items():
            times[key].append(clocked(fn)[0])
    for key, ts in times.items():
        res[key] = {"seconds": ts, "median_s": statistics.median(ts), "spread_s": max(ts) - min(ts), "peak_extra_device_bytes": peak[key]}
    res["weighted_quantile"]["quantiles"] = np.asarray(results["weighted_quantile"]).tolist()
    for ours, theirs in (("weighted_quantile", "torch_sort_cumsum"), ("weighted_histogram2d", "torch_bincount")):
        k, o = res[ours], res[theirs]
        res["%s_over_%s" % (theirs, ours)] = o["median_s"] / k["median_s"]
        gap, spread = o["median_s"] - k["median_s"], max(o["spread_s"], k["spread_s"])
        res["faster_by_more_than_the_spread:%s_or_%s" % (ours, theirs)] = ours if gap > spread else theirs if -gap > spread else "neither"
    res["largest_quantile_difference_to_torch"] = float(np.max(np.abs(np.asarray(results["torch_sort_cumsum"]) - np.asarray(results["weighted_quantile"]))))
    grid = np.asarray(results["weighted_histogram2d"]).astype(np.float64) / scale
    res["largest_relative_cell_difference_to_torch"] = float(np.max(np.abs(results["torch_bincount"] - grid)) / grid.max())
    res["generic_path_gives_the_same_quantiles"] = bool(np.array_equal(weighted.quantile(draws, QS, path="generic"), results["weighted_quantile"]))

    # each kernel alone: device events around the launch, on the prefixes the selection walked
    p = weighted._Prepared(draws, None, "fused")
    tables = {}

    def recording(level, table):
        tables[level] = np.zeros((d, 1), np.uint32) if table is None else np.ascontiguousarray(table[:, :D.MAX_PREFIXES])
        return weighted._key_counts(p, level, tables[level])
    weighted._quantile(recording, np.array(QS))
    lib = _capi.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res["kernels"] = {}

    def timed(label, counts, launch, lds_bytes, bytes_read):
        def run():
            counts.zero_()
            launch()
        zero_ms = statistics.median(event_ms(counts.zero_, a.warmup, a.repeats))
        ms = event_ms(run, a.warmup, a.repeats)
        res["kernels"][label] = {"lds_bytes": lds_bytes, "milliseconds": ms, "median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms),
                                 "zeroing_the_counts_ms": zero_ms, "bytes_read": bytes_read}
    for level in (0, 1, 2):
        table = tables[level]
        k, bins = table.shape[1], 1 << D.KEY_LEVELS[level][1]
        counts = torch.zeros(d, k, bins, dtype=torch.int64, device=theta.device)
        timed("key_counts_level_%d" % level, counts,
              lambda: _capi.check(lib.glabc_weighted_key_counts(p.x.data_ptr(), p.stride, d, p.w.data_ptr(), n, scale, level, k, table.ctypes.data,
                                                                counts.data_ptr(), stream), "glabc_weighted_key_counts"), 8 * k * bins, 8 * n * d)
    los, his = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
    counts = torch.zeros(d, BINS + 3, dtype=torch.int64, device=theta.device)
    timed("histogram_%d_bins" % BINS, counts,
          lambda: _capi.check(lib.glabc_weighted_histogram(p.x.data_ptr(), p.stride, d, p.w.data_ptr(), n, scale, BINS, los.ctypes.data, his.ctypes.data,
                                                           counts.data_ptr(), stream), "glabc_weighted_histogram"), 8 * (BINS + 3), 8 * n * d)
    table = np.ascontiguousarray(pairs, np.int32)
    for bins in (BINS, D.MAX_JOINT_BINS):
        counts2 = torch.zeros(len(pairs), bins * bins + 2, dtype=torch.int64, device=theta.device)
        timed("histogram2d_%d_bins" % bins, counts2,
              lambda: _capi.check(lib.glabc_weighted_histogram2d(p.x.data_ptr(), p.stride, d, p.w.data_ptr(), n, scale, len(pairs), table.ctypes.data, bins,
                                                                 los.ctypes.data, his.ctypes.data, counts2.data_ptr(), stream),
                                  "glabc_weighted_histogram2d"), 8 * (bins * bins + 2), 12 * n * len(pairs))
    print("# %s: quantile %.3f ms against %.3f ms, histogram2d %.3f ms against %.3f ms" % (
        name, 1e3 * res["weighted_quantile"]["median_s"], 1e3 * res["torch_sort_cumsum"]["median_s"],
        1e3 * res["weighted_histogram2d"]["median_s"], 1e3 * res["torch_bincount"]["median_s"]), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=1 << 24)
    ap.add_argument("--quantile", type=float, default=0.1)
    ap.add_argument("--particles", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    model = GK_set(0.5)
    kept = rejection.sample(model, a.draws, kernel="hard", quantile=a.quantile, seed=20261020)
    adjusted = regression.adjust(model, kept)
    res = {"workload": "weighted.quantile(draws, %r) and weighted.histogram2d(draws, bins=%d) against the torch composition" % (QS, BINS),
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup}
    res["adjusted_gk_rows"] = measure("adjusted g-and-k rows", adjusted.theta, adjusted.weights.to(torch.float32), a)
    gen = torch.Generator().manual_seed(1234)
    theta = torch.randn(a.particles, 2, generator=gen).abs_().mul_(torch.tensor([1.0, -1.0])).add_(1.5).cuda()
    w = torch.rand(a.particles, generator=gen).log_().neg_()
    res["population"] = measure("population", theta, (w / w.sum()).to(torch.float32).cuda(), a)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
