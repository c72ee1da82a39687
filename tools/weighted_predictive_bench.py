"""Posterior predictive checks of weighted draws: whole calls of
  (a) predictive.check_weighted(Model, draws, bins=64, range=explicit)     one glabc_weighted_predictive_counts launch (a CompiledModel:
      glabc_rtc_weighted_predictive_counts), the draws kept in registers,
  (b) the composition a user could write before it: predictive.simulate materialises y_rep and the distances, weighted.histogram of
      the K = y_dim + 1 statistics under the same range and scale counts them, and torch sums the multiplicities of the four tails,
timed with a host clock that ends in a device synchronise, on populations of 65 536 and 2^21 draws of Mixture_set and 4096
particles of the compiled Lotka-Volterra Model (constant-ish theta near the posterior, Dirichlet-like weights: the cost does not
depend on the values).  After the warm-ups the two paths alternate in one process; the median and the spread (max - min) of the
repeats are reported, and one path beats the other only if the medians differ by more than both spreads.  No ratio is expected in
advance: calls of this size are host work and launch latency (tools/weighted_bench.py).  Both paths count the very same draws, so
their integer tables are asserted equal.  Peak extra device memory is torch.cuda.max_memory_allocated over a call.

The kernel alone, under device events, next to glabc_predictive_counts on the same one-row history with unit weights: its cost over
the unweighted twin is the price of the 64-bit counters and the weight load.

    python tools/weighted_predictive_bench.py [--repeats 7] [--out profiles/weighted_predictive_bench.json]
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
from glabcmcmc_amd import engine, predictive, weighted  # noqa: E402
from glabcmcmc_amd.examples import LotkaVolterra_smc  # noqa: E402
from glabcmcmc_amd.examples.Mixture import Mixture_set  # noqa: E402
from glabcmcmc_amd.regression import _dimension_major  # noqa: E402

BINS = 64
SEED = 20261021


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def composed(Model, theta, w, lim, thr, scale):
    """-> (counts uint64 [K][BINS + 3], tails uint64 [K][4]) through the entry points of the parent commit"""
    y, dis = predictive.simulate(Model, theta, seed=SEED, row0=0)
    stats = torch.cat([y, dis[:, None]], dim=1)
    parts = []
    for k0 in range(0, stats.shape[1], 8):                         # weighted.histogram takes at most 8 coordinates
        h = weighted.histogram((stats[:, k0:k0 + 8], w), bins=BINS, range=lim[k0:k0 + 8], scale=scale)
        parts.append(np.concatenate([h.counts, h.below[:, None], h.above[:, None], h.nan[:, None]], axis=1))
    counts = np.concatenate(parts)
    m = weighted._multiplicity(w, scale)
    t = torch.as_tensor(thr, device=stats.device)
    zero = torch.zeros_like(m)
    tails = torch.stack([torch.where(stats < t, m[:, None], zero[:, None]).sum(0), torch.where(stats == t, m[:, None], zero[:, None]).sum(0),
                         torch.where(stats > t, m[:, None], zero[:, None]).sum(0), torch.where(torch.isnan(stats), m[:, None], zero[:, None]).sum(0)], dim=1)
    return counts, tails.cpu().numpy().view(np.uint64)


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


def measure(name, Model, theta, w, lim, a):
    n, d = theta.shape
    k = int(Model.y_dim) + 1
    lim = np.asarray(lim, np.float64)
    thr = predictive._thresholds(Model, None, k, True)
    scale = weighted.quantize(w)[1]
    res = {"draws": n, "theta_dim": d, "statistics": k, "scale": scale, "ess": weighted.summary((theta, w))["ess"]}
    runs = {"check_weighted": lambda: predictive.terms_weighted(Model, (theta, w), bins=BINS, range=lim, seed=SEED, scale=scale),
            "composed": lambda: composed(Model, theta, w, lim, thr, scale)}
    results, peak = {}, {}
    for key, fn in runs.items():
        for _ in range(a.warmup - 1):
            clocked(fn)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        _, results[key] = clocked(fn)
        peak[key] = torch.cuda.max_memory_allocated() - before
    t = results["check_weighted"]
    assert np.array_equal(t.counts, results["composed"][0]) and np.array_equal(t.tails, results["composed"][1]), "the two paths disagree"
    res["equal_integers"], res["M"] = True, int(t.n)
    times = {key: [] for key in runs}
    for _ in range(a.repeats):
        for key, fn in runs.items():
            times[key].append(clocked(fn)[0])
    for key, ts in times.items():
        res[key] = {"seconds": ts, "median_s": statistics.median(ts), "spread_s": max(ts) - min(ts), "peak_extra_device_bytes": peak[key]}
    ours, theirs = res["check_weighted"], res["composed"]
    res["composed_over_check_weighted"] = theirs["median_s"] / ours["median_s"]
    gap, spread = theirs["median_s"] - ours["median_s"], max(theirs["spread_s"], ours["spread_s"])
    res["faster_by_more_than_both_spreads"] = "check_weighted" if gap > spread else "composed" if -gap > spread else "neither"

    # the kernel alone next to the unweighted twin on the same one-row history, unit weights
    fused_w, fused_u = predictive._path_weighted(Model, theta, "fused"), predictive._path(Model, theta, "fused")
    x, stride = _dimension_major(theta)
    ones = torch.ones(n, device=theta.device)
    lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
    counts = torch.zeros(k, BINS + 3, dtype=torch.int64, device=theta.device)
    tails = torch.zeros(k, 4, dtype=torch.int64, device=theta.device)
    stream = predictive._stream(theta.device)
    key = engine.draw_seed(SEED)

    def zero():
        counts.zero_()
        tails.zero_()

    def weighted_launch(wt):
        zero()
        fused_w.counts(x.data_ptr(), stride, d, wt.data_ptr(), n, 1.0 if wt is ones else scale, key, 0, BINS, lo.ctypes.data, hi.ctypes.data,
                       thr.ctypes.data, counts.data_ptr(), tails.data_ptr(), None, stream)

    def unweighted_launch():
        zero()
        fused_u.counts(x.data_ptr(), 1, d, n, stride, key, 0, n, BINS, lo.ctypes.data, hi.ctypes.data, thr.ctypes.data, counts.data_ptr(),
                       tails.data_ptr(), None, stream)

    res["kernels"] = {}
    for label, launch in (("zeroing_the_tables", zero), ("weighted_kernel_unit_weights", lambda: weighted_launch(ones)),
                          ("weighted_kernel_population_weights", lambda: weighted_launch(w)), ("unweighted_twin", unweighted_launch)):
        ms = event_ms(launch, a.warmup, a.repeats)
        res["kernels"][label] = {"milliseconds": ms, "median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms)}
    weighted_launch(ones)
    unit = counts.clone(), tails.clone()
    unweighted_launch()
    assert torch.equal(unit[0], counts) and torch.equal(unit[1], tails), "unit weights do not give the twin's tables"
    print("# %s: check_weighted %.3f ms against composed %.3f ms; kernel %.4f ms, twin %.4f ms" % (
        name, 1e3 * ours["median_s"], 1e3 * theirs["median_s"], res["kernels"]["weighted_kernel_unit_weights"]["median_ms"],
        res["kernels"]["unweighted_twin"]["median_ms"]), file=sys.stderr, flush=True)
    return res


def population(n, centre, spread, gen):
    theta = (torch.tensor(centre) + torch.tensor(spread) * torch.randn(n, len(centre), generator=gen)).to(torch.float32).cuda()
    w = torch.rand(n, generator=gen).clamp_(min=2.0 ** -24).log_().neg_()          # rand may return 0: no infinite weight
    return theta, (w / w.sum()).to(torch.float32).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"workload": "predictive.check_weighted(Model, draws, bins=%d, range=explicit) against predictive.simulate -> weighted.histogram + torch tails" % BINS,
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup}
    gen = torch.Generator().manual_seed(1234)
    mixture = Mixture_set(0.05)
    lim2 = [(-1.0, 4.0), (-1.0, 4.0), (0.0, 3.0)]
    for n in (65536, 1 << 21):
        theta, w = population(n, [1.5, 1.5], [0.2, 0.2], gen)
        res["mixture_%d" % n] = measure("Mixture_set, %d draws" % n, mixture, theta, w, lim2, a)
    lv = LotkaVolterra_smc.build()
    theta, w = population(4096, [1.0, 1.0], [0.05, 0.05], gen)
    res["lotka_volterra_4096"] = measure("Lotka-Volterra (compiled), 4096 particles", lv, theta, w, [(-2.0, 6.0)] * 8 + [(0.0, 10.0)], a)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
