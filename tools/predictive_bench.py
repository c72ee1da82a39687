"""The posterior predictive check of a many-chain history that stays on the GPU: whole calls of
  (a) predictive.check(Model, history, bins=64, range=explicit)      one glabc_predictive_counts launch, the draws in registers,
  (b) the composed path, built from entry points that were there before the kernel: the history transposed to row-major points ->
      glabc_model_simulate(eps = NULL, seed ^ GLABC_PREDICTIVE_KEY) -> glabc_model_discrepancy -> y transposed to chain-major ->
      glabc_histogram of y and of the distances over the same range, and torch comparisons for the tails,
on what GLMCMC on Mixture_set returns with return_device=True (65 536 chains x 2000 iterations, theta_dim 2).  Both sides make the
same draws (ids t * chains + c), so their counts and tails must be equal integers; that is checked.  Timed with a host clock that
ends in a device synchronise; after the warm-ups the paths alternate in one process; the median and the spread (max - min) of the
repeats are reported, and one path beats the other only if the medians differ by more than both spreads.  Peak extra device memory is
torch.cuda.max_memory_allocated over a call.  The kernel is then timed alone with device events -- counts and tails, each output
alone, and the extremes-and-tails pass of range=None -- and set against one read of the history at the sustained HBM rate and
against glabc_histogram of the same history, a kernel of the same skeleton that only reads and counts.

    python tools/predictive_bench.py [--chains 65536] [--iters 2000] [--repeats 7] [--out profiles/predictive_bench.json]
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
from glabcmcmc_amd import _capi, predictive  # noqa: E402
from glabcmcmc_amd import diagnostics as D  # noqa: E402
from glabcmcmc_amd.examples.Mixture import Mixture_set  # noqa: E402

HBM_SUSTAINED = 6.29e12           # bytes per second the part sustains on a copy
BINS = 64
SEED = 20261020


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


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


def composed(desc, hist, lim, thr):
    """(T, C, D) device view of a chain-major buffer -> (counts int64 [K][BINS + 3], tails int64 [K][4])"""
    lib = _capi.lib()
    n, c, d = hist.shape
    yd, total = desc.y_dim, n * c
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    theta = hist.reshape(total, d).contiguous()                                       # the transpose: row-major points
    y = torch.empty(total, yd, dtype=torch.float32, device=hist.device)
    _capi.check(lib.glabc_model_simulate(C.byref(desc), theta.data_ptr(), None, total, SEED ^ predictive.PREDICTIVE_KEY, 0, y.data_ptr(), stream),
                "glabc_model_simulate")
    del theta
    dis = torch.empty(total, dtype=torch.float32, device=hist.device)
    _capi.check(lib.glabc_model_discrepancy(C.byref(desc), y.data_ptr(), total, dis.data_ptr(), stream), "glabc_model_discrepancy")
    y_cm = y.view(n, c, yd).permute(0, 2, 1).contiguous()                             # what glabc_histogram reads
    del y
    counts = torch.zeros(yd + 1, BINS + 3, dtype=torch.int64, device=hist.device)
    lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
    _capi.check(lib.glabc_histogram(y_cm.data_ptr(), n, yd, c, c, BINS, lo.ctypes.data, hi.ctypes.data, counts.data_ptr(), stream), "glabc_histogram")
    _capi.check(lib.glabc_histogram(dis.data_ptr(), n, 1, c, c, BINS, lo[yd:].ctypes.data, hi[yd:].ctypes.data, counts[yd:].data_ptr(), stream),
                "glabc_histogram")
    tails = torch.empty(yd + 1, 4, dtype=torch.int64, device=hist.device)
    for k in range(yd + 1):
        x = y_cm[:, k] if k < yd else dis
        t = float(thr[k])
        tails[k, 0], tails[k, 1], tails[k, 2], tails[k, 3] = (x < t).sum(), (x == t).sum(), (x > t).sum(), torch.isnan(x).sum()
    return counts.cpu().numpy(), tails.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"workload": "predictive.check(Mixture_set(0.05), history, bins=%d, range=explicit) of a GLMCMC history on the device" % BINS,
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup,
           "hbm_sustained_bytes_per_s": HBM_SUSTAINED}
    Model = Mixture_set(0.05)
    desc = Model.descriptor()
    lp = g.DiagGaussian(2, torch.zeros(1, 2), torch.log(torch.tensor([0.35, 0.35])))
    ip = g.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.log(torch.tensor([1.6, 1.6])))
    gen = torch.Generator().manual_seed(1234)
    th0 = torch.randn(a.chains, 2, generator=gen)
    y0 = th0.abs() + (0.05 ** 0.5) * torch.randn(a.chains, 2, generator=gen)
    hist = g.GLMCMC(Model, a.iters, th0, y0, lp, None, 0.9, ip, 5, seed=20261019, verbose=False, return_device=True)
    n, c, d = hist.shape
    history_bytes = hist.numel() * 4
    res.update(rows=n, chains=c, theta_dim=d, history_bytes=history_bytes, one_read_at_hbm_sustained_ms=history_bytes / HBM_SUSTAINED * 1e3)
    lim = np.array([[0.0, 3.0], [0.0, 3.0], [0.0, 2.0]])
    thr = predictive._thresholds(Model, None, 3, True)

    def fused():
        t = predictive.terms(Model, hist, bins=BINS, range=lim, seed=SEED)
        return t.counts.astype(np.int64), t.tails.astype(np.int64)

    runs = {"check": fused, "composed": lambda: composed(desc, hist, lim, thr)}
    results, peak, times = {}, {}, {k: [] for k in runs}
    for name, fn in runs.items():
        for _ in range(a.warmup - 1):
            clocked(fn)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        first_s, results[name] = clocked(fn)
        peak[name] = torch.cuda.max_memory_allocated() - before
        print("# %s: %.4f s" % (name, first_s), file=sys.stderr, flush=True)
    for _ in range(a.repeats):
        for name, fn in runs.items():
            times[name].append(clocked(fn)[0])
    for name, ts in times.items():
        res[name] = dict(stats(ts, "s"), peak_extra_device_bytes=peak[name])
    k, o = res["check"], res["composed"]
    res["composed_over_check"] = o["median_s"] / k["median_s"]
    res["check_beats_composed_by_more_than_the_spread"] = bool(o["median_s"] - k["median_s"] > max(o["spread_s"], k["spread_s"]))
    res["composed_beats_check_by_more_than_the_spread"] = bool(k["median_s"] - o["median_s"] > max(o["spread_s"], k["spread_s"]))
    res["counts_equal"] = bool(np.array_equal(results["check"][0], results["composed"][0]))
    res["tails_equal"] = bool(np.array_equal(results["check"][1], results["composed"][1]))
    res["draws_counted"] = int(results["check"][1][0].sum())
    s = predictive.summary(predictive.Terms(n * c, results["check"][0], results["check"][1], lim, thr, True))
    res["p_upper"], res["within_epsilon"] = s.p_upper.tolist(), s.within_epsilon

    # the kernel alone, device events around the entry point
    cm = D._chain_major(hist, "rows")
    assert cm.data_ptr() == hist.data_ptr()                                            # in place
    lib = _capi.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    counts = torch.zeros(3, BINS + 3, dtype=torch.int64, device=hist.device)
    tails = torch.zeros(3, 4, dtype=torch.int64, device=hist.device)
    extremes = torch.from_numpy(np.array([predictive.KEY_NONE] * 3, np.uint32).view(np.int32)).to(hist.device)
    lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])

    def kernel(want):
        p = lambda name, t: t.data_ptr() if name in want else None          # noqa: E731
        return lambda: _capi.check(lib.glabc_predictive_counts(
            C.byref(desc), cm.data_ptr(), n, d, c, c, SEED, 0, c, BINS, lo.ctypes.data, hi.ctypes.data, thr.ctypes.data, p("counts", counts),
            p("tails", tails), p("extremes", extremes), stream), "glabc_predictive_counts")
    res["glabc_predictive_counts"] = {}
    for want in (("counts", "tails"), ("counts",), ("tails",), ("tails", "extremes"), ("counts", "tails", "extremes")):
        ms = event_ms(kernel(want), a.warmup, a.repeats)
        med = statistics.median(ms)
        res["glabc_predictive_counts"]["+".join(want)] = dict(
            stats(ms, "ms"), draws_per_s=n * c / (med * 1e-3),
            one_read_of_the_history_over_kernel_time_as_a_fraction_of_hbm_sustained=history_bytes / (med * 1e-3) / HBM_SUSTAINED)
        print("# kernel %s: %.3f ms" % ("+".join(want), med), file=sys.stderr, flush=True)
    hcounts = torch.zeros(d, BINS + 3, dtype=torch.int64, device=hist.device)
    ms = event_ms(lambda: _capi.check(lib.glabc_histogram(cm.data_ptr(), n, d, c, c, BINS, lo.ctypes.data, hi.ctypes.data, hcounts.data_ptr(), stream),
                                      "glabc_histogram"), a.warmup, a.repeats)
    res["glabc_histogram_of_the_same_history"] = dict(
        stats(ms, "ms"), one_read_of_the_history_over_kernel_time_as_a_fraction_of_hbm_sustained=history_bytes / (statistics.median(ms) * 1e-3) / HBM_SUSTAINED)
    y = torch.empty(n, d, c, dtype=torch.float32, device=hist.device)
    dis = torch.empty(n, c, dtype=torch.float32, device=hist.device)
    ms = event_ms(lambda: _capi.check(lib.glabc_predictive_draws(C.byref(desc), cm.data_ptr(), n, d, c, c, SEED, 0, c, y.data_ptr(), c, dis.data_ptr(),
                                                                 c, stream), "glabc_predictive_draws"), a.warmup, a.repeats)
    res["glabc_predictive_draws"] = dict(stats(ms, "ms"), bytes_moved=history_bytes + y.numel() * 4 + dis.numel() * 4,
                                         bytes_moved_over_kernel_time_as_a_fraction_of_hbm_sustained=(history_bytes + y.numel() * 4 + dis.numel() * 4) /
                                         (statistics.median(ms) * 1e-3) / HBM_SUSTAINED)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
