"""Posterior quantiles of a many-chain history that stays on the GPU: whole calls of
  (a) diagnostics.quantile(history, (0.025, 0.5, 0.975))      three glabc_key_counts passes and the host's walk of the counts,
  (b) torch.sort of each coordinate's flattened values, then the same interpolation,
  (c) torch.kthvalue per rank and coordinate, then the same interpolation,
  (d) torch.quantile per coordinate (it refuses inputs of this size: what it says is recorded),
timed with a host clock that ends in a device synchronise.  The history is what GLMCMC on Mixture_set returns with
return_device=True.  After a warm-up of each, the paths alternate in one process; the median and the spread (max - min) of the
repeats are reported, and (a) beats another path only if the medians differ by more than both spreads.  A path that raises (out
of memory, a refusal) is recorded with its message and left out.  Peak extra device memory is torch.cuda.max_memory_allocated
over a call.  Each level's glabc_key_counts launch is timed alone with device events, on the prefixes the selection walked, and
set against one read of the history at the sustained HBM rate; with --modes-lib (tools/ubench/quant_modes.hip) every contention
mode of the counting kernel is timed the same way at every level, and must give the library's counts.

    python tools/quantile_bench.py [--chains 65536] [--iters 2000] [--repeats 7] [--modes-lib tools/ubench/libquant_modes.so]
                                   [--out profiles/quantile_bench.json]
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
QS = (0.025, 0.5, 0.975)
MODES = ("direct", "runs")          # csrc/glabc_quant.hip CountMode
SLOW_CALL_S = 5.0                 # a path whose call takes longer is timed with 3 repeats and no further warm-up
TOO_SLOW_S = 30.0                 # ... and past this its first call is all that is recorded


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def ranks_and_weights(n):
    h = np.array(QS) * (n - 1.0)
    lo = np.floor(h).astype(np.int64)
    return lo, np.minimum(lo + 1, n - 1), h - lo


def interpolate(x_lo, x_hi, frac):
    x_lo, x_hi = np.asarray(x_lo, np.float64), np.asarray(x_hi, np.float64)
    return x_lo + frac[:, None] * (x_hi - x_lo)


def sort_quantile(hist):
    t, c, d = hist.shape
    lo, hi, frac = ranks_and_weights(t * c)
    cols = []
    for j in range(d):
        s = torch.sort(hist[:, :, j].reshape(-1)).values
        cols.append(s[torch.as_tensor(np.concatenate([lo, hi]), device=hist.device)].cpu().numpy())
        del s
    x = np.stack(cols, axis=1)
    return interpolate(x[:len(QS)], x[len(QS):], frac)


def kthvalue_quantile(hist):
    t, c, d = hist.shape
    lo, hi, frac = ranks_and_weights(t * c)
    x = np.empty((2 * len(QS), d), np.float32)
    for j in range(d):
        flat = hist[:, :, j].reshape(-1)
        for i, r in enumerate(np.concatenate([lo, hi])):
            x[i, j] = float(torch.kthvalue(flat, int(r) + 1).values)
        del flat
    return interpolate(x[:len(QS)], x[len(QS):], frac)


def torch_quantile(hist):
    q = torch.tensor(QS, dtype=hist.dtype, device=hist.device)
    return np.stack([torch.quantile(hist[:, :, j].reshape(-1), q).cpu().numpy().astype(np.float64) for j in range(hist.shape[2])], axis=1)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--modes-lib", default=None)
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
    res = {"workload": "diagnostics.quantile(history, %r) of a GLMCMC history on Mixture_set (return_device=True)" % (QS,),
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "chains": c, "rows": n, "theta_dim": d,
           "repeats": a.repeats, "history_bytes": history_bytes, "hbm_sustained_bytes_per_s": HBM_SUSTAINED,
           "one_read_at_hbm_sustained_ms": history_bytes / HBM_SUSTAINED * 1e3}

    runs = {"selection": lambda: D.quantile(hist, QS), "torch_sort": lambda: sort_quantile(hist),
            "torch_kthvalue": lambda: kthvalue_quantile(hist), "torch_quantile": lambda: torch_quantile(hist)}
    results, peak, repeats, refused = {}, {}, {}, {}
    for name, fn in list(runs.items()):
        try:
            first, _ = clocked(fn)
            print("# %s: first call %.3f s" % (name, first), file=sys.stderr, flush=True)
            if first > TOO_SLOW_S:
                raise TimeoutError("the first call took %.1f s" % first)
            slow = first > SLOW_CALL_S
            for _ in range(0 if slow else a.warmup - 1):
                clocked(fn)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            _, results[name] = clocked(fn)
            peak[name] = torch.cuda.max_memory_allocated() - before
            repeats[name] = 3 if slow else a.repeats
        except Exception as e:          # noqa: BLE001 -- a refusal or an out-of-memory error is a result here
            refused[name] = "%s: %s" % (type(e).__name__, str(e).splitlines()[0][:300])
            del runs[name]
            torch.cuda.empty_cache()
    times = {k: [] for k in runs}
    for i in range(a.repeats):
        for name, fn in runs.items():
            if i < repeats[name]:
                times[name].append(clocked(fn)[0])
    for name, ts in times.items():
        res[name] = {"seconds": ts, "median_s": statistics.median(ts), "spread_s": max(ts) - min(ts), "peak_extra_device_bytes": peak[name],
                     "quantiles": np.asarray(results[name]).tolist()}
    res["refused"] = refused
    k = res["selection"]
    for other in times:
        if other != "selection":
            o = res[other]
            res["selection_over_" + other] = o["median_s"] / k["median_s"]
            res["selection_beats_%s_by_more_than_the_spread" % other] = bool(o["median_s"] - k["median_s"] > max(o["spread_s"], k["spread_s"]))
            res["largest_difference_to_" + other] = float(np.max(np.abs(np.array(o["quantiles"]) - np.array(k["quantiles"]))))

    # each level's launch alone: the prefixes the selection walked, device events around glabc_key_counts
    cm = D._chain_major(hist, "rows")
    tables = {}

    def recording(level, table):
        tables[level] = np.zeros((d, 1), np.uint32) if table is None else np.ascontiguousarray(table[:, :D.MAX_PREFIXES])
        return D._key_counts(cm, level, tables[level])
    D.select(recording, q=QS)
    lib = _capi.lib()
    modes = None
    if a.modes_lib:
        modes = C.CDLL(os.path.abspath(a.modes_lib))
        modes.quant_modes_key_counts.restype = C.c_int
        modes.quant_modes_key_counts.argtypes = [C.c_int] + _capi.ENTRY_POINTS["glabc_key_counts"][1]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res["levels"] = {}
    for level in (0, 1, 2):
        table = tables[level]
        p, bins = table.shape[1], 1 << D.KEY_LEVELS[level][1]
        counts = torch.zeros(d, p, bins, dtype=torch.int64, device=hist.device)

        def launch(fn=lib.glabc_key_counts, head=()):
            counts.zero_()
            _capi.check(fn(*head, cm.data_ptr(), n, d, c, c, level, p, table.ctypes.data, counts.data_ptr(), stream), "glabc_key_counts")
        zero_ms = statistics.median(event_ms(counts.zero_, a.warmup, a.repeats))
        ms = event_ms(launch, a.warmup, a.repeats)
        want = counts.cpu().numpy().copy()
        med = statistics.median(ms)
        entry = {"n_prefixes": p, "lds_bytes": 4 * p * bins, "digits_hit": int((want.sum(axis=(0, 1)) > 0).sum()),
                 "values_counted": int(want.sum()), "milliseconds": ms, "median_ms": med, "spread_ms": max(ms) - min(ms),
                 "zeroing_the_counts_ms": zero_ms,
                 "fraction_of_hbm_sustained": history_bytes / ((med - zero_ms) * 1e-3) / HBM_SUSTAINED}
        if modes is not None:
            for m, name in enumerate(MODES):
                ms = event_ms(lambda: launch(modes.quant_modes_key_counts, (m,)), a.warmup, a.repeats)
                entry["mode_" + name] = {"milliseconds": ms, "median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms),
                                         "counts_equal_the_library": bool(np.array_equal(counts.cpu().numpy(), want))}
        res["levels"]["level_%d" % level] = entry
        print("# level %d: %.3f ms" % (level, med), file=sys.stderr, flush=True)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
