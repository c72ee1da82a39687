"""The posterior predictive check of a CompiledModel on a history that stays on the GPU: whole calls of
predictive.check(bins=64, range=explicit) three ways --
  (a) fused: one glabc_rtc_predictive_counts launch of the run-time compiled predictive_kernel, the draws in registers,
  (b) composed: the entry points that specify a draw (CompiledModel.composed_predictive: per history row glabc_dist_forward ->
      glabc_rtc_simulate -> the distance) and predictive._torch_tables on the materialised statistics; equal tables are required,
  (c) path="generic": generate_samples in chunks, the noise from torch's generator (other draws: no equality to ask for)
-- on two Models: the Mixture restatement on a chains x iters x 2 history (default 65 536 x 2000), with the built-in
glabc_predictive_counts on Mixture_set beside it (the gap is the cost of the user frame), and the Lotka-Volterra Model of
examples/LotkaVolterra_smc.py on a history small enough for the generic call to fit in memory (default 64 rows x 4096 chains).
Host clock ending in a device synchronise; after the warm-ups the paths alternate in one process; medians and spreads (max - min)
are reported.  Peak extra device memory is torch.cuda.max_memory_allocated over a call.  Then the kernel alone (device events,
counts and tails), at the rule R = 1 row per item and at the built-in kernels' R = 16 / D (GLABC_RTC_PRED_ROWS at compile time).

    python tools/rtc_predictive_bench.py [--chains 65536] [--iters 2000] [--repeats 7] [--out profiles/rtc_predictive_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from glabcmcmc_amd import _capi, engine, predictive  # noqa: E402
from glabcmcmc_amd import diagnostics as D  # noqa: E402
from glabcmcmc_amd.compiled import CompiledModel  # noqa: E402
from glabcmcmc_amd.examples import LotkaVolterra_smc  # noqa: E402
from glabcmcmc_amd.examples.Mixture import Mixture_set  # noqa: E402
from test_rtc import mixture_source  # noqa: E402

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


def alternate(runs, warmup, repeats):
    """-> ({name: timing and peak memory}, {name: the last result})"""
    results, peak, times = {}, {}, {k: [] for k in runs}
    for name, fn in runs.items():
        for _ in range(warmup - 1):
            clocked(fn)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        first_s, results[name] = clocked(fn)
        peak[name] = torch.cuda.max_memory_allocated() - before
        print("# %s: %.4f s" % (name, first_s), file=sys.stderr, flush=True)
    for _ in range(repeats):
        for name, fn in runs.items():
            times[name].append(clocked(fn)[0])
    return {name: dict(stats(ts, "s"), peak_extra_device_bytes=peak[name]) for name, ts in times.items()}, results


def three_ways(Model, hist, lim, a, extra=None):
    """hist: (T, C, D) view of a chain-major device buffer"""
    handle, desc = Model.predictive_program(), Model.descriptor()
    cm = D._chain_major(hist, "rows")
    n, d, c = cm.shape
    k = desc.y_dim + 1
    thr = predictive._thresholds(Model, None, k, True)
    key = engine.draw_seed(SEED)

    def fused():
        t = predictive.terms(Model, hist, bins=BINS, range=lim, seed=SEED, path="fused")
        return t.counts.astype(np.int64), t.tails.astype(np.int64)

    def composed():
        y, dis = Model.composed_predictive(handle, desc, cm, key, 0, c)
        st = torch.cat([y.permute(0, 2, 1).reshape(-1, desc.y_dim), dis.reshape(-1, 1)], dim=1)
        del y, dis
        counts, tails = predictive._torch_tables(st, BINS, lim, thr)
        return counts.astype(np.int64), tails.astype(np.int64)

    def generic():
        t = predictive.terms(Model, hist, bins=BINS, range=lim, seed=SEED, path="generic")
        return t.counts.astype(np.int64), t.tails.astype(np.int64)

    runs = {"fused": fused, "composed": composed, "generic": generic}
    if extra:
        runs.update(extra)
    res, out = alternate(runs, a.warmup, a.repeats)
    res["rows"], res["chains"], res["theta_dim"], res["history_bytes"] = n, c, d, cm.numel() * 4
    res["composed_tables_equal_fused"] = bool(np.array_equal(out["fused"][0], out["composed"][0]) and np.array_equal(out["fused"][1], out["composed"][1]))
    res["draws_counted"] = int(out["fused"][1][0].sum())
    for other in runs:
        if other != "fused":
            res[other + "_over_fused"] = res[other]["median_s"] / res["fused"]["median_s"]
    return res, out, (cm, desc, thr)


def kernel_alone(source, dims, desc, cm, lim, thr, rows, a):
    """glabc_rtc_predictive_counts with counts and tails, device events, of a program compiled at `rows` rows per item"""
    lib = _capi.lib()
    os.environ["GLABC_RTC_PRED_ROWS"] = str(rows)
    handle, log = C.c_void_p(), C.create_string_buffer(1 << 14)
    rc = lib.glabc_rtc_compile_predictive(source.encode(), *dims, C.byref(handle), log, len(log))
    del os.environ["GLABC_RTC_PRED_ROWS"]
    assert rc == 0, log.value.decode()
    n, d, c = cm.shape
    k = desc.y_dim + 1
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    counts = torch.zeros(k, BINS + 3, dtype=torch.int64, device=cm.device)
    tails = torch.zeros(k, 4, dtype=torch.int64, device=cm.device)
    lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
    ms = event_ms(lambda: _capi.check(lib.glabc_rtc_predictive_counts(
        handle, C.byref(desc), cm.data_ptr(), n, d, c, c, SEED, 0, c, BINS, lo.ctypes.data, hi.ctypes.data, thr.ctypes.data, counts.data_ptr(),
        tails.data_ptr(), None, stream), "glabc_rtc_predictive_counts"), a.warmup, a.repeats)
    lib.glabc_rtc_release(handle)
    return dict(stats(ms, "ms"), rows_per_item=rows, draws_per_s=n * c / (statistics.median(ms) * 1e-3), compile_log=log.value.decode())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--lv-chains", type=int, default=4096)
    ap.add_argument("--lv-rows", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"workload": "predictive.check(CompiledModel, history, bins=%d, range=explicit): fused, composed entry points, generic" % BINS,
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup}

    # ---- the Mixture restatement, with the built-in kernel beside it
    builtin = Mixture_set(0.05)
    bd = builtin.descriptor()
    source = mixture_source([bd.noise.p2[0], bd.noise.p2[1]])
    Model = CompiledModel(2, 2, source, builtin._prior(), [bd.y_obs[0], bd.y_obs[1]], 0.05)
    gen = torch.Generator().manual_seed(1234)
    buf = (1.4 + 0.3 * torch.randn(a.iters, 2, a.chains, generator=gen)).cuda()          # posterior-like draws, chain-major
    hist = buf.permute(0, 2, 1)
    lim = np.array([[0.0, 3.0], [0.0, 3.0], [0.0, 2.0]])

    def fused_builtin():
        t = predictive.terms(builtin, hist, bins=BINS, range=lim, seed=SEED)
        return t.counts.astype(np.int64), t.tails.astype(np.int64)

    r, out, (cm, desc, thr) = three_ways(Model, hist, lim, a, {"builtin_fused": fused_builtin})
    r["user_frame_tables_equal_builtin"] = bool(np.array_equal(out["fused"][0], out["builtin_fused"][0]) and
                                                np.array_equal(out["fused"][1], out["builtin_fused"][1]))
    r["kernel_alone"] = {"R=1 (the rule)": kernel_alone(source, (2, 2, 2), desc, cm, lim, thr, 1, a),
                         "R=8 (16 / D)": kernel_alone(source, (2, 2, 2), desc, cm, lim, thr, 8, a)}
    lib = _capi.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    counts, tails = torch.zeros(3, BINS + 3, dtype=torch.int64, device="cuda"), torch.zeros(3, 4, dtype=torch.int64, device="cuda")
    lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
    n, d, c = cm.shape
    ms = event_ms(lambda: _capi.check(lib.glabc_predictive_counts(
        C.byref(bd), cm.data_ptr(), n, d, c, c, SEED, 0, c, BINS, lo.ctypes.data, hi.ctypes.data, thr.ctypes.data, counts.data_ptr(),
        tails.data_ptr(), None, stream), "glabc_predictive_counts"), a.warmup, a.repeats)
    r["kernel_alone"]["built-in glabc_predictive_counts (R = 8)"] = stats(ms, "ms")
    res["mixture_restated"] = r
    del buf, hist, cm
    torch.cuda.empty_cache()

    # ---- Lotka-Volterra: 3000 RK4 steps per draw
    lv = LotkaVolterra_smc.build()
    buf = (torch.tensor([1.0, 1.0]).view(1, 2, 1) + 0.1 * torch.randn(a.lv_rows, 2, a.lv_chains, generator=gen)).abs().cuda()
    hist = buf.permute(0, 2, 1)
    lim = np.array([[0.0, 4.0]] * 8 + [[0.0, 8.0]])
    r, out, (cm, desc, thr) = three_ways(lv, hist, lim, a)
    r["kernel_alone"] = {"R=1 (the rule)": kernel_alone(LotkaVolterra_smc.SOURCE, (2, 8, 8), desc, cm, lim, thr, 1, a),
                         "R=8 (16 / D)": kernel_alone(LotkaVolterra_smc.SOURCE, (2, 8, 8), desc, cm, lim, thr, 8, a)}
    res["lotka_volterra"] = r
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
