"""Rejection ABC on Mixture_set (theta_dim 2): the prior-predictive distances of n draws,
  (a) the fused sweep                 glabc_abc_draws with the distance as its only output, launches of 2^24 draws
  (b) the composed path               glabc_dist_forward -> transpose -> glabc_model_simulate(eps = NULL) -> glabc_model_discrepancy,
                                      the entry points the fused kernel restates, on the same chunks of 2^24 draws: theta and y
                                      go through device memory (one transpose; the log-density glabc_dist_forward also writes
                                      is part of that entry point)
timed on device events, and whole rejection.sample(kernel="model") calls (acceptance sweep, torch.nonzero, regeneration of the
kept draws) timed with a host clock that ends in a device synchronise.  After two warm-up calls of each, (a) and (b) alternate
in one process; the median and the spread (max - min) of the repeats are reported, and (a) beats (b) only if the medians differ
by more than both spreads.  The two paths must give the same distances, bit for bit.  The kernel's unique memory traffic is
the 4 bytes per draw it writes; it is set against the sustained HBM rate to say what the kernel is NOT bound by.

    python tools/rejection_bench.py [--draws 67108864] [--repeats 7] [--warmup 2] [--out profiles/rejection_bench.json]
"""
import argparse
import ctypes as C
import datetime
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-abc-mcmc_amd"))
from glabcmcmc_amd import _capi, rejection  # noqa: E402
from glabcmcmc_amd.examples.Mixture import Mixture_set  # noqa: E402

HBM_SUSTAINED = 6.29e12           # bytes per second the part sustains on a copy
SEED = 20261019


def composed(desc, n, dev, out):
    lib, stream = _capi.lib(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    d, yd = desc.theta_dim, desc.y_dim
    for row0 in range(0, n, rejection.MAX_LAUNCH):
        k = min(rejection.MAX_LAUNCH, n - row0)
        z, log_p = torch.empty(d, k, dtype=torch.float32, device=dev), torch.empty(k, dtype=torch.float32, device=dev)
        _capi.check(lib.glabc_dist_forward(C.byref(desc.prior), k, SEED, row0, z.data_ptr(), log_p.data_ptr(), stream), "glabc_dist_forward")
        theta = z.t().contiguous()
        y = torch.empty(k, yd, dtype=torch.float32, device=dev)
        _capi.check(lib.glabc_model_simulate(C.byref(desc), theta.data_ptr(), None, k, SEED ^ _capi.ABC_NOISE_KEY, row0, y.data_ptr(), stream),
                    "glabc_model_simulate")
        _capi.check(lib.glabc_model_discrepancy(C.byref(desc), y.data_ptr(), k, out.data_ptr() + 4 * row0, stream), "glabc_model_discrepancy")
    return out


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def stats(ts, unit):
    return {unit: ts, "median_" + unit: statistics.median(ts), "spread_" + unit: max(ts) - min(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=1 << 26)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    model = Mixture_set(0.05)
    desc = model.descriptor()
    n = a.draws
    out_b = torch.empty(n, dtype=torch.float32, device=dev)
    fused = lambda: rejection._sweep(rejection._Entry(desc), SEED, n, dev, "distance")          # noqa: E731
    twin = lambda: composed(desc, n, dev, out_b)                               # noqa: E731
    for _ in range(a.warmup):
        fused()
        twin()
    ta, tb = [], []
    for _ in range(a.repeats):
        ms, da = event_ms(fused)
        ta.append(ms)
        ms, db = event_ms(twin)
        tb.append(ms)
    same = bool(torch.equal(da.view(torch.int32), db.view(torch.int32)))
    del da, db, out_b
    res = {"workload": "prior-predictive distances of Mixture_set (theta_dim 2), rejection ABC", "date": datetime.date.today().isoformat(),
           "device": torch.cuda.get_device_name(0), "draws": n, "launch_draws": rejection.MAX_LAUNCH, "repeats": a.repeats, "warmup": a.warmup,
           "fused_distance_sweep": stats(ta, "ms"), "composed_entry_points": stats(tb, "ms"), "distances_equal_bit_for_bit": same}
    fa, fb = res["fused_distance_sweep"], res["composed_entry_points"]
    fa["draws_per_s"] = n / (fa["median_ms"] * 1e-3)
    fb["draws_per_s"] = n / (fb["median_ms"] * 1e-3)
    fa["unique_bytes"] = 4 * n
    fa["unique_bytes_per_s"] = 4 * n / (fa["median_ms"] * 1e-3)
    fa["fraction_of_hbm_sustained"] = fa["unique_bytes_per_s"] / HBM_SUSTAINED
    # what (b) moves at the least: z written, read, theta written, read, y written, read, log_p and the distance written
    fb["least_bytes"] = 4 * n * (6 * desc.theta_dim + 2)
    res["hbm_sustained_bytes_per_s"] = HBM_SUSTAINED
    res["composed_over_fused"] = fb["median_ms"] / fa["median_ms"]
    res["fused_beats_composed_by_more_than_both_spreads"] = bool(fb["median_ms"] - fa["median_ms"] > max(fa["spread_ms"], fb["spread_ms"]))

    whole = lambda: rejection.sample(model, n, kernel="model", seed=SEED)          # noqa: E731
    for _ in range(a.warmup):
        whole()
    ts, kept = [], 0
    for _ in range(a.repeats):
        s, r = clocked(whole)
        ts.append(s)
        kept = int(r.ids.numel())
    res["sample_model_kernel"] = dict(stats(ts, "s"), accepted=kept, draws_per_s=n / statistics.median(ts))
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
