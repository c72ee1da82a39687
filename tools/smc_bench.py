"""ABC-SMC on one MI355X.

1. The distance-only sweep of a generation: n proposals of Mixture_set (theta_dim 2) from a population of S particles,
  (a) the fused sweep        glabc_smc_draws with the distance as its only output
  (b) the composed path      glabc_kde_sample -> transpose -> glabc_model_prior_log_prob -> glabc_model_simulate(eps = NULL) ->
                             glabc_model_discrepancy -> where(log_prior == -inf, inf, distance), the entry points the fused kernel
                             restates: theta, y and the log-prior go through device memory
  timed on device events at S = 4096 and S = 65 536.  After two warm-up calls of each, (a) and (b) alternate in one process; the
  median and the spread (max - min) of the repeats are reported, and (a) beats (b) only if the medians differ by more than both
  spreads.  The two paths must give the same distances, bit for bit.

2. Whole calls: smc.sample(kernel="model", N) against a rejection.sample(kernel="model") call sized to accept N draws (its
  acceptance rate comes from a pilot of 2^24 draws; a call of more than --rejection-cap draws is timed at the cap and its time
  scaled), with a host clock that ends in a device synchronise, on Mixture_set with its N(0, I) prior, Mixture_set with a
  Uniform(-10, 10)^2 prior and GK_set.  Simulations and seconds of both are reported.

    python tools/smc_bench.py [--draws 16777216] [--particles 4096] [--repeats 7] [--warmup 2] [--out profiles/smc_bench.json]
"""
import argparse
import ctypes as C
import datetime
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-abc-mcmc_amd"))
from glabcmcmc_amd import _capi, distribution, rejection, smc  # noqa: E402
from glabcmcmc_amd.examples.GK import GK_set  # noqa: E402
from glabcmcmc_amd.examples.Mixture import Mixture_set  # noqa: E402

SEED = 20261020


def composed(desc, kde, n, dev):
    lib, stream = _capi.lib(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    d, yd = desc.theta_dim, desc.y_dim
    z = torch.empty(d, n, dtype=torch.float32, device=dev)
    _capi.check(lib.glabc_kde_sample(C.byref(kde.descriptor()), n, SEED, 0, z.data_ptr(), stream), "glabc_kde_sample")
    theta = z.t().contiguous()
    lp, y, dis = (torch.empty(s, dtype=torch.float32, device=dev) for s in ((n,), (n, yd), (n,)))
    _capi.check(lib.glabc_model_prior_log_prob(C.byref(desc), theta.data_ptr(), n, lp.data_ptr(), stream), "glabc_model_prior_log_prob")
    _capi.check(lib.glabc_model_simulate(C.byref(desc), theta.data_ptr(), None, n, SEED ^ _capi.ABC_NOISE_KEY, 0, y.data_ptr(), stream),
                "glabc_model_simulate")
    _capi.check(lib.glabc_model_discrepancy(C.byref(desc), y.data_ptr(), n, dis.data_ptr(), stream), "glabc_model_discrepancy")
    return torch.where(lp == -math.inf, torch.full_like(dis, math.inf), dis)


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


def sweep(model, S, n, dev, a):
    """the distance-only sweep at a population of S particles: the S nearest of 64 S prior draws under Silverman's rule"""
    desc = model.descriptor()
    r = rejection.sample(model, 64 * S, kernel="hard", n_accept=S, seed=SEED)
    kde = smc.KernelDensity("silverman", device=dev).fit(r.theta)
    fused = lambda: smc._launch(rejection._Entry(desc), kde, SEED, 0, None, n, dev, ("distance",))["distance"]          # noqa: E731
    twin = lambda: composed(desc, kde, n, dev)                                                        # noqa: E731
    for _ in range(a.warmup):
        fused()
        twin()
    ta, tb = [], []
    for _ in range(a.repeats):
        ms, da = event_ms(fused)
        ta.append(ms)
        ms, db = event_ms(twin)
        tb.append(ms)
    fa, fb = stats(ta, "ms"), stats(tb, "ms")
    fa["draws_per_s"], fb["draws_per_s"] = n / (fa["median_ms"] * 1e-3), n / (fb["median_ms"] * 1e-3)
    return {"particles": S, "draws": n, "fused_distance_sweep": fa, "composed_entry_points": fb,
            "distances_equal_bit_for_bit": bool(torch.equal(da.view(torch.int32), db.view(torch.int32))),
            "composed_over_fused": fb["median_ms"] / fa["median_ms"],
            "fused_beats_composed_by_more_than_both_spreads": bool(fb["median_ms"] - fa["median_ms"] > max(fa["spread_ms"], fb["spread_ms"]))}


def whole(name, model, N, a):
    run = lambda: smc.sample(model, N, kernel="model", seed=SEED)          # noqa: E731
    for _ in range(a.warmup):
        run()
    ts = []
    for _ in range(a.repeats):
        s, p = clocked(run)
        ts.append(s)
    out = {"model": name, "particles": N,
           "smc": dict(stats(ts, "s"), simulations=sum(g["n_draws"] for g in p.generations), generations=len(p.generations), ess=p.ess,
                       ladder=[g["epsilon"] for g in p.generations])}
    pilot = rejection.sample(model, 1 << 24, kernel="model", seed=SEED + 1)
    rate = max(int(pilot.ids.numel()), 1) / float(1 << 24)
    needed = int(math.ceil(N / rate))
    n_rej = min(needed, a.rejection_cap)
    rej = lambda: rejection.sample(model, n_rej, kernel="model", seed=SEED + 2)          # noqa: E731
    for _ in range(a.warmup):
        rej()
    ts = []
    for _ in range(a.repeats):
        s, r = clocked(rej)
        ts.append(s)
    st = stats(ts, "s")
    out["rejection"] = dict(st, pilot_accepted=int(pilot.ids.numel()), pilot_draws=1 << 24, simulations_for_N=needed, draws_timed=n_rej,
                            accepted=int(r.ids.numel()), median_s_scaled_to_N=st["median_s"] * needed / n_rej)
    out["simulations_rejection_over_smc"] = needed / out["smc"]["simulations"]
    out["seconds_rejection_over_smc"] = out["rejection"]["median_s_scaled_to_N"] / out["smc"]["median_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=1 << 24)
    ap.add_argument("--particles", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rejection-cap", type=int, default=1 << 30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    res = {"workload": "ABC-SMC proposals of Mixture_set (theta_dim 2) and whole smc.sample calls", "date": datetime.date.today().isoformat(),
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup,
           "sweeps": [sweep(Mixture_set(0.05), S, a.draws, dev, a) for S in (4096, 65536)]}
    wide = distribution.Uniform(2, torch.tensor([-10.0, -10.0]), torch.tensor([10.0, 10.0]))
    res["whole_calls"] = [whole("Mixture_set(0.05), prior N(0, I)", Mixture_set(0.05), a.particles, a),
                          whole("Mixture_set(0.05), prior Uniform(-10, 10)^2", Mixture_set(0.05, prior=wide), a.particles, a),
                          whole("GK_set(1.0), prior Uniform(0, 10)^4", GK_set(1.0), a.particles, a)]
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
