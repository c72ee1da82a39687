"""Coverage checks of an ABC posterior: whole calls of
  (a) coverage.check(Model, R, n, ...)     glabc_coverage_counts sweeps, the table of n prior draws regenerated in registers,
  (b) the composition a user could write before it: rejection.draws materialises the table (theta, y), then per test
      glabc_model_discrepancy of a copy of the Model whose y_obs is y*_r, torch comparisons and sums -- one test at a time, so that
      nothing larger than the table and one vector of n distances exists,
timed with a host clock that ends in a device synchronise.  After the warm-ups the two paths alternate in one process; the median and
the spread (max - min) of the repeats are reported, and one path beats the other only if the medians differ by more than both
spreads.  Under the hard kernel both paths count the very same pairs, so their integers are asserted equal; under the Model's kernel
the composition takes torch.exp where the kernel takes glabc_expf, so it is timed only.  Peak extra device memory is
torch.cuda.max_memory_allocated over a call.

Sizes: Mixture_set, n = 2^20, R = 1024, both kernels, and quantile = 0.01 on it (32 sweeps against torch.kthvalue per test); g-and-k,
n = 2^20, R = 256.  The kernel alone is timed under device events (one full launch, one counting-only launch) and reported as
pair evaluations per second.

    python tools/coverage_bench.py [--repeats 7] [--out profiles/coverage_bench.json]
"""
import argparse
import copy
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
from glabcmcmc_amd import _capi, coverage, engine, rejection  # noqa: E402
from glabcmcmc_amd.examples.GK import GK_set  # noqa: E402
from glabcmcmc_amd.examples.Mixture import Mixture_set  # noqa: E402

SEED = 20261021


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def composed(Model, n, tests, widths, kernel, quantile=None):
    """-> (mass, mass2, below) int64 device tensors through the entry points of the parent commit"""
    lib, desc = _capi.lib(), Model.descriptor()
    table = rejection.draws(Model, n, seed=SEED, want=("theta", "y"))
    theta, y = table.theta, table.y.contiguous()
    ts, ys = tests
    ys_host = ys.cpu().tolist()
    r, d = ts.shape
    dis = torch.empty(n, device=theta.device)
    mass, mass2 = torch.zeros(r, dtype=torch.int64, device=theta.device), torch.zeros(r, dtype=torch.int64, device=theta.device)
    below = torch.zeros(r, d, dtype=torch.int64, device=theta.device)
    rank = None if quantile is None else int(quantile * (n - 1))
    for t in range(r):
        swapped = copy.copy(desc)
        swapped.y_obs = type(desc.y_obs)(*(ys_host[t] + [0.0] * (8 - len(ys_host[t]))))
        _capi.check(lib.glabc_model_discrepancy(C.byref(swapped), y.data_ptr(), n, dis.data_ptr(), None), "glabc_model_discrepancy")
        if kernel == "hard":
            w = torch.kthvalue(dis, rank + 1).values if rank is not None else widths[t]
            m = (dis <= w).to(torch.int64)
        else:
            m = coverage.multiplicity(dis, widths[t], "model")
        mass[t], mass2[t] = m.sum(), (m * m).sum()
        below[t] = (m[:, None] * (theta < ts[t]).to(torch.int64)).sum(dim=0)
    return mass, mass2, below


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


def measure(name, Model, n, r, kernel, eps, a, quantile=None):
    dev = engine.require_device(None)
    t = rejection.draws(Model, r, seed=SEED ^ coverage.COVERAGE_TEST_KEY, want=("theta", "y"))
    tests = (t.theta.contiguous(), t.y.contiguous())
    widths = torch.full((r,), float(eps), device=dev)
    kw = dict(kernel=kernel, tests=tests, seed=SEED)
    kw.update(dict(quantile=quantile) if quantile is not None else dict(epsilon=widths))
    runs = {"check": lambda: coverage.check(Model, r, n, **kw), "composed": lambda: composed(Model, n, tests, widths, kernel, quantile)}
    res = {"draws": n, "tests": r, "pairs": n * r, "kernel": kernel, "theta_dim": int(Model.theta_dim), "y_dim": int(Model.y_dim),
           "epsilon": None if quantile is not None else float(eps), "quantile": quantile}
    results, peak = {}, {}
    for key, fn in runs.items():
        for _ in range(a.warmup - 1):
            clocked(fn)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        _, results[key] = clocked(fn)
        peak[key] = torch.cuda.max_memory_allocated() - before
    c, other = results["check"], results["composed"]
    if kernel == "hard":
        assert torch.equal(c.mass, other[0].cpu()) and torch.equal(c.mass2, other[1].cpu()) and torch.equal(c.below, other[2].cpu()), \
            "the two paths disagree"
        res["equal_integers"] = True
    res["n_empty"], res["chi2"], res["coverage_0.9"] = c.n_empty, c.chi2(10).value, float(c.coverage(0.9).pooled[0])
    times = {key: [] for key in runs}
    for _ in range(a.repeats):
        for key, fn in runs.items():
            times[key].append(clocked(fn)[0])
    for key, ts in times.items():
        res[key] = {"seconds": ts, "median_s": statistics.median(ts), "spread_s": max(ts) - min(ts), "peak_extra_device_bytes": peak[key]}
    ours, theirs = res["check"], res["composed"]
    res["composed_over_check"] = theirs["median_s"] / ours["median_s"]
    gap, spread = theirs["median_s"] - ours["median_s"], max(theirs["spread_s"], ours["spread_s"])
    res["faster_by_more_than_both_spreads"] = "check" if gap > spread else "composed" if -gap > spread else "neither"
    if quantile is None:
        # the kernel alone: one launch over the whole table, the full sums and the counting-only form
        lib, desc = _capi.lib(), Model.descriptor()
        th, ys = tests[0].t().contiguous(), tests[1].t().contiguous()
        mass, mass2 = torch.zeros(r, dtype=torch.int64, device=dev), torch.zeros(r, dtype=torch.int64, device=dev)
        below = torch.zeros(r, th.shape[0], dtype=torch.int64, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def launch(full):
            _capi.check(lib.glabc_coverage_counts(C.byref(desc), SEED, 0, n, th.data_ptr(), ys.data_ptr(), widths.data_ptr(), r, r,
                                                  0 if kernel == "hard" else 1, mass.data_ptr(), mass2.data_ptr() if full else None,
                                                  below.data_ptr() if full else None, stream), "glabc_coverage_counts")
        res["kernels"] = {}
        for label, full in (("full", True), ("counting_only", False)):
            ms = event_ms(lambda: launch(full), a.warmup, a.repeats)
            res["kernels"][label] = {"milliseconds": ms, "median_ms": statistics.median(ms), "spread_ms": max(ms) - min(ms),
                                     "pairs_per_second": n * r / (1e-3 * statistics.median(ms))}
    print("# %s: check %.3f ms against composed %.3f ms%s" % (
        name, 1e3 * ours["median_s"], 1e3 * theirs["median_s"],
        "" if quantile is not None else "; kernel %.4f ms = %.3g pairs/s, counting only %.4f ms" % (
            res["kernels"]["full"]["median_ms"], res["kernels"]["full"]["pairs_per_second"], res["kernels"]["counting_only"]["median_ms"])),
        file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--draws", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    res = {"workload": "coverage.check(Model, R, n) against rejection.draws -> per-test glabc_model_discrepancy + torch sums",
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup}
    mixture, gk = Mixture_set(0.05), GK_set(200.0)
    res["mixture_hard"] = measure("Mixture_set, hard, R = 1024", mixture, a.draws, 1024, "hard", 0.3, a)
    res["mixture_model"] = measure("Mixture_set, model, R = 1024", mixture, a.draws, 1024, "model", 0.3, a)
    res["gk_hard"] = measure("g-and-k, hard, R = 256", gk, a.draws, 256, "hard", 200.0, a)
    res["mixture_quantile"] = measure("Mixture_set, quantile 0.01, R = 1024", mixture, a.draws, 1024, "hard", 0.0, a, quantile=0.01)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
