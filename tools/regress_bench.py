"""ABC regression adjustment of kept draws that stay on the GPU: whole calls of
  (a) regression.adjust(GK_set, draws)                glabc_weighted_gram, the host fit of the 154-or-fewer doubles, glabc_regression_apply,
  (b) the composed torch path on the same arrays: Epanechnikov weights, the float64 design matrix X = (1, y - y_obs), X^T (w X) and
      X^T (w theta), torch.linalg.solve on the device, theta - (y - y_obs) B as a float64 matmul, cast to float32,
timed with a host clock that ends in a device synchronise, on what rejection.sample(GK_set, 2^24 draws, kernel="hard",
quantile=0.1) returns (1.7e6 rows, 4 + 8 columns).  After the warm-ups the paths alternate in one process; the median and the spread
(max - min) of the repeats are reported, and one path beats the other only if the medians differ by more than both spreads.  Peak
extra device memory is torch.cuda.max_memory_allocated over a call.  The two kernels are timed alone with device events and set
against one read of their inputs at the sustained HBM rate (the Gram's wavefronts of a segment share the rows through the cache;
the fraction says what the call costs in units of one read).

    python tools/regress_bench.py [--draws 16777216] [--quantile 0.1] [--repeats 7] [--out profiles/regress_bench.json]
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
from glabcmcmc_amd import _capi, regression, rejection  # noqa: E402
from glabcmcmc_amd.examples.GK import GK_set  # noqa: E402

HBM_SUSTAINED = 6.29e12           # bytes per second the part sustains on a copy


def clocked(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def torch_adjust(theta, y, dis, y_obs, delta):
    """-> (adjusted theta float32 (n, D), B float64 (YD, D)) composed from torch operations on the device"""
    d = dis.double()
    u = d / delta
    w = torch.where(d <= delta, 1.0 - u * u, torch.zeros_like(d))
    x = torch.cat([torch.ones(theta.shape[0], 1, dtype=torch.float64, device=theta.device), y.double() - y_obs], dim=1)
    wx = w[:, None] * x
    coef = torch.linalg.solve(x.t() @ wx, wx.t() @ theta.double())
    return (theta.double() - x[:, 1:] @ coef[1:]).float(), coef[1:]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=1 << 24)
    ap.add_argument("--quantile", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    model = GK_set(0.5)
    draws = rejection.sample(model, a.draws, kernel="hard", quantile=a.quantile, seed=20261020)
    n, d, yd = draws.theta.shape[0], draws.theta.shape[1], draws.y.shape[1]
    delta = float(draws.distance.max())
    y_obs_dev = model.y_obs.double().cuda()
    input_bytes = 4 * n * (d + yd + 1)
    res = {"workload": "regression.adjust of rejection.sample(GK_set, %d draws, kernel='hard', quantile=%g)" % (a.draws, a.quantile),
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup,
           "hbm_sustained_bytes_per_s": HBM_SUSTAINED, "rows": n, "theta_dim": d, "y_dim": yd, "delta": delta, "input_bytes": input_bytes,
           "one_read_at_hbm_sustained_ms": input_bytes / HBM_SUSTAINED * 1e3}
    runs = {"adjust": lambda: regression.adjust(model, draws),
            "torch_composed": lambda: torch_adjust(draws.theta, draws.y, draws.distance, y_obs_dev, delta)}
    results, peak = {}, {}
    for name, fn in runs.items():
        for _ in range(a.warmup - 1):
            clocked(fn)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        first_s, results[name] = clocked(fn)
        peak[name] = torch.cuda.max_memory_allocated() - before
        print("# %s: %.4f s" % (name, first_s), file=sys.stderr, flush=True)
    times = {k: [] for k in runs}
    for _ in range(a.repeats):
        for name, fn in runs.items():
            times[name].append(clocked(fn)[0])
    for name, ts in times.items():
        res[name] = dict(stats(ts, "s"), peak_extra_device_bytes=peak[name])
    k, o = res["adjust"], res["torch_composed"]
    res["torch_composed_over_adjust"] = o["median_s"] / k["median_s"]
    res["adjust_beats_torch_by_more_than_the_spread"] = bool(o["median_s"] - k["median_s"] > max(o["spread_s"], k["spread_s"]))
    res["torch_beats_adjust_by_more_than_the_spread"] = bool(k["median_s"] - o["median_s"] > max(o["spread_s"], k["spread_s"]))
    ours, (theirs, their_beta) = results["adjust"], results["torch_composed"]
    res["beta_minus_torch_max_abs"] = float(np.abs(ours.beta - their_beta.cpu().numpy()).max())
    res["beta_max_abs"] = float(np.abs(ours.beta).max())
    res["adjusted_theta_minus_torch_max_abs"] = float((ours.theta - theirs).abs().max())
    res["outside_prior"], res["ess"] = ours.outside_prior, ours.ess
    res["mean"], res["sd"] = ours.mean.tolist(), np.sqrt(np.diag(ours.covariance)).tolist()
    # two whole calls give the same bits; so do two torch calls, or not
    again = regression.adjust(model, draws)
    res["adjust_repeats_bit_for_bit"] = bool(np.array_equal(again.gram, ours.gram) and torch.equal(again.theta, ours.theta))
    res["torch_repeats_bit_for_bit"] = bool(torch.equal(torch_adjust(draws.theta, draws.y, draws.distance, y_obs_dev, delta)[1], their_beta))
    del results, ours, theirs, again

    # each kernel alone, device events around the entry point
    lib = _capi.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    th, stride_t = regression._dimension_major(draws.theta)
    ys, stride_y = regression._dimension_major(draws.y)
    dis = draws.distance.contiguous()
    y_obs = np.ascontiguousarray(model.y_obs.numpy().reshape(-1), np.float64)
    gram = torch.empty(regression.n_stats(d, yd), dtype=torch.float64, device="cuda")
    work = torch.empty(regression.workspace_size(n, d, yd), dtype=torch.float64, device="cuda")
    ms = event_ms(lambda: _capi.check(lib.glabc_weighted_gram(th.data_ptr(), stride_t, d, ys.data_ptr(), stride_y, yd, dis.data_ptr(), None, n,
                                                              y_obs.ctypes.data, delta, 0, gram.data_ptr(), work.data_ptr(), stream),
                                      "glabc_weighted_gram"), a.warmup, a.repeats)
    res["glabc_weighted_gram"] = dict(stats(ms, "ms"), workspace_bytes=work.numel() * 8, segments=(n + 1023) // 1024,
                                      one_read_of_the_inputs_over_kernel_time_as_a_fraction_of_hbm_sustained=input_bytes /
                                      (statistics.median(ms) * 1e-3) / HBM_SUSTAINED)
    beta = np.ascontiguousarray(regression.fit(gram.cpu().numpy(), d, yd).beta)
    out = torch.empty(d, n, dtype=torch.float32, device="cuda")
    ms2 = event_ms(lambda: _capi.check(lib.glabc_regression_apply(th.data_ptr(), stride_t, d, ys.data_ptr(), stride_y, yd, n, y_obs.ctypes.data,
                                                                  beta.ctypes.data, out.data_ptr(), n, stream), "glabc_regression_apply"),
                   a.warmup, a.repeats)
    apply_bytes = 4 * n * (2 * d + yd)
    res["glabc_regression_apply"] = dict(stats(ms2, "ms"), bytes_read_and_written=apply_bytes,
                                         bytes_over_kernel_time_as_a_fraction_of_hbm_sustained=apply_bytes / (statistics.median(ms2) * 1e-3) /
                                         HBM_SUSTAINED)
    print("# kernels: weighted_gram %.3f ms, regression_apply %.3f ms" % (statistics.median(ms), statistics.median(ms2)), file=sys.stderr, flush=True)
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
