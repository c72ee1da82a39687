"""The full-covariance perturbation kernel of ABC-SMC against the diagonal one, on one MI355X.

1. The distance-only sweep of a generation: n proposals from a population of S particles -- the S nearest of 64 S prior draws --
  (a) the diagonal kernel    glabc_smc_draws, Silverman's bandwidth
  (b) the full kernel        glabc_smc_draws_full, Silverman's factor times the Cholesky factor of the population covariance
  on the SAME population, the distance as the only output, timed on device events at S = 4096 and S = 65 536 for theta_dim 2
  (Mixture_set), 4 (g-and-k) and 8 (|theta| + noise).  After two warm-up calls of each, (a) and (b) alternate in one process; the
  median and the spread (max - min) of the repeats are reported, and one beats the other only if the medians differ by more than
  both spreads.

2. Whole calls: smc.sample(kernel="model", N, bandwidth=...) with perturbation="diagonal" against perturbation="full", alternating,
  with a host clock that ends in a device synchronise, on the correlated linear Model (examples/Correlated_smc.py, a CompiledModel),
  g-and-k and Lotka-Volterra (examples/LotkaVolterra_smc.py), under "beaumont" and under "silverman": simulations, generations, ESS
  and seconds of both.  Where the full kernel loses -- more simulations, a smaller ESS or more seconds -- the entry says so.

    python tools/smc_full_bench.py [--draws 16777216] [--particles 2000] [--repeats 7] [--warmup 2] [--out profiles/smc_full_bench.json]
"""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gl-abc-mcmc_amd"))
from glabcmcmc_amd import distribution, rejection, smc  # noqa: E402
from glabcmcmc_amd.examples import Correlated_smc, LotkaVolterra_smc  # noqa: E402
from glabcmcmc_amd.examples.GK import GK_set  # noqa: E402
from glabcmcmc_amd.examples.Mixture import Mixture_set  # noqa: E402

SEED = 20261021


class AbsGauss(Mixture_set):
    """Mixture_set at d parameters: y = |theta| + N(0, 0.05 I), prior N(0, I), y_obs = 1.5 everywhere"""

    def __init__(self, epsilon, d):
        super().__init__(epsilon)
        self.theta_dim = self.y_dim = d
        self.y_obs = torch.full((1, d), 1.5)

    def _likelihood(self):
        d = self.theta_dim
        return distribution.DiagGaussian(d, torch.zeros(d), torch.log(torch.full((d,), 0.05).sqrt()))

    def _prior(self):
        d = self.theta_dim
        return distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d))


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


def sweep(name, model, S, n, dev, a):
    entry = rejection._Entry(model.descriptor())
    r = rejection.sample(model, 64 * S, kernel="hard", n_accept=S, seed=SEED)
    kde = smc.KernelDensity("silverman", device=dev).fit(r.theta)
    weights = torch.full((S,), 1.0 / S, dtype=torch.float64, device=dev)
    chol = smc.pack_cholesky(smc.full_factor(r.theta, weights, "silverman"), entry.theta_dim)
    diagonal = lambda: smc._launch(entry, kde, SEED, 0, None, n, dev, ("distance",))["distance"]          # noqa: E731
    full = lambda: smc._launch(entry, kde, SEED, 0, None, n, dev, ("distance",), chol)["distance"]        # noqa: E731
    for _ in range(a.warmup):
        diagonal()
        full()
    ta, tb = [], []
    for _ in range(a.repeats):
        ta.append(event_ms(diagonal)[0])
        tb.append(event_ms(full)[0])
    fa, fb = stats(ta, "ms"), stats(tb, "ms")
    fa["draws_per_s"], fb["draws_per_s"] = n / (fa["median_ms"] * 1e-3), n / (fb["median_ms"] * 1e-3)
    apart = abs(fb["median_ms"] - fa["median_ms"]) > max(fa["spread_ms"], fb["spread_ms"])
    return {"model": name, "theta_dim": entry.theta_dim, "particles": S, "draws": n, "diagonal": fa, "full": fb,
            "full_over_diagonal": fb["median_ms"] / fa["median_ms"], "medians_apart_by_more_than_both_spreads": bool(apart)}


def whole(name, model, N, bandwidth, a):
    run = lambda p: smc.sample(model, N, kernel="model", bandwidth=bandwidth, seed=SEED, perturbation=p)          # noqa: E731
    for _ in range(a.warmup):
        run("diagonal")
        run("full")
    ts, last = {"diagonal": [], "full": []}, {}
    for _ in range(a.repeats):
        for p in ("diagonal", "full"):
            s, last[p] = clocked(lambda: run(p))
            ts[p].append(s)
    out = {"model": name, "particles": N, "bandwidth": bandwidth}
    for p in ("diagonal", "full"):
        pop = last[p]
        out[p] = dict(stats(ts[p], "s"), simulations=sum(g["n_draws"] for g in pop.generations), generations=len(pop.generations), ess=pop.ess)
    out["simulations_diagonal_over_full"] = out["diagonal"]["simulations"] / out["full"]["simulations"]
    out["seconds_diagonal_over_full"] = out["diagonal"]["median_s"] / out["full"]["median_s"]
    loses = [what for what, lost in (("more simulations", out["full"]["simulations"] > out["diagonal"]["simulations"]),
                                     ("a smaller ESS", out["full"]["ess"] < out["diagonal"]["ess"]),
                                     ("more seconds", out["full"]["median_s"] > out["diagonal"]["median_s"])) if lost]
    out["full_loses_in"] = loses
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=1 << 24)
    ap.add_argument("--particles", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    models = [("Mixture_set(0.05)", Mixture_set(0.05)), ("GK_set(1.0)", GK_set(1.0)), ("|theta| + noise, theta_dim 8, epsilon 0.5", AbsGauss(0.5, 8))]
    res = {"workload": "ABC-SMC: full-covariance against diagonal perturbation kernel, distance-only sweeps and whole smc.sample calls",
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup,
           "note": "one process, one session; nothing else was measured",
           "sweeps": [sweep(name, m, S, a.draws, dev, a) for name, m in models for S in (4096, 65536)]}
    calls = [("examples/Correlated_smc.py (CompiledModel)", Correlated_smc.build()), ("GK_set(1.0), prior Uniform(0, 10)^4", GK_set(1.0)),
             ("examples/LotkaVolterra_smc.py (CompiledModel)", LotkaVolterra_smc.build())]
    res["whole_calls"] = []
    for name, m in calls:
        for bw in ("beaumont", "silverman"):
            try:
                res["whole_calls"].append(whole(name, m, a.particles, bw, a))
            except RuntimeError as exc:                                    # a run that does not finish is a result too
                res["whole_calls"].append({"model": name, "particles": a.particles, "bandwidth": bw, "error": str(exc)})
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
