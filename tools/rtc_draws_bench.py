"""Rejection ABC and ABC-SMC on run-time compiled Models (glabc_rtc_abc_draws / glabc_rtc_smc_draws), on one MI355X.

1. The distance-only sweep of n draws through the draws program, against the composed entry points that specify a draw
   (CompiledModel.composed_draws: glabc_dist_forward twice -> glabc_rtc_simulate -> glabc_model_discrepancy; theta, eps and y go
   through device memory), timed on device events, for the Mixture simulator restated as a CompiledModel -- with the built-in
   glabc_abc_draws on Mixture_set beside it -- and for the Lotka-Volterra Model of examples/LotkaVolterra_smc.py.  After two warm-up
   calls of each the paths alternate in one process; medians and spreads (max - min) of the repeats are reported.  The distances
   must be equal bit for bit.

2. Whole calls on Lotka-Volterra, host clock ending in a device synchronise: smc.sample(kernel="model") and
   rejection.sample(kernel="model"), fused against path="generic" (what path="auto" ran before the draws program existed).  The
   generic path needs calculate_log_kernel_dis, which CompiledModel does not have: the tool adds the Gaussian kernel of the
   descriptor to a subclass, for the generic side only.

3. ABC-SMC against a rejection call sized to accept as many draws (its rate from a pilot), both fused, as in tools/smc_bench.py.

    python tools/rtc_draws_bench.py [--draws 16777216] [--particles 4096] [--repeats 7] [--warmup 2] [--out profiles/rtc_draws_bench.json]
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
from glabcmcmc_amd import distribution, engine, rejection, smc  # noqa: E402
from glabcmcmc_amd.compiled import CompiledModel  # noqa: E402
from glabcmcmc_amd.examples import LotkaVolterra_smc  # noqa: E402
from glabcmcmc_amd.examples.Mixture import Mixture_set  # noqa: E402

SEED = 20261020
MIXTURE_SOURCE = """
GLABC_SIMULATOR void glabc_user_simulate(const float* theta, const float* eps, float* y)
{
    const float s[2] = {%sf, %sf};
    for (int j = 0; j < 2; ++j) {
        const float noise = 0.0f + s[j] * eps[j];
        y[j] = fabsf(theta[j]) + noise;
    }
}
"""


class WithKernelOfDistance(CompiledModel):
    """the generic path's kernel="model" needs the kernel as a function of the distance: the descriptor's Gaussian, in torch"""

    def calculate_log_kernel_dis(self, dis, epsilon=None):
        eps = self.epsilon if epsilon is None else epsilon
        kern = distribution.DiagGaussian(1, loc=torch.tensor([0.0]), log_scale=torch.log(torch.tensor([eps])))
        return kern.log_prob(dis.cpu().view(-1, 1)).to(dis.device)


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


def alternate(fns, a, timer):
    """warm-ups of each, then the repeats alternating -> ([times] per function, last outputs)"""
    for _ in range(a.warmup):
        for fn in fns:
            fn()
    ts, outs = [[] for _ in fns], [None] * len(fns)
    for _ in range(a.repeats):
        for i, fn in enumerate(fns):
            t, outs[i] = timer(fn)
            ts[i].append(t)
    return ts, outs


def sweep(name, model, n, dev, a, builtin=None):
    seed = engine.draw_seed(SEED)
    entry = rejection._path(model, "fused", model.epsilon)
    desc, handle = entry.desc, entry.program
    fns = [lambda: rejection._launch(entry, seed, 0, None, n, dev, ("distance",))["distance"],
           lambda: model.composed_draws(handle, desc, seed, 0, n)["distance"]]
    names = ["program_distance_sweep", "composed_entry_points"]
    if builtin is not None:
        b = rejection._path(builtin, "fused", builtin.epsilon)
        fns.append(lambda: rejection._launch(b, seed, 0, None, n, dev, ("distance",))["distance"])
        names.append("builtin_glabc_abc_draws")
    ts, outs = alternate(fns, a, event_ms)
    out = {"model": name, "draws": n}
    for k, t in zip(names, ts):
        out[k] = dict(stats(t, "ms"), draws_per_s=n / (statistics.median(t) * 1e-3))
    out["distances_equal_bit_for_bit"] = all(bool(torch.equal(outs[0].view(torch.int32), o.view(torch.int32))) for o in outs[1:])
    out["composed_over_program"] = out[names[1]]["median_ms"] / out[names[0]]["median_ms"]
    if builtin is not None:
        out["program_over_builtin"] = out[names[0]]["median_ms"] / out[names[2]]["median_ms"]
    return out


def whole(fused_model, generic_model, N, n_rej, a):
    prior = generic_model.prior
    calls = {"smc.sample": [lambda: smc.sample(fused_model, N, kernel="model", seed=SEED, path="fused"),
                            lambda: smc.sample(generic_model, N, kernel="model", path="generic", prior=prior)],
             "rejection.sample": [lambda: rejection.sample(fused_model, n_rej, kernel="model", seed=SEED, path="fused"),
                                  lambda: rejection.sample(generic_model, n_rej, kernel="model", path="generic", prior=prior)]}
    out = {}
    for name, fns in calls.items():
        torch.manual_seed(SEED)
        ts, outs = alternate(fns, a, clocked)
        rec = {"fused": stats(ts[0], "s"), "generic": stats(ts[1], "s"), "generic_over_fused": statistics.median(ts[1]) / statistics.median(ts[0])}
        if name == "smc.sample":
            rec["particles"] = N
            for side, p in zip(("fused", "generic"), outs):
                rec[side].update(simulations=sum(g["n_draws"] for g in p.generations), generations=len(p.generations), ess=p.ess,
                                 ladder=[g["epsilon"] for g in p.generations])
        else:
            rec["draws"] = n_rej
            for side, r in zip(("fused", "generic"), outs):
                rec[side]["accepted"] = int(r.ids.numel())
        out[name] = rec
    return out


def smc_against_rejection(model, N, pilot_draws, a):
    ts, outs = alternate([lambda: smc.sample(model, N, kernel="model", seed=SEED, path="fused")], a, clocked)
    p = outs[0]
    out = {"particles": N, "smc": dict(stats(ts[0], "s"), simulations=sum(g["n_draws"] for g in p.generations), generations=len(p.generations),
                                       ess=p.ess, ladder=[g["epsilon"] for g in p.generations])}
    pilot = rejection.sample(model, pilot_draws, kernel="model", seed=SEED + 1, path="fused")
    rate = max(int(pilot.ids.numel()), 1) / float(pilot_draws)
    needed = int(math.ceil(N / rate))
    n_rej = min(needed, a.rejection_cap)
    ts, outs = alternate([lambda: rejection.sample(model, n_rej, kernel="model", seed=SEED + 2, path="fused")], a, clocked)
    st = stats(ts[0], "s")
    out["rejection"] = dict(st, pilot_accepted=int(pilot.ids.numel()), pilot_draws=pilot_draws, simulations_for_N=needed, draws_timed=n_rej,
                            accepted=int(outs[0].ids.numel()), median_s_scaled_to_N=st["median_s"] * needed / n_rej)
    out["simulations_rejection_over_smc"] = needed / out["smc"]["simulations"]
    out["seconds_rejection_over_smc"] = out["rejection"]["median_s_scaled_to_N"] / out["smc"]["median_s"]
    out["smc_wins_on_wall_time"] = bool(out["seconds_rejection_over_smc"] > 1.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=1 << 24)
    ap.add_argument("--particles", type=int, default=4096)
    ap.add_argument("--whole-rejection-draws", type=int, default=1 << 22)
    ap.add_argument("--pilot-draws", type=int, default=1 << 22)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rejection-cap", type=int, default=1 << 28)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    builtin = Mixture_set(0.05)
    d = builtin.descriptor()
    mixture = CompiledModel(2, 2, MIXTURE_SOURCE % (float(d.noise.p2[0]).hex(), float(d.noise.p2[1]).hex()), builtin._prior(),
                            [d.y_obs[0], d.y_obs[1]], 0.05)
    lv = LotkaVolterra_smc.build()
    lv_generic = WithKernelOfDistance(lv.theta_dim, lv.y_dim, lv.simulator_source, lv.prior, lv.y_obs, lv.epsilon, noise_dim=lv.noise_dim)
    res = {"workload": "rejection ABC and ABC-SMC on run-time compiled Models (glabc_rtc_abc_draws / glabc_rtc_smc_draws)",
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup,
           "lotka_volterra_rk4_steps": LotkaVolterra_smc.N_STEPS}

    def save():
        print(json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")

    res["sweeps"] = [sweep("Mixture_set(0.05) restated as a CompiledModel", mixture, a.draws, dev, a, builtin=builtin),
                     sweep("examples/LotkaVolterra_smc.py", lv, a.draws, dev, a)]
    save()
    res["smc_against_rejection_lotka_volterra"] = smc_against_rejection(lv, a.particles, a.pilot_draws, a)
    save()
    res["whole_calls_lotka_volterra"] = whole(lv, lv_generic, a.particles, a.whole_rejection_draws, a)
    save()


if __name__ == "__main__":
    main()
