"""Randomised differential test of the run-time compiled lane-group kernel (glabc_rtc_compile_wide) against the CPU checker
(not collected by pytest; run on the GPU box):

    python tests/fuzz_rtc_wide.py [seconds] [seed]

Each case: a random user simulator (theta / y / noise dimensions 1..8) with a random subset of the Model's prior / discrepancy /
kernel as user source too, a batch size 17..4096 (log-uniform), a random lanes per chain (the library's choice, or forced 8 / 16 /
32 / 64), random proposals, epsilon, global_frequency, chain id offset and iterations per launch.  Histories, final states,
log-weights, flags, move counts and streamed sums must equal the checker's bit for bit.  A forced lane count whose LDS the device
cannot give a workgroup must be refused (GLABC_ERR_ARG) with the chains left untouched.
"""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "gl-abc-mcmc_amd")]
import oracle_lib                                                   # noqa: E402
from glabcmcmc_amd import _capi, engine                             # noqa: E402
from helpers import bits, make_dist                                 # noqa: E402
from fuzz_parity import random_dist, random_hooks, random_simulator   # noqa: E402
from test_rtc import host_hooks, host_simulator                     # noqa: E402

MAX_LDS = None


def max_lds():
    global MAX_LDS
    if MAX_LDS is None:
        MAX_LDS = torch.cuda.get_device_properties(0).shared_memory_per_block
    return MAX_LDS


def one_case(rng, oracle, k):
    import glabcmcmc_amd as g_
    d, yd, nd = (int(rng.integers(1, 9)) for _ in range(3))
    N = int(np.exp(rng.uniform(np.log(17), np.log(4096.5))))
    lanes = int(rng.choice([0, 0, 8, 16, 32, 64]))
    src = random_simulator(rng, d, yd, nd)
    if rng.random() < 0.5:
        src += random_hooks(rng, d, yd)
    keep_lib, fn = host_simulator(src, d, yd, nd)
    oracle.oracle_set_user_simulator(fn)
    oracle.oracle_set_user_model(*host_hooks(keep_lib))
    eps = float(np.exp(rng.uniform(np.log(0.05), np.log(5))))
    gf = float(rng.choice([0.0, 1.0, rng.random()]))
    lspec, gspec = random_dist(rng, d, True), random_dist(rng, d, False)
    prior = make_dist(("gauss", [0.0] * d, [float(v) for v in np.exp(rng.normal(0.2, 0.3, d))]))
    cm = g_.CompiledModel(d, yd, src, prior, [float(v) for v in rng.normal(0.8, 0.3, yd)], eps, noise_dim=nd)
    model = cm.descriptor()
    local, glob = make_dist(lspec).descriptor(), make_dist(gspec).descriptor()
    n = int(rng.integers(1, 700))
    T = max(1, min(int(rng.integers(1, 25)), 3_000_000 // (n * N) + 1))
    kpl = int(rng.integers(1, T + 1))
    seed, chain0 = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40))
    theta0 = rng.normal(0, 1, (n, d)).astype(np.float32)
    y0 = rng.normal(0.8, 0.5, (n, yd)).astype(np.float32)
    dev = torch.device("cuda", 0)
    chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev, chain0=chain0)
    hist = torch.full((T, d, n), float("nan"), device=dev)
    mom = engine.Moments(n, d, dev)
    L = lanes or (8 if N <= 64 else 16 if N <= 128 else 32 if N <= 256 else 64)
    fits = 4 * (256 // L) * (N + 33) <= max_lds()
    desc = dict(case=k, d=d, yd=yd, nd=nd, N=N, lanes=lanes, eps=eps, gf=gf, local=lspec, glob=gspec, n=n, T=T, kpl=kpl, source=src)
    prog = cm.program(_capi.ALGO_GLMCMC, N)
    try:
        engine.run_steps(None, model, local, glob, chains, T, 1, seed, gf, N, history=hist, moments=mom, lanes_per_chain=lanes,
                         steps_per_launch=kpl, rtc_program=prog)
        refused = False
    except RuntimeError as e:
        refused = "status -4" in str(e)
        if not refused:
            raise
    torch.cuda.synchronize()
    if not fits:
        ok = refused and bool(torch.isnan(hist).all()) and int(chains.n_moves.sum()) == 0
        del cm
        oracle.oracle_set_user_model(None, None, None)
        return ok, dict(desc, refused=True), 0
    hc = oracle_lib.HostChains(theta0, y0, chain0=chain0)
    hh = np.zeros((T, d, n), np.float32)
    hm = oracle_lib.HostMoments(n, d)
    run, keep = oracle_lib.make_run(seed=seed, step0=1, n_steps=T, gf=gf, batch=N, history=hh, moments=hm)
    cs = hc.struct()
    assert oracle.oracle_glmcmc_steps(C.byref(model), C.byref(local), C.byref(glob), C.byref(cs), C.byref(run)) == 0
    ok = not refused and np.array_equal(bits(hist.cpu().numpy()), bits(hh)) \
        and np.array_equal(bits(chains.theta.cpu().numpy()), bits(hc.theta)) and np.array_equal(bits(chains.y.cpu().numpy()), bits(hc.y)) \
        and np.array_equal(bits(chains.log_w.cpu().numpy()), bits(hc.log_w)) \
        and np.array_equal(chains.flags.cpu().numpy().astype(np.uint32), hc.flags) \
        and np.array_equal(chains.n_moves.cpu().numpy().astype(np.uint32), hc.n_moves) \
        and np.array_equal(mom.sum_theta.cpu().numpy(), hm.sum_theta) and np.array_equal(mom.sum_outer.cpu().numpy(), hm.sum_outer) \
        and np.array_equal(mom.sum_jump.cpu().numpy(), hm.sum_jump)
    del cm
    oracle.oracle_set_user_model(None, None, None)
    return ok, desc, int(hc.n_moves.sum())


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
    oracle = oracle_lib.load()
    _capi.lib()
    t0, k, moves, refused, bad = time.time(), 0, 0, 0, []
    while time.time() - t0 < budget:
        ok, desc, mv = one_case(rng, oracle, k)
        moves += mv
        refused += bool(desc.get("refused"))
        if not ok:
            bad.append(desc)
            print("MISMATCH", desc, flush=True)
        k += 1
        if k % 10 == 0:
            print("%d cases (%d refused as too large for LDS), %d moves, %d mismatches, %.0fs" % (k, refused, moves, len(bad), time.time() - t0),
                  flush=True)
    print("done: %d cases (%d forced lane counts refused as too large for LDS, as required), %d accepted moves, %d mismatches"
          % (k, refused, moves, len(bad)))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
