"""Parity of the gfx950 kernels (through the C ABI) with
  (1) the reference itself -- the golden chains produced by the unmodified reference loops
      on the specified Philox stream (tests/golden/*_philox_*.npz), bit for bit;
  (2) the CPU oracle on fresh seeded inputs -- histories, final states, counters, bit for bit;
  (3) size-independent properties at BASELINE.json's full size (65 536 chains).
GPU only:  python -m pytest tests -m gpu
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle_lib
from helpers import GLMALA_GOLDENS_EXACT, GLMALA_GOLDENS_MKL, SAMPLER_GOLDENS, bits, descriptors, load_golden, make_dist, mala_params

pytestmark = pytest.mark.gpu

ENTRY = {"glmcmc": "glabc_glmcmc_steps", "globalmcmc": "glabc_globalmcmc_steps"}


def hip_run(algo, model, local, glob, theta0, y0, T, seed, gf, N, chain0=0, steps_per_launch=None, moments=False,
            step0=1, chains=None, history=True, lanes=0, debug_flags=0):
    from glabcmcmc_amd import engine
    dev = torch.device("cuda", 0)
    if chains is None:
        chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev, chain0=chain0)
        if algo == "glmcmc":
            engine.init_weights(model, glob, chains)
    hist = torch.empty(T, chains.d, chains.n, dtype=torch.float32, device=dev) if history else None
    mom = engine.Moments(chains.n, chains.d, dev) if moments else None
    engine.run_steps(ENTRY[algo], model, local, glob, chains, T, step0, seed, gf, N, history=hist, moments=mom,
                     steps_per_launch=steps_per_launch, lanes_per_chain=lanes, debug_flags=debug_flags)
    torch.cuda.synchronize()
    return (hist.cpu().numpy() if history else None), chains, mom


def oracle_run(oracle, algo, model, local, glob, theta0, y0, T, seed, gf, N, chain0=0, moments=False):
    hc = oracle_lib.HostChains(theta0, y0, chain0=chain0)
    hh = np.zeros((T, theta0.shape[1], theta0.shape[0]), np.float32)
    mom = oracle_lib.HostMoments(theta0.shape[0], theta0.shape[1]) if moments else None
    run, keep = oracle_lib.make_run(seed=seed, step0=1, n_steps=T, gf=gf, batch=N, history=hh, moments=mom)
    cs = hc.struct()
    if algo == "glmcmc":
        assert oracle.oracle_init_weights(C.byref(model), C.byref(glob), C.byref(cs)) == 0
        rc = oracle.oracle_glmcmc_steps(C.byref(model), C.byref(local), C.byref(glob), C.byref(cs), C.byref(run))
    else:
        rc = oracle.oracle_globalmcmc_steps(C.byref(model), C.byref(local), C.byref(glob), C.byref(cs), C.byref(run))
    assert rc == 0
    return hh, hc, mom


def assert_same_state(chains, hc, isir):
    assert np.array_equal(bits(chains.theta.cpu().numpy()), bits(hc.theta))
    assert np.array_equal(bits(chains.y.cpu().numpy()), bits(hc.y))
    assert np.array_equal(chains.n_moves.cpu().numpy().astype(np.uint32), hc.n_moves)
    if isir:
        assert np.array_equal(bits(chains.log_w.cpu().numpy()), bits(hc.log_w))
        assert np.array_equal(chains.flags.cpu().numpy().astype(np.uint32), hc.flags)


# ---------------------------------------------------------------------------------- (1)
@pytest.mark.parametrize("name", [n for n in SAMPLER_GOLDENS if "philox" in n])
def test_hip_reproduces_reference_chains(hip, name):
    """The kernel, on the Philox stream, visits exactly the float32 states the unmodified
    reference loop visited when it was fed the same stream."""
    g = load_golden(name)
    cfg = g["cfg"]
    model, local, glob = descriptors(cfg, g)
    hist, chains, _ = hip_run(str(g["algo"]), model, local, glob, g["theta0"], g["y0"], cfg["T"], cfg["seed"],
                              cfg["gf"], cfg["N"], chain0=cfg.get("chain0", 0))
    got = np.concatenate([g["theta0"][None], hist.transpose(0, 2, 1)], axis=0)
    same = bits(got) == bits(g["chains"])
    assert same.all(), "first mismatch at (t, chain, dim) = %s" % (np.argwhere(~same)[0],)


@pytest.mark.parametrize("name", [n for n in SAMPLER_GOLDENS if "tape" in n])
def test_hip_replays_stored_tapes(hip, name):
    """glabc_run.tape on the GPU: the stored-tape goldens (NumPy-generated numbers, independent of the Philox
    specification) replayed through the kernels give the reference's chains bit for bit."""
    from glabcmcmc_amd import _capi as A
    from glabcmcmc_amd import engine
    g = load_golden(name)
    cfg = g["cfg"]
    model, local, glob = descriptors(cfg, g)
    algo = str(g["algo"])
    dev = torch.device("cuda", 0)
    chains = engine.ChainBatch(torch.from_numpy(g["theta0"]), torch.from_numpy(g["y0"]), dev)
    if algo == "glmcmc":
        engine.init_weights(model, glob, chains)
    T = cfg["T"]
    u = torch.from_numpy(np.ascontiguousarray(g["tape_u"])).to(dev)
    r = torch.from_numpy(np.ascontiguousarray(g["tape_r"])).to(dev)
    z = torch.from_numpy(np.ascontiguousarray(g["tape_z"])).to(dev)
    tape = A.Tape(u.data_ptr(), r.data_ptr(), z.data_ptr(), g["tape_z"].shape[2], 0)
    hist = torch.empty(T, 2, chains.n, dtype=torch.float32, device=dev)
    run = A.Run()
    run.seed, run.step0, run.n_steps, run.global_frequency, run.batch_size = 0, 1, T, cfg["gf"], cfg["N"]
    run.history, run.hist_stride, run.tape = hist.data_ptr(), chains.n, C.pointer(tape)
    cs = chains.struct()
    fn = hip.glabc_glmcmc_steps if algo == "glmcmc" else hip.glabc_globalmcmc_steps
    assert fn(C.byref(model), C.byref(local), C.byref(glob), C.byref(cs), C.byref(run), None) == 0
    torch.cuda.synchronize()
    got = np.concatenate([g["theta0"][None], hist.cpu().numpy().transpose(0, 2, 1)], axis=0)
    same = bits(got) == bits(g["chains"])
    assert same.all(), "first mismatch at (t, chain, dim) = %s" % (np.argwhere(~same)[0],)


# ---------------------------------------------------------------------------------- (2)
CASES = [
    # algo, d, N, gf, eps, local, global, chains, T
    ("glmcmc", 2, 5, 0.9, 0.05, ("gauss", [0, 0], [0.35, 0.35]), ("gauss", [0, 0], [1, 1]), 4096, 300),
    ("glmcmc", 2, 5, 0.5, 0.3, ("gauss", [0, 0], [0.35, 0.35]), ("gauss", [0, 0], [1, 1]), 1000, 257),
    ("glmcmc", 2, 1, 0.3, 0.3, ("gauss", [0, 0], [0.5, 0.5]), ("gauss", [0.2, -0.1], [1.5, 0.7]), 777, 200),
    ("glmcmc", 2, 2, 1.0, 0.3, ("gauss", [0, 0], [0.5, 0.5]), ("gauss", [0, 0], [1, 1]), 640, 100),
    ("glmcmc", 2, 7, 0.0, 0.3, ("gauss", [0, 0], [0.5, 0.5]), ("gauss", [0, 0], [1, 1]), 640, 100),
    ("glmcmc", 2, 8, 0.8, 0.2, ("gauss", [0, 0], [0.35, 0.35]), ("gauss", [0, 0], [1, 1]), 512, 150),
    ("glmcmc", 2, 16, 0.8, 0.2, ("gauss", [0, 0], [0.35, 0.35]), ("gauss", [0, 0], [1, 1]), 512, 100),
    ("glmcmc", 2, 4, 0.7, 0.3, ("uniform", [-0.5, -0.5], [0.5, 0.5]), ("uniform", [-3, -3], [3, 3]), 1024, 200),
    ("glmcmc", 2, 3, 0.6, 0.3, ("gauss", [0, 0], [0.35, 0.35]), ("uniform", [-3, -3], [3, 3]), 1024, 200),
    ("globalmcmc", 2, 1, 0.5, 0.05, ("gauss", [0, 0], [0.35, 0.35]), ("gauss", [0, 0], [1, 1]), 4096, 300),
    ("globalmcmc", 2, 1, 0.5, 0.3, ("uniform", [-0.5, -0.5], [0.5, 0.5]), ("gauss", [0, 0], [1, 1]), 1000, 200),
    ("globalmcmc", 2, 1, 1.0, 0.3, ("gauss", [0, 0], [0.35, 0.35]), ("uniform", [-3, -3], [3, 3]), 640, 100),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-N%d-gf%g-%s-%s" % (c[0], c[2], c[3], c[5][0], c[6][0]))
def test_hip_equals_oracle(hip, oracle, case):
    algo, d, N, gf, eps, lspec, gspec, n, T = case
    cfg = dict(epsilon=eps, local=lspec, **{"global": gspec})
    model, local, glob = descriptors(cfg)
    rng = np.random.default_rng(n * 31 + T)
    theta0 = rng.standard_normal((n, d)).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((n, d))).astype(np.float32)
    seed, chain0 = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40))
    hist, chains, mom = hip_run(algo, model, local, glob, theta0, y0, T, seed, gf, N, chain0=chain0, moments=True)
    hh, hc, hm = oracle_run(oracle, algo, model, local, glob, theta0, y0, T, seed, gf, N, chain0=chain0, moments=True)
    same = bits(hist) == bits(hh)
    assert same.all(), "first mismatch at (t, dim, chain) = %s" % (np.argwhere(~same)[0],)
    assert_same_state(chains, hc, algo == "glmcmc")
    assert hc.n_moves.sum() > 0
    # streamed moments: same float64 operations in the same order on both sides
    assert np.array_equal(mom.sum_theta.cpu().numpy(), hm.sum_theta)
    assert np.array_equal(mom.sum_outer.cpu().numpy(), hm.sum_outer)
    assert np.array_equal(mom.sum_jump.cpu().numpy(), hm.sum_jump)


GK_CASES = [
    ("glmcmc", 5, 0.8, 1.0, ("gauss", [0.0] * 4, [0.15] * 4), ("uniform", [0.0] * 4, [10.0] * 4), 1500, 200, 1),
    ("glmcmc", 5, 0.8, 1.0, ("gauss", [0.0] * 4, [0.15] * 4), ("uniform", [0.0] * 4, [10.0] * 4), 700, 150, 2),
    ("glmcmc", 3, 0.5, 0.7, ("gauss", [0.0] * 4, [0.2, 0.1, 0.2, 0.1]), ("gauss", [3.0, 1.5, 2.0, 1.0], [2.0, 1.0, 1.5, 0.7]), 700, 150, 4),
    ("glmcmc", 8, 0.9, 0.5, ("uniform", [-0.3] * 4, [0.3] * 4), ("uniform", [0.0] * 4, [10.0] * 4), 300, 100, 1),
    ("globalmcmc", 1, 0.5, 1.0, ("gauss", [0.0] * 4, [0.15] * 4), ("uniform", [0.0] * 4, [10.0] * 4), 1500, 300, 0),
]


@pytest.mark.parametrize("case", GK_CASES, ids=lambda c: "%s-N%d-%s-%s-L%d" % (c[0], c[1], c[4][0], c[5][0], c[8]))
def test_gk_model_equals_oracle(hip, oracle, case):
    """BASELINE config 4's model (g-and-k order statistics, theta_dim 4, y_dim 8): kernel == oracle, bit for bit."""
    algo, N, gf, eps, lspec, gspec, n, T, lanes = case
    cfg = dict(model="gk", epsilon=eps, local=lspec, **{"global": gspec})
    model, local, glob = descriptors(cfg)
    rng = np.random.default_rng(n + T + N)
    theta0 = rng.uniform(0.5, 5.0, (n, 4)).astype(np.float32)
    y0 = np.sort(rng.uniform(1.0, 8.0, (n, 8)).astype(np.float32), axis=1)
    seed, chain0 = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40))
    hist, chains, mom = hip_run(algo, model, local, glob, theta0, y0, T, seed, gf, N, chain0=chain0, moments=True, lanes=lanes)
    hh, hc, hm = oracle_run(oracle, algo, model, local, glob, theta0, y0, T, seed, gf, N, chain0=chain0, moments=True)
    same = bits(hist) == bits(hh)
    assert same.all(), "first mismatch at (t, dim, chain) = %s" % (np.argwhere(~same)[0],)
    assert_same_state(chains, hc, algo == "glmcmc")
    assert np.array_equal(mom.sum_jump.cpu().numpy(), hm.sum_jump)
    assert hc.n_moves.sum() > 0


def test_gk_model_callbacks_on_gpu(hip, oracle):
    from glabcmcmc_amd.examples.GK import GK_set
    m = GK_set(0.8)
    desc = m.descriptor()
    rng = np.random.default_rng(3)
    theta = rng.uniform(-1, 11, (500, 4)).astype(np.float32)
    y = np.sort(rng.uniform(0, 9, (500, 8)).astype(np.float32), axis=1)
    o = np.empty(500, np.float32)
    assert oracle.oracle_model_prior_log_prob(C.byref(desc), theta.ctypes.data, 500, o.ctypes.data) == 0
    assert np.array_equal(bits(m.prior_log_prob(torch.from_numpy(theta).cuda()).cpu().numpy()), bits(o))
    assert np.isinf(o).any() and np.isfinite(o).any()
    assert oracle.oracle_model_log_kernel(C.byref(desc), y.ctypes.data, 500, o.ctypes.data) == 0
    assert np.array_equal(bits(m.calculate_log_kernel(torch.from_numpy(y).cuda()).cpu().numpy()), bits(o))
    assert oracle.oracle_model_discrepancy(C.byref(desc), y.ctypes.data, 500, o.ctypes.data) == 0
    assert np.array_equal(bits(m.discrepancy(torch.from_numpy(y).cuda()).cpu().numpy()), bits(o))


def test_gk_posterior_concentrates(hip):
    """GLMCMC on the g-and-k model through the public API: chains started from the prior move toward the
    parameters that generated y_obs (A = 3, B = 1)."""
    import glabcmcmc_amd as g
    from glabcmcmc_amd.examples.GK import GK_set
    m = GK_set(0.6)
    torch.manual_seed(0)
    n = 4096
    theta0 = torch.rand(n, 4) * 10
    y0 = m.generate_samples(theta0)
    lp = g.DiagGaussian(4, torch.zeros(1, 4), torch.log(torch.tensor([0.15, 0.1, 0.2, 0.1])))
    ip = g.Uniform(4, torch.zeros(4), torch.full((4,), 10.0))
    out = g.GLMCMC(m, 3000, theta0, y0, lp, None, 0.7, ip, 8, seed=5, return_device=True)
    late = out[2000:].mean(dim=(0, 1)).cpu().numpy()
    assert abs(late[0] - 3.0) < 0.35 and abs(late[1] - 1.0) < 0.6, late


@pytest.mark.parametrize("lanes", [1, 2, 4])
@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 6, 8, 13, 16])
def test_lanes_per_chain_is_only_geometry(hip, oracle, N, lanes):
    """1, 2 or 4 lanes cooperating on a chain (glabc_run.lanes_per_chain) give the oracle's bits."""
    cfg = dict(epsilon=0.2, local=("gauss", [0, 0], [0.35, 0.35]), **{"global": ("gauss", [0.1, -0.1], [1.0, 1.25])})
    model, local, glob = descriptors(cfg)
    rng = np.random.default_rng(1000 * N + lanes)
    n, T = 333, 120
    theta0 = rng.standard_normal((n, 2)).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((n, 2))).astype(np.float32)
    hist, chains, _ = hip_run("glmcmc", model, local, glob, theta0, y0, T, 7 + N, 0.75, N, chain0=3, lanes=lanes)
    hh, hc, _ = oracle_run(oracle, "glmcmc", model, local, glob, theta0, y0, T, 7 + N, 0.75, N, chain0=3)
    same = bits(hist) == bits(hh)
    assert same.all(), "first mismatch at (t, dim, chain) = %s" % (np.argwhere(~same)[0],)
    assert_same_state(chains, hc, True)
    assert hc.n_moves.sum() > 0


TEAM_CASES = [
    # d, N, gf, eps, local, global, chains, T
    (2, 5, 0.9, 0.05, ("gauss", [0, 0], [0.35, 0.35]), ("gauss", [0, 0], [1, 1]), 1000, 300),       # the bench configuration
    (2, 2, 0.75, 0.2, ("gauss", [0, 0], [0.35, 0.35]), ("gauss", [0.1, -0.1], [1.0, 1.25]), 333, 120),
    (2, 3, 0.75, 0.2, ("gauss", [0, 0], [0.35, 0.35]), ("gauss", [0.1, -0.1], [1.0, 1.25]), 64, 120),
    (2, 4, 1.0, 0.3, ("uniform", [-0.5, -0.5], [0.5, 0.5]), ("uniform", [-3, -3], [3, 3]), 130, 150),
    (2, 6, 0.0, 0.3, ("gauss", [0, 0], [0.5, 0.5]), ("gauss", [0, 0], [1, 1]), 65, 100),
    (2, 8, 0.8, 0.2, ("gauss", [0, 0], [0.35, 0.35]), ("gauss", [0, 0], [1, 1]), 512, 150),
    (2, 13, 0.8, 0.2, ("gauss", [0, 0], [0.35, 0.35]), ("uniform", [-3, -3], [3, 3]), 200, 100),
    (2, 16, 0.8, 0.2, ("gauss", [0, 0], [0.35, 0.35]), ("gauss", [0, 0], [1, 1]), 1, 100),
    (1, 5, 0.7, 0.3, ("gauss", [0], [0.4]), ("gauss", [0], [1]), 300, 150),
    (3, 5, 0.7, 0.3, ("gauss", [0, 0, 0], [0.4, 0.3, 0.2]), ("gauss", [0, 0, 0], [1, 1, 1]), 300, 150),
    (3, 7, 0.7, 0.3, ("uniform", [-0.4] * 3, [0.4] * 3), ("gauss", [0.1, 0, -0.1], [1.2, 0.9, 1]), 129, 100),
    (4, 5, 0.7, 0.3, ("gauss", [0] * 4, [0.3] * 4), ("gauss", [0] * 4, [1] * 4), 300, 150),
    # theta_dim 4 on both sides of the LDS limit (tests/test_launch_plan.py pins which kernel each row reaches): N = 8 runs teams
    # of two and three wavefronts, N = 11 of two only, and N = 12 fits no team -- the launch falls through to sampler_kernel
    (4, 8, 0.7, 0.3, ("gauss", [0] * 4, [0.3] * 4), ("gauss", [0] * 4, [1] * 4), 300, 150),
    (4, 11, 0.7, 0.3, ("gauss", [0] * 4, [0.3] * 4), ("uniform", [-3] * 4, [3] * 4), 100, 80),
    (4, 12, 0.7, 0.3, ("gauss", [0] * 4, [0.3] * 4), ("uniform", [-3] * 4, [3] * 4), 100, 80),
]


@pytest.mark.parametrize("waves", [2, 3, 4])
@pytest.mark.parametrize("case", TEAM_CASES, ids=lambda c: "d%d-N%d-gf%g-%s" % (c[0], c[1], c[2], c[5][0]))
def test_team_geometry_is_only_geometry(hip, oracle, case, waves, monkeypatch):
    """glabc_team.h: two to four wavefronts per 64 chains -- one keeps the chains and decides, the others evaluate candidates
    one iteration ahead -- forced with GLABC_DEBUG_TEAM (GLABC_TEAM_WAVES picks the team size; the library falls back to a
    smaller team when the batch cannot be split that far): histories, states, counters and sums equal the CPU checker's, and
    with them sampler_kernel's, bit for bit; several launches, ragged last workgroup, chain id offset."""
    monkeypatch.setenv("GLABC_TEAM_WAVES", str(waves))
    from glabcmcmc_amd import _capi as A
    from glabcmcmc_amd import distribution
    d, N, gf, eps, lspec, gspec, n, T = case
    if d == 2:
        model, local, glob = descriptors(dict(epsilon=eps, local=lspec, **{"global": gspec}))
    else:
        prior = distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d)).descriptor()
        noise = distribution.DiagGaussian(d, torch.zeros(d), torch.log(torch.full((d,), 0.05).sqrt())).descriptor()
        kern = distribution.DiagGaussian(1, torch.tensor([0.0]), torch.log(torch.tensor([eps]))).descriptor()
        model = A.Model()
        model.sim_kind, model.theta_dim, model.y_dim = A.SIM_ABS_GAUSS, d, d
        model.prior, model.noise = prior, noise
        for j in range(d):
            model.y_obs[j] = 1.5 - 0.25 * j
        model.kern_log_scale, model.kern_scale, model.kern_c0, model.epsilon = kern.p1[0], kern.p2[0], kern.c0, eps
        local, glob = make_dist(lspec).descriptor(), make_dist(gspec).descriptor()
    rng = np.random.default_rng(31 * N + d)
    theta0 = rng.standard_normal((n, d)).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((n, d))).astype(np.float32)
    seed, chain0 = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40))
    hist, chains, mom = hip_run("glmcmc", model, local, glob, theta0, y0, T, seed, gf, N, chain0=chain0, moments=True,
                                steps_per_launch=41, debug_flags=A.DEBUG_TEAM)
    hh, hc, hm = oracle_run(oracle, "glmcmc", model, local, glob, theta0, y0, T, seed, gf, N, chain0=chain0, moments=True)
    same = bits(hist) == bits(hh)
    assert same.all(), "first mismatch at (t, dim, chain) = %s" % (np.argwhere(~same)[0],)
    assert_same_state(chains, hc, True)
    assert np.array_equal(mom.sum_theta.cpu().numpy(), hm.sum_theta)
    assert np.array_equal(mom.sum_jump.cpu().numpy(), hm.sum_jump)
    assert hc.n_moves.sum() > 0
    if waves == 2:          # and the one-wavefront kernel, forced the other way
        hist1, chains1, _ = hip_run("glmcmc", model, local, glob, theta0, y0, T, seed, gf, N, chain0=chain0,
                                    steps_per_launch=41, debug_flags=A.DEBUG_NO_TEAM)
        assert np.array_equal(bits(hist1), bits(hist))


GLOBAL_TEAM_CASES = [
    # d, gf, eps, local, global, chains, T
    (2, 0.5, 0.05, ("gauss", [0, 0], [0.35, 0.35]), ("gauss", [0, 0], [1, 1]), 1000, 300),          # the bench configuration (unit variant)
    (2, 0.3, 0.2, ("gauss", [0, 0], [0.35, 0.35]), ("gauss", [0.1, -0.1], [1.0, 1.25]), 333, 200),
    (2, 0.7, 0.3, ("uniform", [-0.5, -0.5], [0.5, 0.5]), ("uniform", [-3, -3], [3, 3]), 130, 200),
    (2, 0.5, 0.3, ("uniform", [-0.5, -0.5], [0.5, 0.5]), ("gauss", [0, 0], [1.2, 1.2]), 65, 200),   # normals on one branch, uniforms on the other
    (2, 1.0, 0.3, ("gauss", [0, 0], [0.5, 0.5]), ("gauss", [0, 0], [1, 1]), 64, 100),
    (2, 0.0, 0.3, ("gauss", [0, 0], [0.5, 0.5]), ("gauss", [0, 0], [1, 1]), 1, 100),
    (1, 0.5, 0.3, ("gauss", [0], [0.4]), ("gauss", [0], [1]), 300, 150),
    (3, 0.5, 0.3, ("uniform", [-0.4] * 3, [0.4] * 3), ("gauss", [0.1, 0, -0.1], [1.2, 0.9, 1]), 129, 150),
    (4, 0.5, 0.3, ("gauss", [0] * 4, [0.3] * 4), ("uniform", [-3] * 4, [3] * 4), 300, 150),
]


@pytest.mark.parametrize("waves", [2, 3])
@pytest.mark.parametrize("case", GLOBAL_TEAM_CASES, ids=lambda c: "d%d-gf%g-%s-%s" % (c[0], c[1], c[3][0], c[4][0]))
def test_globalmcmc_team_geometry_is_only_geometry(hip, oracle, case, waves, monkeypatch):
    """global_team_kernel (glabc_team.h): GlobalMCMC with two wavefronts per 64 chains -- the helper draws an iteration's random
    numbers (branch, log u, proposal draws, simulator normals) one iteration ahead, the main wavefront does the rest -- forced
    with GLABC_DEBUG_TEAM: histories, states, move counts and sums equal the CPU checker's and the one-wavefront kernel's, bit
    for bit; several launches, ragged last workgroup, chain id offset.  Two wavefronts (one helper), or three (one helper draws
    the step head, the other the candidate's numbers; with a Gaussian proposal on one branch and a Uniform one on the other it
    draws the branch as well)."""
    monkeypatch.setenv("GLABC_TEAM_WAVES", str(waves))
    from glabcmcmc_amd import _capi as A
    from glabcmcmc_amd import distribution
    d, gf, eps, lspec, gspec, n, T = case
    if d == 2:
        model, local, glob = descriptors(dict(epsilon=eps, local=lspec, **{"global": gspec}))
    else:
        prior = distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d)).descriptor()
        noise = distribution.DiagGaussian(d, torch.zeros(d), torch.log(torch.full((d,), 0.05).sqrt())).descriptor()
        kern = distribution.DiagGaussian(1, torch.tensor([0.0]), torch.log(torch.tensor([eps]))).descriptor()
        model = A.Model()
        model.sim_kind, model.theta_dim, model.y_dim = A.SIM_ABS_GAUSS, d, d
        model.prior, model.noise = prior, noise
        for j in range(d):
            model.y_obs[j] = 1.5 - 0.25 * j
        model.kern_log_scale, model.kern_scale, model.kern_c0, model.epsilon = kern.p1[0], kern.p2[0], kern.c0, eps
        local, glob = make_dist(lspec).descriptor(), make_dist(gspec).descriptor()
    rng = np.random.default_rng(37 + d)
    theta0 = rng.standard_normal((n, d)).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((n, d))).astype(np.float32)
    seed, chain0 = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40))
    hist, chains, mom = hip_run("globalmcmc", model, local, glob, theta0, y0, T, seed, gf, 1, chain0=chain0, moments=True,
                                steps_per_launch=41, debug_flags=A.DEBUG_TEAM)
    hh, hc, hm = oracle_run(oracle, "globalmcmc", model, local, glob, theta0, y0, T, seed, gf, 1, chain0=chain0, moments=True)
    same = bits(hist) == bits(hh)
    assert same.all(), "first mismatch at (t, dim, chain) = %s" % (np.argwhere(~same)[0],)
    assert_same_state(chains, hc, False)
    assert np.array_equal(mom.sum_theta.cpu().numpy(), hm.sum_theta)
    assert np.array_equal(mom.sum_jump.cpu().numpy(), hm.sum_jump)
    assert hc.n_moves.sum() > 0
    hist1, chains1, _ = hip_run("globalmcmc", model, local, glob, theta0, y0, T, seed, gf, 1, chain0=chain0,
                                steps_per_launch=41, debug_flags=A.DEBUG_NO_TEAM)
    assert np.array_equal(bits(hist1), bits(hist))


def test_globalmcmc_team_reproduces_reference_chains_and_gk(hip, oracle):
    """the reference's golden GlobalMCMC chains (Mixture_set and the g-and-k Model) through the team geometry"""
    from glabcmcmc_amd import _capi as A
    for name in [n for n in SAMPLER_GOLDENS if "philox" in n and "globalmcmc" in n]:
        g = load_golden(name)
        cfg = g["cfg"]
        model, local, glob = descriptors(cfg, g)
        hist, chains, _ = hip_run("globalmcmc", model, local, glob, g["theta0"], g["y0"], cfg["T"], cfg["seed"], cfg["gf"], 1,
                                  chain0=cfg.get("chain0", 0), debug_flags=A.DEBUG_TEAM)
        want = g["chains"][1:].transpose(0, 2, 1)              # (T, d, n)
        assert (bits(hist) == bits(want)).all(), name


@pytest.mark.parametrize("name", [n for n in SAMPLER_GOLDENS if "philox" in n and "glmcmc" in n])
def test_team_reproduces_reference_chains(hip, name):
    """The reference's golden chains through the team geometry (where the configuration has one: batch size 2 .. 16)."""
    from glabcmcmc_amd import _capi as A
    g = load_golden(name)
    cfg = g["cfg"]
    if not 2 <= cfg["N"] <= 16:
        pytest.skip("no team kernel for this batch size")
    model, local, glob = descriptors(cfg, g)
    hist, chains, _ = hip_run(str(g["algo"]), model, local, glob, g["theta0"], g["y0"], cfg["T"], cfg["seed"],
                              cfg["gf"], cfg["N"], chain0=cfg.get("chain0", 0), debug_flags=A.DEBUG_TEAM)
    got = np.concatenate([g["theta0"][None], hist.transpose(0, 2, 1)], axis=0)
    same = bits(got) == bits(g["chains"])
    assert same.all(), "first mismatch at (t, chain, dim) = %s" % (np.argwhere(~same)[0],)


@pytest.mark.parametrize("d,N", [(1, 5), (3, 5), (4, 5), (5, 5), (6, 3), (7, 16), (8, 5), (8, 16), (5, 1), (8, 2)])
def test_other_dimensions(hip, oracle, d, N):
    """theta_dim 1 .. 8 (the Model is |theta| + noise in any dimension; 5 .. 8 are the default-schedule objects)."""
    from glabcmcmc_amd import _capi as A
    from glabcmcmc_amd import distribution
    prior = distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d)).descriptor()
    noise = distribution.DiagGaussian(d, torch.zeros(d), torch.log(torch.full((d,), 0.05).sqrt())).descriptor()
    kern = distribution.DiagGaussian(1, torch.tensor([0.0]), torch.log(torch.tensor([0.3]))).descriptor()
    model = A.Model()
    model.sim_kind, model.theta_dim, model.y_dim = A.SIM_ABS_GAUSS, d, d
    model.prior, model.noise = prior, noise
    for j in range(d):
        model.y_obs[j] = 1.5 - 0.25 * j
    model.kern_log_scale, model.kern_scale, model.kern_c0, model.epsilon = kern.p1[0], kern.p2[0], kern.c0, 0.3
    local = make_dist(("gauss", [0.0] * d, [0.35] * d)).descriptor()
    glob = make_dist(("gauss", [0.1 * j for j in range(d)], [1.0 + 0.1 * j for j in range(d)])).descriptor()
    rng = np.random.default_rng(d)
    n, T = 1030, 150 if d <= 4 else 60
    theta0 = rng.standard_normal((n, d)).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((n, d))).astype(np.float32)
    for algo, lanes in (("glmcmc", 0), ("glmcmc", 1), ("glmcmc", 2), ("glmcmc", 4), ("globalmcmc", 0)):
        if (lanes == 2 and N < 2) or (lanes == 4 and N < 3):
            continue
        hist, chains, _ = hip_run(algo, model, local, glob, theta0, y0, T, 99 + d, 0.6, N, lanes=lanes)
        hh, hc, _ = oracle_run(oracle, algo, model, local, glob, theta0, y0, T, 99 + d, 0.6, N)
        assert np.array_equal(bits(hist), bits(hh))
        assert_same_state(chains, hc, algo == "glmcmc")
        assert hc.n_moves.sum() > 0


def test_launch_geometry_and_sharding_invariance(hip):
    """Results do not depend on iterations-per-launch nor on how chains are split over
    calls / GPUs: two shards with chain0 offsets equal one big call (the multi-GPU contract)."""
    cfg = dict(epsilon=0.3, local=("gauss", [0, 0], [0.35, 0.35]), **{"global": ("gauss", [0, 0], [1, 1])})
    model, local, glob = descriptors(cfg)
    rng = np.random.default_rng(5)
    n, T, N, seed = 3000, 120, 5, 424242
    theta0 = rng.standard_normal((n, 2)).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((n, 2))).astype(np.float32)
    ref, c_ref, _ = hip_run("glmcmc", model, local, glob, theta0, y0, T, seed, 0.8, N, chain0=10)
    a, c_a, _ = hip_run("glmcmc", model, local, glob, theta0, y0, T, seed, 0.8, N, chain0=10, steps_per_launch=7)
    assert np.array_equal(bits(a), bits(ref))
    assert np.array_equal(bits(c_a.log_w.cpu().numpy()), bits(c_ref.log_w.cpu().numpy()))
    k = 1111
    s0, _, _ = hip_run("glmcmc", model, local, glob, theta0[:k], y0[:k], T, seed, 0.8, N, chain0=10)
    s1, _, _ = hip_run("glmcmc", model, local, glob, theta0[k:], y0[k:], T, seed, 0.8, N, chain0=10 + k)
    assert np.array_equal(bits(np.concatenate([s0, s1], axis=2)), bits(ref))
    other, _, _ = hip_run("glmcmc", model, local, glob, theta0, y0, T, seed + 1, 0.8, N, chain0=10)
    assert not np.array_equal(other, ref)


def test_empty_and_ragged_inputs(hip):
    cfg = dict(epsilon=0.3, local=("gauss", [0, 0], [0.35, 0.35]), **{"global": ("gauss", [0, 0], [1, 1])})
    model, local, glob = descriptors(cfg)
    rng = np.random.default_rng(6)
    for n in (1, 63, 65):                       # not multiples of the wavefront
        theta0 = rng.standard_normal((n, 2)).astype(np.float32)
        y0 = np.abs(theta0).astype(np.float32)
        hist, chains, _ = hip_run("glmcmc", model, local, glob, theta0, y0, 40, 3, 0.8, 5)
        assert hist.shape == (40, 2, n) and np.isfinite(hist).all()
    # zero iterations: state untouched
    theta0 = rng.standard_normal((10, 2)).astype(np.float32)
    _, chains, _ = hip_run("glmcmc", model, local, glob, theta0, np.abs(theta0), 0, 3, 0.8, 5, history=False)
    assert np.array_equal(chains.theta.cpu().numpy().T, theta0)


def test_bad_arguments_are_refused(hip):
    from glabcmcmc_amd import _capi as A
    from glabcmcmc_amd import engine
    cfg = dict(epsilon=0.3, local=("gauss", [0, 0], [0.35, 0.35]), **{"global": ("gauss", [0, 0], [1, 1])})
    model, local, glob = descriptors(cfg)
    dev = torch.device("cuda", 0)
    chains = engine.ChainBatch(torch.zeros(8, 2), torch.zeros(8, 2), dev)
    cs = chains.struct()

    def call(m=model, lo=local, g=glob, c=cs, **kw):
        run = A.Run()
        run.seed, run.step0, run.n_steps, run.global_frequency, run.batch_size = 1, 1, 4, 0.5, 5
        for k, v in kw.items():
            setattr(run, k, v)
        return hip.glabc_glmcmc_steps(C.byref(m), C.byref(lo), C.byref(g), C.byref(c), C.byref(run), None)

    assert call() == 0
    assert call(batch_size=0) == -4 and call(batch_size=4097) == -4 and call(n_steps=-1) == -4
    assert call(batch_size=17, lanes_per_chain=2) == -4 and call(batch_size=5, lanes_per_chain=8) == -4
    bad = make_dist(("gauss", [0, 0], [1, 1])).descriptor()
    bad.p2[0] = float("nan")
    assert call(g=bad) == -4
    bad3 = make_dist(("gauss", [0, 0, 0], [1, 1, 1])).descriptor()
    assert call(g=bad3) == -2
    nul = chains.struct()
    nul.theta = None
    assert call(c=nul) == -1
    assert hip.glabc_status_string(-4) == b"bad argument"
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------- GLMALA
def hip_glmala(model, glob, mala, theta0, y0, T, seed, gf, N, chain0=0, steps_per_launch=None, moments=False, lanes=0):
    from glabcmcmc_amd import engine
    dev = torch.device("cuda", 0)
    chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev, chain0=chain0).add_mala_state()
    engine.glmala_init(model, chains)
    hist = torch.empty(T, chains.d, chains.n, dtype=torch.float32, device=dev)
    mom = engine.Moments(chains.n, chains.d, dev) if moments else None
    engine.run_glmala_steps(model, glob, mala, chains, T, 1, seed, gf, N, history=hist, moments=mom,
                            steps_per_launch=steps_per_launch, lanes_per_chain=lanes)
    torch.cuda.synchronize()
    return hist.cpu().numpy(), chains, mom


def oracle_glmala(oracle, model, glob, mala, theta0, y0, T, seed, gf, N, chain0=0, moments=False):
    hc = oracle_lib.HostChains(theta0, y0, chain0=chain0).add_mala_state()
    hh = np.zeros((T, theta0.shape[1], theta0.shape[0]), np.float32)
    mom = oracle_lib.HostMoments(theta0.shape[0], theta0.shape[1]) if moments else None
    run, keep = oracle_lib.make_run(seed=seed, step0=1, n_steps=T, gf=gf, batch=N, history=hh, moments=mom)
    cs = hc.struct()
    assert oracle.oracle_glmala_init(C.byref(model), C.byref(cs)) == 0
    assert oracle.oracle_glmala_steps(C.byref(model), C.byref(glob), C.byref(mala), C.byref(cs), C.byref(run)) == 0
    return hh, hc, mom


@pytest.mark.parametrize("name", GLMALA_GOLDENS_EXACT)
def test_hip_glmala_reproduces_reference_chains(hip, name):
    """GLMALA kernel vs the reference's chains (reference run with a correctly rounded torch.sqrt,
    see tests/golden/make_golden.py and DESIGN.md): bit for bit."""
    g = load_golden(name)
    cfg = g["cfg"]
    model, _, glob = descriptors(cfg, g)
    hist, chains, _ = hip_glmala(model, glob, mala_params(cfg), g["theta0"], g["y0"], cfg["T"], cfg["seed"], cfg["gf"],
                                 cfg["N"], chain0=cfg.get("chain0", 0))
    got = np.concatenate([g["theta0"][None], hist.transpose(0, 2, 1)], axis=0)
    same = bits(got) == bits(g["chains"])
    assert same.all(), "first mismatch at (t, chain, dim) = %s" % (np.argwhere(~same)[0],)


@pytest.mark.parametrize("name", GLMALA_GOLDENS_MKL)
def test_hip_glmala_vs_unpatched_reference(hip, name):
    """The GLMALA KERNEL against the reference exactly as it runs (its own torch.sqrt -- MKL VML, 1 ulp low for 0.65 % of
    float32 inputs): every chain follows the reference bit for bit until its first sqrt-ulp event, that first difference is
    a few float32 ulp, and the number of accepted moves stays within 1 % -- the divergence profile the CPU checker shows
    (tests/test_oracle_golden.py::test_glmala_vs_unpatched_reference), now on the HIP path."""
    from test_oracle_golden import divergence_profile
    g = load_golden(name)
    cfg = g["cfg"]
    model, _, glob = descriptors(cfg, g)
    hist, chains, _ = hip_glmala(model, glob, mala_params(cfg), g["theta0"], g["y0"], cfg["T"], cfg["seed"], cfg["gf"],
                                 cfg["N"], chain0=cfg.get("chain0", 0))
    got = np.concatenate([g["theta0"][None], hist.transpose(0, 2, 1)], axis=0)
    ref = g["chains"]
    first, ulp = divergence_profile(got, ref)
    assert (first >= 1).all()
    assert ulp.max() <= 16.0 and (not (ulp > 0).any() or np.median(ulp[ulp > 0]) <= 2.0), ulp
    if name == "glmala_philox_bench":                   # BASELINE config 3
        assert (first == ref.shape[0]).mean() >= 0.75
    moves_ref = (np.diff(ref, axis=0) != 0).any(-1).sum()
    moves_got = int(chains.n_moves.cpu().numpy().astype(np.int64).sum())
    assert abs(moves_got - int(moves_ref)) <= 0.01 * moves_ref + 1


MALA_CASES = [
    # N, gf, eps, tau, num_grad, global, chains, T
    (5, 0.8, 0.05, 0.3, 100, ("gauss", [0, 0], [1, 1]), 512, 60),
    (3, 0.3, 0.3, 0.25, 10, ("gauss", [0, 0], [1, 1]), 700, 150),
    (2, 0.0, 0.3, 0.2, 7, ("gauss", [0.1, 0.2], [1.2, 0.8]), 333, 100),
    (4, 0.5, 0.3, 0.3, 12, ("uniform", [-3, -3], [3, 3]), 640, 120),
    (8, 0.6, 0.2, 0.3, 5, ("gauss", [0, 0], [1, 1]), 256, 100),
    (1, 1.0, 0.3, 0.3, 4, ("gauss", [0, 0], [1, 1]), 256, 60),
]


@pytest.mark.parametrize("lanes", [1, 2])      # 64 / 32 chains per wavefront (glabc_mala.h glmala_kernel CPW)
@pytest.mark.parametrize("case", MALA_CASES, ids=lambda c: "N%d-gf%g-num%d-%s" % (c[0], c[1], c[4], c[5][0]))
def test_hip_glmala_equals_oracle(hip, oracle, case, lanes):
    N, gf, eps, tau, num, gspec, n, T = case
    cfg = dict(epsilon=eps, tau=tau, num_grad=num, local=("gauss", [0, 0], [1, 1]), **{"global": gspec})
    model, _, glob = descriptors(cfg)
    if N == 3:
        model.y_obs[0] = 1e-3           # an observation near zero: the kernels with the general square root
    mala = mala_params(cfg)
    rng = np.random.default_rng(n + T)
    theta0 = rng.standard_normal((n, 2)).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((n, 2))).astype(np.float32)
    seed, chain0 = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40))
    hist, chains, mom = hip_glmala(model, glob, mala, theta0, y0, T, seed, gf, N, chain0=chain0, moments=True,
                                   steps_per_launch=37, lanes=lanes)
    hh, hc, hm = oracle_glmala(oracle, model, glob, mala, theta0, y0, T, seed, gf, N, chain0=chain0, moments=True)
    same = bits(hist) == bits(hh)
    assert same.all(), "first mismatch at (t, dim, chain) = %s" % (np.argwhere(~same)[0],)
    # the float64 state, bit for bit
    assert np.array_equal(chains.theta64.cpu().numpy(), hc.theta64)
    assert np.array_equal(chains.y64.cpu().numpy(), hc.y64)
    assert np.array_equal(chains.log_w64.cpu().numpy(), hc.log_w64)
    assert np.array_equal(chains.grad.cpu().numpy(), hc.grad)
    assert np.array_equal(chains.flags.cpu().numpy().astype(np.uint32), hc.flags)
    assert np.array_equal(chains.n_moves.cpu().numpy().astype(np.uint32), hc.n_moves)
    assert np.array_equal(mom.sum_jump.cpu().numpy(), hm.sum_jump)
    assert np.array_equal(mom.sum_theta.cpu().numpy(), hm.sum_theta)
    assert np.array_equal(mom.sum_outer.cpu().numpy(), hm.sum_outer)
    assert hc.n_moves.sum() > 0


def test_glmala_function_shapes(hip):
    import glabcmcmc_amd as g
    from glabcmcmc_amd.examples.Mixture import Mixture_set
    m = Mixture_set(0.3)
    ip = g.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.tensor([0.0, 0.0]))
    one = g.GLMALA(m, 50, torch.tensor([0.0, 0.0]), torch.tensor([[1.4, 1.6]]), 0.3, 10, None, 0.8, ip, 5, seed=3,
                   verbose=False)
    assert one.shape == (50, 2) and one.device.type == "cpu" and one.dtype == torch.float32
    many = g.GLMALA(m, 30, torch.zeros(100, 2), torch.full((100, 2), 1.5), 0.3, 10, None, 0.8, ip, 5, seed=3)
    assert many.shape == (30, 100, 2)


# ---------------------------------------------------------------------------------- primitives
@pytest.fixture(scope="module")
def prim():
    return load_golden("primitives")


def test_distribution_log_prob_on_gpu(hip, prim):
    from glabcmcmc_amd import distribution
    for tag in ("std", "lp", "gen", "d1", "d4", "d7", "d8"):
        loc = torch.from_numpy(prim["dg_%s_loc" % tag])
        g = distribution.DiagGaussian(len(loc), loc, torch.from_numpy(prim["dg_%s_log_scale" % tag]))
        # exp(log_scale) as the machine that produced the golden values computed it (torch's CPU exp differs in
        # the last bit between CPU types); through the C ABI directly
        desc = g.descriptor()
        for j in range(desc.dim):
            desc.p2[j] = float(prim["dg_%s_scale" % tag][j])
        z = torch.from_numpy(prim["dg_%s_z" % tag]).cuda()
        o = torch.empty(z.shape[0], dtype=torch.float32, device="cuda")
        assert hip.glabc_dist_log_prob(C.byref(desc), z.data_ptr(), z.shape[0], o.data_ptr(), None) == 0
        assert np.array_equal(bits(o.cpu().numpy()), bits(prim["dg_%s_log_prob" % tag])), tag
        assert g.log_prob(z).shape == (z.shape[0],)                  # the host-mirror path runs too
    for tag in ("box", "inc", "d4"):
        g = distribution.Uniform(len(prim["un_%s_low" % tag]), torch.from_numpy(prim["un_%s_low" % tag]),
                                 torch.from_numpy(prim["un_%s_high" % tag]))
        out = g.log_prob(torch.from_numpy(prim["un_%s_z" % tag]).cuda()).cpu().numpy()
        assert np.array_equal(bits(out), bits(prim["un_%s_log_prob" % tag])), tag


@pytest.mark.parametrize("eps", [0.05, 0.3])
def test_model_callbacks_on_gpu(hip, oracle, prim, eps):
    from glabcmcmc_amd.examples.Mixture import Mixture_set
    m = Mixture_set(eps)
    tag = "mix_%g" % eps
    theta = torch.from_numpy(prim[tag + "_theta"]).cuda()
    y = torch.from_numpy(prim[tag + "_y"]).cuda()
    assert np.array_equal(bits(m.prior_log_prob(theta).cpu().numpy()), bits(prim[tag + "_prior"]))
    desc = m.descriptor()
    n = y.shape[0]
    o = np.empty(n, np.float32)
    yy = prim[tag + "_y"]
    assert oracle.oracle_model_discrepancy(C.byref(desc), yy.ctypes.data, n, o.ctypes.data) == 0
    assert np.array_equal(bits(m.discrepancy(y).cpu().numpy()), bits(o))
    assert oracle.oracle_model_log_kernel(C.byref(desc), yy.ctypes.data, n, o.ctypes.data) == 0
    got = m.calculate_log_kernel(y).cpu().numpy()
    assert np.array_equal(bits(got), bits(o))
    ref = prim[tag + "_logk"]
    assert np.all(np.abs(got - ref) <= 4e-7 * np.maximum(np.abs(ref), 1.0))


def test_esjd_kernel(hip, oracle, prim):
    from glabcmcmc_amd import esjd
    from test_esjd_shapes import ESJD_RTOL
    i = 0
    while "esjd_chain_%d" % i in prim:
        x = prim["esjd_chain_%d" % i]
        ref = prim["esjd_value_%d" % i]
        got = esjd(torch.from_numpy(x))
        assert got.shape == () and got.dtype == np.float32
        # the stored values are torch's float32 results: within 1.9e-7 of the float64 value for all nine chains (condition
        # numbers 1 .. 13), so the measured bound of tests/test_esjd_shapes.py holds here too (it was 2e-5, and 2e-4 above d = 4)
        assert abs(got - ref) <= ESJD_RTOL * abs(ref), (i, got, ref)
        i += 1
    assert i >= 9                                          # theta_dim 5, 6 and 8 included
    assert esjd(torch.tensor([[0, 0], [1, 0], [1, 2], [1, 2], [0, 1.0]])) == np.float32(0.75)


def test_esjd_from_history_equals_streamed_moments(hip):
    from glabcmcmc_amd.ESJD import esjd_per_chain
    cfg = dict(epsilon=0.3, local=("gauss", [0, 0], [0.35, 0.35]), **{"global": ("gauss", [0, 0], [1, 1])})
    model, local, glob = descriptors(cfg)
    rng = np.random.default_rng(8)
    n, T = 2048, 400
    theta0 = rng.standard_normal((n, 2)).astype(np.float32)
    y0 = np.abs(theta0).astype(np.float32)
    hist, chains, mom = hip_run("glmcmc", model, local, glob, theta0, y0, T, 17, 0.8, 5, moments=True)
    full = torch.from_numpy(np.concatenate([theta0.T[None], hist], axis=0)).cuda()
    a = esjd_per_chain(full).cpu().numpy()
    b = mom.esjd().cpu().numpy()
    assert np.allclose(a, b, rtol=1e-5, atol=1e-9)
    assert (a > 0).mean() > 0.9


# ---------------------------------------------------------------------------------- (3)
def test_full_size_bit_parity_and_posterior(hip, oracle):
    """BASELINE config 2 at full width: 65 536 chains, GLMCMC iSIR N=5, gf 0.9, eps 0.05.
    (a) the first 150 iterations of ALL chains equal the CPU oracle bit for bit;
    (b) after burn-in the pooled posterior moments match the analytic ABC posterior
        (|theta_i| ~ N(1.425178, 0.049881)) and ESJD from streamed
        moments equals ESJD from the recorded history within 1e-3."""
    from glabcmcmc_amd.ESJD import esjd_per_chain
    cfg = dict(epsilon=0.05, local=("gauss", [0, 0], [0.35, 0.35]), **{"global": ("gauss", [0, 0], [1, 1])})
    model, local, glob = descriptors(cfg)
    n, N, gf, seed = 65536, 5, 0.9, 20261003
    rng = np.random.default_rng(1)
    theta0 = np.zeros((n, 2), np.float32)
    y0 = (0.2236068 * rng.standard_normal((n, 2))).astype(np.float32)
    T0 = 150
    hist, chains, _ = hip_run("glmcmc", model, local, glob, theta0, y0, T0, seed, gf, N)
    hh, hc, _ = oracle_run(oracle, "glmcmc", model, local, glob, theta0, y0, T0, seed, gf, N)
    assert np.array_equal(bits(hist), bits(hh))
    assert_same_state(chains, hc, True)
    # burn in (no history), then 1500 recorded iterations with streamed moments
    hip_run("glmcmc", model, local, glob, None, None, 2350, seed, gf, N, chains=chains, step0=1 + T0, history=False)
    start = chains.theta.clone()
    T1 = 1500
    hist, chains, mom = hip_run("glmcmc", model, local, glob, None, None, T1, seed, gf, N, chains=chains,
                                step0=1 + T0 + 2350, moments=True)
    mean_abs = np.abs(hist).mean()
    mean_sq = (hist.astype(np.float64) ** 2).mean()
    assert abs(mean_abs - 1.425178) / 1.425178 < 2e-3, mean_abs
    assert abs(mean_sq - 2.081014) / 2.081014 < 3e-3, mean_sq
    assert abs(hist.mean()) < 0.02                                    # four symmetric modes
    sq = mom.second_moment().cpu().numpy()
    assert abs((sq[:, 0, 0].mean() + sq[:, 1, 1].mean()) / 2 - mean_sq) / mean_sq < 1e-6
    full = torch.cat([start[None], torch.from_numpy(hist).cuda()], dim=0)
    e_hist = esjd_per_chain(full).cpu().numpy().astype(np.float64)
    e_mom = mom.esjd().cpu().numpy().astype(np.float64)
    # a chain with fewer than two independent jumps has a singular jump matrix: det = +-rounding,
    # and det ** (1/2) is NaN for the negative ones -- in ESJD.py:24 as well as here
    ok = np.isfinite(e_hist) & np.isfinite(e_mom)
    assert ok.mean() > 0.97
    assert abs(e_hist[ok].mean() - e_mom[ok].mean()) / e_hist[ok].mean() < 1e-3
    assert 0.001 < e_hist[ok].mean() < 1.0


def test_gamma_log_prob_on_gpu(hip, oracle, prim):
    from glabcmcmc_amd import distribution
    for tag in ("a", "b", "c"):
        g = distribution.Gamma(torch.from_numpy(prim["gm_%s_shape" % tag]), torch.from_numpy(prim["gm_%s_rate" % tag]))
        d = g.gamma_descriptor()
        z = prim["gm_%s_z" % tag]
        o = np.empty(len(z))
        assert oracle.oracle_gamma_log_prob(C.byref(d), z.ctypes.data, len(z), o.ctypes.data) == 0
        got = g.log_prob(torch.from_numpy(z).cuda()).cpu().numpy()
        assert got.dtype == np.float64
        assert np.array_equal(got.view(np.uint64), o.view(np.uint64)), tag


def test_checkpoint_resume_is_exact(hip, tmp_path):
    """save the state + Philox position mid-run, reload, continue: identical bits to the
    uninterrupted run (GLMCMC state and streaming sums; GLMALA's float64 state as well)."""
    from glabcmcmc_amd import checkpoint, engine
    cfg = dict(epsilon=0.3, tau=0.3, num_grad=8, local=("gauss", [0, 0], [0.35, 0.35]), **{"global": ("gauss", [0, 0], [1, 1])})
    model, local, glob = descriptors(cfg)
    rng = np.random.default_rng(12)
    n, T1, T2, N, seed = 500, 60, 45, 5, 99
    theta0 = rng.standard_normal((n, 2)).astype(np.float32)
    y0 = np.abs(theta0).astype(np.float32)
    dev = torch.device("cuda", 0)
    # uninterrupted
    full, cfull, mfull = hip_run("glmcmc", model, local, glob, theta0, y0, T1 + T2, seed, 0.8, N, moments=True)
    # interrupted at T1
    _, c1, m1 = hip_run("glmcmc", model, local, glob, theta0, y0, T1, seed, 0.8, N, moments=True)
    checkpoint.save(str(tmp_path / "ck.pt"), c1, seed, 1 + T1, moments=m1, extra={"note": "glmcmc"})
    c2, seed2, step2, m2, extra = checkpoint.load(str(tmp_path / "ck.pt"), dev)
    assert (seed2, step2, extra["note"]) == (seed, 1 + T1, "glmcmc")
    hist2 = torch.empty(T2, 2, n, dtype=torch.float32, device=dev)
    engine.run_steps("glabc_glmcmc_steps", model, local, glob, c2, T2, step2, seed2, 0.8, N, history=hist2, moments=m2)
    torch.cuda.synchronize()
    assert np.array_equal(bits(hist2.cpu().numpy()), bits(full[T1:]))
    assert np.array_equal(m2.sum_jump.cpu().numpy(), mfull.sum_jump.cpu().numpy()) and m2.steps == T1 + T2
    assert np.array_equal(bits(c2.log_w.cpu().numpy()), bits(cfull.log_w.cpu().numpy()))
    # GLMALA
    mala = mala_params(cfg)
    full, cfull, _ = hip_glmala(model, glob, mala, theta0, y0, T1 + T2, seed, 0.5, N)
    _, c1, _ = hip_glmala(model, glob, mala, theta0, y0, T1, seed, 0.5, N)
    checkpoint.save(str(tmp_path / "ck2.pt"), c1, seed, 1 + T1)
    c2, seed2, step2, _, _ = checkpoint.load(str(tmp_path / "ck2.pt"), dev)
    hist2 = torch.empty(T2, 2, n, dtype=torch.float32, device=dev)
    engine.run_glmala_steps(model, glob, mala, c2, T2, step2, seed2, 0.5, N, history=hist2)
    torch.cuda.synchronize()
    assert np.array_equal(bits(hist2.cpu().numpy()), bits(full[T1:]))
    assert np.array_equal(c2.theta64.cpu().numpy(), cfull.theta64.cpu().numpy())
    assert np.array_equal(c2.grad.cpu().numpy(), cfull.grad.cpu().numpy())
    # a checkpoint written on another random-stream layout is refused, not silently continued on a different stream
    state = torch.load(str(tmp_path / "ck2.pt"), weights_only=True)
    state["stream_layout"] = 1
    torch.save(state, str(tmp_path / "old.pt"))
    with pytest.raises(RuntimeError, match="random-stream layout"):
        checkpoint.load(str(tmp_path / "old.pt"), dev)


def test_global_frequency_sweep(hip):
    """SURVEY 8(f) f-2 (examples/Mixture_hyper.py): the sweep runs, ESJD of the iSIR mixes beats pure local moves."""
    from glabcmcmc_amd.examples.Mixture_hyper import sweep
    out = sweep(num_ite=400, chains_per_cell=1024, frequencies=[0, 0.5, 0.9, 1], seeds=[1, 2], verbose=False)
    assert out["esjd"].shape == (2, 4) and np.isfinite(out["resjd_mean"]).all()
    assert out["best_gf"] in (0, 0.5, 0.9, 1)
    assert out["esjd"][:, 2].mean() > out["esjd"][:, 0].mean()
    from glabcmcmc_amd.examples.Mixture_hyper import sweep_fused
    fused = sweep_fused(num_ite=400, chains_per_cell=1024, frequencies=[0, 0.5, 0.9, 1], seeds=[1, 2])
    assert fused.shape == (2, 4) and np.allclose(fused.mean(0), out["esjd"].mean(0), rtol=0.15)


def test_example_script_runs_every_sampler(hip, tmp_path):
    """examples/Mixture.py's __main__ (reference examples/Mixture.py:55-85) with all five runner calls enabled."""
    from glabcmcmc_amd.examples import Mixture
    chains = Mixture.main(num_ite=400, output_dir=str(tmp_path), verbose=False)
    assert set(chains) == {"global", "glmcmc", "aglmcmc", "glmala", "glmcmc_nf"}
    for name, c in chains.items():
        assert c.shape == (400, 2) and c.dtype == torch.float32 and not c.is_cuda, name
        assert torch.isfinite(c).all(), name
        assert torch.equal(c[0], torch.zeros(2)), name
    for f in ("global_mcmc_results.csv", "glmcmc_results.csv", "aglmcmc_results.csv", "glmala_results.csv", "glmcmc_nf_results.csv"):
        assert (tmp_path / f).exists(), f


def test_large_history_comes_back_through_pinned_memory(hip):
    """_host.finish: histories above 2^22 floats return as the (num_ite, C, d) view of a pinned chain-major buffer --
    the same numbers as the device result."""
    import glabcmcmc_amd as g
    from glabcmcmc_amd.examples.Mixture import Mixture_set
    m = Mixture_set(0.3)
    lp = g.DiagGaussian(2, loc=torch.zeros(1, 2), log_scale=torch.log(torch.tensor([0.35, 0.35])))
    ip = g.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.tensor([0.0, 0.0]))
    theta0 = torch.zeros(4096, 2)
    y0 = torch.zeros(4096, 2) + 0.1
    a = g.GLMCMC(m, 600, theta0, y0, lp, None, 0.7, ip, 5, seed=11)
    b = g.GLMCMC(m, 600, theta0, y0, lp, None, 0.7, ip, 5, seed=11, return_device=True)
    assert a.shape == (600, 4096, 2) and not a.is_cuda and a.is_pinned()
    assert torch.equal(a, b.cpu())


@pytest.mark.parametrize("eps,N,lanes", [(0.05, 5, 1), (0.3, 16, 1), (0.002, 3, 1), (0.05, 5, 2), (1e-4, 8, 4)])
def test_fast_index_equals_ieee_index(hip, eps, N, lanes):
    """The iSIR index from reciprocal-multiplied weights (with its IEEE-division fallback near a partial sum) gives the
    chains of the always-IEEE path (GLABC_DEBUG_EXACT_INDEX) bit for bit -- including tiny epsilon, where most weights
    underflow to 0 and the total can be 0 or denormal."""
    from glabcmcmc_amd import _capi
    cfg = dict(epsilon=eps, local=("gauss", [0, 0], [0.35, 0.35]), **{"global": ("gauss", [0, 0], [1, 1])})
    model, local, glob = descriptors(cfg)
    rng = np.random.default_rng(int(eps * 1e6) + N)
    n, T = 8192, 300
    theta0 = (rng.standard_normal((n, 2)) * 2).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2 * rng.standard_normal((n, 2))).astype(np.float32)
    fast, cf, _ = hip_run("glmcmc", model, local, glob, theta0, y0, T, 77, 0.9, N, lanes=lanes)
    exact, ce, _ = hip_run("glmcmc", model, local, glob, theta0, y0, T, 77, 0.9, N, lanes=lanes,
                           debug_flags=_capi.DEBUG_EXACT_INDEX)
    assert np.array_equal(bits(fast), bits(exact))
    assert np.array_equal(bits(cf.log_w.cpu().numpy()), bits(ce.log_w.cpu().numpy()))
    assert np.array_equal(cf.n_moves.cpu().numpy(), ce.n_moves.cpu().numpy())
    assert int(cf.n_moves.sum()) > 0


@pytest.mark.parametrize("y_obs,n,eps", [((1e-3, 2.0), 3000, 0.2), ((0.0, 0.0), 3000, 0.2), ((1.5, 1.5), 200000, 0.2),
                                         ((1.5, 1.5), 3000, 3e6), ((1.5, 1.5), 3000, 0.7311), ((1.5, 1.5), 3000, 1.9999999)])
def test_unit_gaussian_variant_and_its_fallback(hip, oracle, y_obs, n, eps):
    """The branch-free unit-Gaussian kernel variant (lean square root, no +0 log-scale terms) needs every
    |y_obs_j| >= 2^-6 and a kernel scale in [2^-20, 2^20] whose reciprocal division the host verified; other
    configurations take the generic kernels.  All against the oracle (IEEE division, full sqrt), bit for bit -- the
    large case (more than two waves per SIMD) also exercises the default-schedule object."""
    cfg = dict(epsilon=eps, local=("gauss", [0, 0], [0.35, 0.35]), **{"global": ("gauss", [0, 0], [1, 1])})
    model, local, glob = descriptors(cfg)
    for j in range(2):
        model.y_obs[j] = y_obs[j]
    rng = np.random.default_rng(5)
    T = 60 if n < 100000 else 12
    theta0 = (rng.standard_normal((n, 2)) * 0.5).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((n, 2))).astype(np.float32)
    hist, chains, _ = hip_run("glmcmc", model, local, glob, theta0, y0, T, 9, 0.8, 5)
    hh, hc, _ = oracle_run(oracle, "glmcmc", model, local, glob, theta0, y0, T, 9, 0.8, 5)
    assert np.array_equal(bits(hist), bits(hh))
    assert_same_state(chains, hc, True)
    assert hc.n_moves.sum() > 0


def test_sharded_example_is_invariant_to_the_number_of_ranks(hip):
    """examples/Mixture_sharded.py with 1 rank and with 2 ranks (gloo, both on this GPU): the same chains, hence the same
    pooled statistics to the last bit."""
    import json
    import os
    import subprocess
    import sys
    from conftest import PKG_PARENT
    env = dict(os.environ, PYTHONPATH=PKG_PARENT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    args = ["-m", "glabcmcmc_amd.examples.Mixture_sharded", "--chains", "6000", "--iters", "150", "--backend", "gloo", "--one-gpu"]
    one = subprocess.run([sys.executable] + args, env=env, capture_output=True, text=True, timeout=300)
    assert one.returncode == 0, one.stderr[-2000:]
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                          "127.0.0.1", "--master-port", "29541"] + args, env=env, capture_output=True, text=True, timeout=300)
    assert two.returncode == 0, two.stderr[-2000:]
    a = json.loads(one.stdout.strip().split("\n")[-1])
    b = json.loads([l for l in two.stdout.strip().split("\n") if l.startswith("{")][-1])
    assert (a["ranks"], b["ranks"]) == (1, 2) and a["chains"] == b["chains"] == 6000
    assert a["esjd_checksum"] == b["esjd_checksum"] and a["mean_theta_sq"] == b["mean_theta_sq"]


def test_streamed_history_equals_the_in_memory_one(hip, tmp_path):
    """streaming.stream_history: history blocks leave over a copy stream + writer thread while the next
    block is computed; the .npy file holds exactly the rows of one in-memory run, for block sizes that do and do not
    divide the run."""
    from glabcmcmc_amd import engine, streaming
    cfg = dict(epsilon=0.3, local=("gauss", [0, 0], [0.35, 0.35]), **{"global": ("gauss", [0, 0], [1, 1])})
    model, local, glob = descriptors(cfg)
    rng = np.random.default_rng(3)
    n, T, seed = 4096, 230, 17
    theta0 = rng.standard_normal((n, 2)).astype(np.float32)
    y0 = np.abs(theta0).astype(np.float32)
    full, cfull, _ = hip_run("glmcmc", model, local, glob, theta0, y0, T, seed, 0.8, 5)
    dev = torch.device("cuda", 0)
    for block in (50, 64, 1000):
        chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev)
        engine.init_weights(model, glob, chains)
        path = str(tmp_path / ("hist_%d.npy" % block))
        shape = streaming.stream_history("glabc_glmcmc_steps", model, local, glob, chains, T, seed, 0.8, 5, path, block=block)
        assert tuple(shape) == (T, 2, n)
        got = np.load(path)
        assert np.array_equal(bits(got), bits(full)), block
        assert np.array_equal(bits(chains.theta.cpu().numpy()), bits(cfull.theta.cpu().numpy()))


@pytest.mark.parametrize("algo", ["glmcmc", "globalmcmc"])
def test_per_chain_global_frequency(hip, oracle, algo):
    """glabc_run.global_frequency_per_chain: every chain with its own frequency (a hyper-parameter grid in one launch) --
    against the oracle, bit for bit; a constant array equals the scalar run; GLMALA refuses the array."""
    from glabcmcmc_amd import engine
    cfg = dict(epsilon=0.3, local=("gauss", [0, 0], [0.35, 0.35]), **{"global": ("gauss", [0, 0], [1, 1])})
    model, local, glob = descriptors(cfg)
    rng = np.random.default_rng(8)
    n, T, seed, N = 3000, 80, 21, 5 if algo == "glmcmc" else 1
    theta0 = rng.standard_normal((n, 2)).astype(np.float32)
    y0 = np.abs(theta0).astype(np.float32)
    gf = rng.choice(np.linspace(0, 1, 11), n).astype(np.float32)
    dev = torch.device("cuda", 0)
    chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev)
    if algo == "glmcmc":
        engine.init_weights(model, glob, chains)
    hist = torch.empty(T, 2, n, device=dev)
    gfg = torch.from_numpy(gf).to(dev)
    engine.run_steps(ENTRY[algo], model, local, glob, chains, T, 1, seed, 0.123, N, history=hist, gf_per_chain=gfg)
    torch.cuda.synchronize()
    # oracle with the same array
    hc = oracle_lib.HostChains(theta0, y0)
    hh = np.zeros((T, 2, n), np.float32)
    if algo == "glmcmc":
        assert oracle.oracle_init_weights(C.byref(model), C.byref(glob), C.byref(hc.struct())) == 0
    run, keep = oracle_lib.make_run(seed=seed, step0=1, n_steps=T, gf=0.123, batch=N, history=hh)
    run.global_frequency_per_chain = gf.ctypes.data
    fn = oracle.oracle_glmcmc_steps if algo == "glmcmc" else oracle.oracle_globalmcmc_steps
    assert fn(C.byref(model), C.byref(local), C.byref(glob), C.byref(hc.struct()), C.byref(run)) == 0
    assert np.array_equal(bits(hist.cpu().numpy()), bits(hh))
    # a constant array is the scalar
    a, _, _ = hip_run(algo, model, local, glob, theta0, y0, T, seed, 0.7, N)
    chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev)
    if algo == "glmcmc":
        engine.init_weights(model, glob, chains)
    engine.run_steps(ENTRY[algo], model, local, glob, chains, T, 1, seed, 0.0, N, history=hist,
                     gf_per_chain=torch.full((n,), 0.7, device=dev))
    torch.cuda.synchronize()
    assert np.array_equal(bits(hist.cpu().numpy()), bits(a))


def test_randomised_configurations_equal_oracle(hip, oracle):
    """Half a minute of tests/fuzz_parity.py in the script's own mix of cases -- random dimension, batch size (register, team
    and wide kernels), epsilon, frequencies, proposal kinds and parameters, observations near zero, lanes, launch splits; every
    fourth case GLMALA, every eighth the g-and-k Model, every sixteenth a random user simulator (with random user prior /
    discrepancy / kernel) compiled at run time, now and then the flow and its gradient: kernels == checker, bit for bit (the
    gradient within its tolerance).  The script itself runs for as long as asked (this round: 7223 + 20 655 + 621 configurations
    without a mismatch, profiles/r03c_fuzz_*.txt, r03b_fuzz.txt)."""
    import time
    import fuzz_parity as fz
    rng = np.random.default_rng(12345)
    t0, k, kinds = time.time(), 0, set()
    while time.time() - t0 < 30.0 or k < 40:
        fn = fz.one_case_nf_grad if k % 64 == 17 else fz.one_case_rtc if k % 16 == 6 else fz.one_case_mala if k % 4 == 3 else \
            fz.one_case_gk if k % 8 == 5 else fz.one_case_nf if k % 32 == 9 else fz.one_case
        ok, desc, _ = fn(rng, oracle, k)
        assert ok, desc
        kinds.add(fn.__name__)
        k += 1
    assert k >= 40 and {"one_case", "one_case_mala", "one_case_gk", "one_case_rtc", "one_case_nf"} <= kinds


@pytest.mark.gpu
def test_glmala_law_matches_a_large_reference_sample(hip):
    """north_star: 'posterior moments and ESJD within 1e-3' for GLMALA, whose chains cannot be compared bit for bit with the
    reference as it runs.  tests/golden/glmala_stats.npz holds time averages over 500 iterations of a large
    sample of chains of the UNMODIFIED reference GLMALA run AS IS (tests/golden/make_glmala_stats.py: BASELINE config 3,
    theta0 = 0; the fixture records how many -- about 25 CPU-minutes per thousand chains in the build container); the kernel
    runs the same experiment on 2 097 152 chains.  Every pooled statistic must agree within 4 combined standard errors; the
    combined standard error of the posterior moments (E|theta_j|, E theta_j^2) must be below north_star's 1e-3 relative, and --
    once the reference sample has reached 440 000 chains -- that of ESJD and of the move rate as well."""
    from glabcmcmc_amd import GLMALA, distribution, engine
    from glabcmcmc_amd.examples.Mixture import Mixture_set
    g = load_golden("glmala_stats")
    cfg = eval(str(g["cfg"]), {"__builtins__": {}}, {"dict": dict})
    names = eval(str(g["names"]), {"__builtins__": {}}, {})
    ref_mean, ref_se = dict(zip(names, g["mean"])), dict(zip(names, g["se"]))
    assert int(g["n_chains"]) >= 150000
    n, T = 2097152, cfg["T"]
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(99)
    theta0 = torch.zeros(n, 2)
    y0 = (0.05 ** 0.5) * torch.randn(n, 2, generator=gen)
    ip = distribution.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.tensor([0.0, 0.0]))
    mom = engine.Moments(n, 2, dev)
    st = {}
    hist = GLMALA(Mixture_set(cfg["epsilon"]), T + 1, theta0, y0, cfg["tau"], cfg["num_grad"], None, cfg["gf"], ip, cfg["N"],
                  seed=2026, stats=mom, return_device=True, verbose=False, state_out=st)          # (T+1, n, 2) on the device
    x = hist[1:].double()
    jj = (mom.sum_jump / T)                                                                      # [3][n]
    det = (jj[0] * jj[2] - jj[1] ** 2).clamp_min(0.0)
    got = {
        "mean_abs_0": x[:, :, 0].abs().mean(0), "mean_abs_1": x[:, :, 1].abs().mean(0),
        "mean_sq_0": (x[:, :, 0] ** 2).mean(0), "mean_sq_1": (x[:, :, 1] ** 2).mean(0),
        "jump_00": jj[0], "jump_01": jj[1], "jump_11": jj[2], "esjd": det.sqrt(),
        "move_rate": st["chains"].n_moves.double() / T,
        "final_abs_0": x[-1, :, 0].abs(), "final_abs_1": x[-1, :, 1].abs(),
        "final_sq_0": x[-1, :, 0] ** 2, "final_sq_1": x[-1, :, 1] ** 2,
    }
    report = {}
    for k in names:
        v = got[k].cpu().numpy()
        m, se = v.mean(), v.std(ddof=1) / np.sqrt(n)
        comb = float(np.hypot(se, ref_se[k]))
        report[k] = (m, ref_mean[k], comb)
        assert abs(m - ref_mean[k]) <= 4.0 * comb, (k, m, ref_mean[k], comb)
    for k in ("mean_abs_0", "mean_abs_1", "mean_sq_0", "mean_sq_1"):
        m, r, comb = report[k]
        assert comb / abs(r) < 1e-3 and abs(m - r) / abs(r) < 2.5e-3, (k, report[k])
    tight = int(g["n_chains"]) >= 440000
    print("GLMALA law, %d kernel chains against %d unmodified reference chains (statistic: kernel, reference, relative difference, "
          "combined relative standard error)" % (n, int(g["n_chains"])))
    for k in names:
        m, r, comb = report[k]
        print("  %-12s %.6f %.6f %+.2e %.2e" % (k, m, r, (m - r) / abs(r) if r else 0.0, comb / abs(r) if r else 0.0))
    for k in ("esjd", "move_rate"):
        m, r, comb = report[k]
        assert comb / abs(r) < (1e-3 if tight else 2e-3), (k, report[k], int(g["n_chains"]))
        if tight:
            assert abs(m - r) / abs(r) < 3.5e-3, (k, report[k])


# ---------------------------------------------------------------------------------- wide batches (glabc_wide.hip)
WIDE_CASES = [
    # d, N, lanes (0 = library's choice), gf, eps, global spec, chains, T, debug_flags
    (2, 17, 0, 0.9, 0.3, ("gauss", [0, 0], [1, 1]), 777, 60, 0),
    (2, 32, 8, 0.8, 0.05, ("gauss", [0, 0], [1, 1]), 1000, 80, 0),
    (2, 32, 16, 0.8, 0.05, ("gauss", [0, 0], [1, 1]), 1000, 80, 0),
    (2, 32, 32, 0.8, 0.05, ("gauss", [0, 0], [1, 1]), 333, 50, 0),
    (2, 32, 64, 0.8, 0.05, ("gauss", [0, 0], [1, 1]), 130, 50, 0),
    (2, 64, 0, 0.5, 0.3, ("uniform", [-3, -3], [3, 3]), 500, 60, 0),
    (2, 100, 0, 0.7, 0.1, ("gauss", [0.3, -0.2], [1.4, 1.1]), 300, 50, 0),
    (2, 256, 0, 0.9, 0.3, ("gauss", [0, 0], [1, 1]), 200, 30, 0),
    (2, 256, 64, 0.9, 0.3, ("gauss", [0, 0], [1, 1]), 100, 30, 1),          # GLABC_DEBUG_EXACT_INDEX: the reference's loop always
    (2, 1000, 0, 0.9, 0.3, ("gauss", [0, 0], [1, 1]), 64, 20, 0),           # torch.sum's cascade levels (n >= 512)
    (1, 40, 0, 0.6, 0.3, ("uniform", [-3], [3]), 400, 60, 0),
    (3, 33, 0, 0.6, 0.4, ("gauss", [0, 0, 0], [1.2, 1.2, 1.2]), 300, 50, 0),
    (4, 20, 0, 0.6, 0.5, ("gauss", [0] * 4, [1.2] * 4), 300, 50, 0),
]


@pytest.mark.parametrize("case", WIDE_CASES, ids=lambda c: "d%d-N%d-L%d-%s%s" % (c[0], c[1], c[2], c[5][0], "-exact" if c[8] else ""))
def test_wide_batches_equal_oracle(hip, oracle, case):
    """batch_size > 16: lane groups of a wavefront share a chain's proposals (ATen-order total over 32 accumulator lanes,
    chunked double prefix sums for the index).  Histories, final state, flags, log-weights, move counts and the streamed
    sums equal the CPU checker's bit for bit, for every group width."""
    from test_stream_independence import abs_gauss_model
    d, N, lanes, gf, eps, gspec, n, T, dbg = case
    model = abs_gauss_model(d, eps)
    local = make_dist(("gauss", [0.0] * d, [0.35] * d)).descriptor()
    glob = make_dist(gspec).descriptor()
    rng = np.random.default_rng(N * 7 + d)
    theta0 = rng.standard_normal((n, d)).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((n, d))).astype(np.float32)
    seed, chain0 = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40))
    hist, chains, mom = hip_run("glmcmc", model, local, glob, theta0, y0, T, seed, gf, N, chain0=chain0, moments=True,
                                lanes=lanes, debug_flags=dbg, steps_per_launch=23)
    hh, hc, hm = oracle_run(oracle, "glmcmc", model, local, glob, theta0, y0, T, seed, gf, N, chain0=chain0, moments=True)
    same = bits(hist) == bits(hh)
    assert same.all(), "first mismatch at (t, dim, chain) = %s" % (np.argwhere(~same)[0],)
    assert_same_state(chains, hc, True)
    assert hc.n_moves.sum() > n
    assert np.array_equal(mom.sum_theta.cpu().numpy(), hm.sum_theta)
    assert np.array_equal(mom.sum_outer.cpu().numpy(), hm.sum_outer)
    assert np.array_equal(mom.sum_jump.cpu().numpy(), hm.sum_jump)


def test_wide_batch_gk_model_equals_oracle(hip, oracle):
    from glabcmcmc_amd.examples.GK import GK_set
    cfg = dict(model="gk", epsilon=1.0, local=("gauss", [0.0] * 4, [0.15] * 4), **{"global": ("uniform", [0.0] * 4, [10.0] * 4)})
    model, local, glob = descriptors(cfg)
    rng = np.random.default_rng(5)
    n, T, N = 300, 40, 48
    theta0 = rng.uniform(0.5, 5.0, (n, 4)).astype(np.float32)
    torch.manual_seed(3)
    y0 = GK_set(1.0).generate_samples(torch.from_numpy(theta0)).numpy().copy()
    hist, chains, _ = hip_run("glmcmc", model, local, glob, theta0, y0, T, 77, 0.8, N, chain0=5)
    hh, hc, _ = oracle_run(oracle, "glmcmc", model, local, glob, theta0, y0, T, 77, 0.8, N, chain0=5)
    assert np.array_equal(bits(hist), bits(hh))
    assert_same_state(chains, hc, True)
    assert hc.n_moves.sum() > n


def test_wide_batch_through_the_python_api_equals_the_generic_path(hip):
    """GLMCMC(..., batch_size=40): the fused wide kernel and the split-phase path (propose / Mixture_set's row-wise
    kernels / select) are two implementations of the same specification -- identical chains."""
    from glabcmcmc_amd import GLMCMC, distribution
    from glabcmcmc_amd.examples.Mixture import Mixture_set
    m = Mixture_set(0.2)
    lp = distribution.DiagGaussian(2, torch.zeros(1, 2), torch.log(torch.tensor([0.35, 0.35])))
    ip = distribution.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.tensor([0.0, 0.0]))
    g = torch.Generator().manual_seed(5)
    th0 = torch.randn(512, 2, generator=g)
    y0 = th0.abs() + 0.2236 * torch.randn(512, 2, generator=g)
    a = GLMCMC(m, 60, th0, y0, lp, None, 0.8, ip, 40, seed=3, verbose=False, path="fused")
    b = GLMCMC(m, 60, th0, y0, lp, None, 0.8, ip, 40, seed=3, verbose=False, path="generic")
    assert np.array_equal(bits(a.numpy()), bits(b.numpy()))
    assert (a[1:] != a[:-1]).any()


def test_gamma_forward_on_gpu(hip, oracle):
    """glabc_gamma_forward == the CPU checker bit for bit (variates and log_p); through Gamma(..., device='cuda').forward"""
    from glabcmcmc_amd import distribution
    prim = load_golden("primitives")
    for tag in ("a", "b", "c"):
        g = distribution.Gamma(torch.from_numpy(prim["gf_%s_shape" % tag]), torch.from_numpy(prim["gf_%s_rate" % tag]),
                               device="cuda")
        seed, row0 = (int(v) for v in prim["gf_%s_seed_row0" % tag])
        n = 100000
        z, lp = g.forward(n, seed=seed, row0=row0)
        d = g.gamma_descriptor()
        zo, lo = np.empty((n, d.dim)), np.empty(n)
        assert oracle.oracle_gamma_forward(C.byref(d), n, seed, row0, zo.ctypes.data, lo.ctypes.data) == 0
        assert z.dtype == torch.float64 and np.array_equal(z.cpu().numpy().reshape(n, -1).view(np.uint64), zo.view(np.uint64)), tag
        assert np.array_equal(lp.cpu().numpy().view(np.uint64), lo.view(np.uint64)), tag
        assert np.array_equal(zo[:400].view(np.uint64), prim["gf_%s_z" % tag].view(np.uint64))
        mean = zo.mean(0)
        want = prim["gf_%s_shape" % tag].astype(np.float64) / prim["gf_%s_rate" % tag]
        assert np.all(np.abs(mean - want) < 0.02 * want + 0.01)


def test_gamma_importance_proposal_runs_glmcmc(hip):
    """Gamma as the importance proposal of GLMCMC (a9): no glabc_dist descriptor, so the split-phase path draws the
    candidates with glabc_gamma_forward and evaluates log_prob with glabc_gamma_log_prob; the chains reach the posterior of
    the |theta| model restricted to theta > 0 (the proposal's support): E theta_j^2 as for the symmetric model."""
    from glabcmcmc_amd import GLMCMC, distribution, engine
    from glabcmcmc_amd.examples.UserModel import TorchMixture
    from test_stream_independence import analytic
    n, eps, T = 8192, 0.3, 300
    m = TorchMixture(2, eps)
    lp = distribution.DiagGaussian(2, torch.zeros(2), torch.log(torch.tensor([0.3, 0.3])))
    ip = distribution.Gamma(torch.tensor([4.0, 4.0]), torch.tensor([3.0, 3.0]), device="cuda", seed=5)      # mean 1.33
    th0 = torch.full((n, 2), 1.3)
    y0 = th0.abs() + 0.2236 * torch.randn(n, 2)
    st = {}
    GLMCMC(m, 150, th0, y0, lp, None, 0.7, ip, 6, seed=1, record_history=False, verbose=False, state_out=st)
    ch = st["chains"]
    mom = engine.Moments(n, 2, torch.device("cuda", 0))
    GLMCMC(m, T + 1, ch.theta.t().cpu(), ch.y.t().cpu(), lp, None, 0.7, ip, 6, seed=2, record_history=False, stats=mom,
           verbose=False)
    _, want_sq = analytic(eps)
    per_chain = mom.sum_outer[0].cpu().numpy() / T
    se = per_chain.std(ddof=1) / np.sqrt(n)
    assert abs(per_chain.mean() - want_sq) < 5 * se + 3e-3 * want_sq, (per_chain.mean(), want_sq, se)
    assert (ch.theta > 0).float().mean() > 0.95          # iSIR moves land on the Gamma's support; local moves rarely cross 0


# ---------------------------------------------------------------------------------- Gamma inside the samplers (a9)
def _gamma_desc(shape, rate):
    from glabcmcmc_amd import distribution
    return distribution.Gamma(torch.tensor(shape, dtype=torch.float32), torch.tensor(rate, dtype=torch.float32)).descriptor()


GAMMA_CASES = [
    # algo, d, N, gf, importance / global, prior, chains, T
    ("glmcmc", 2, 5, 0.8, ("gamma", [4.0, 4.0], [3.0, 3.0]), None, 700, 150),
    ("glmcmc", 2, 5, 0.8, ("gauss", [0.8, 0.8], [1.0, 1.0]), ("gamma", [2.0, 3.0], [1.5, 2.0]), 513, 150),
    ("glmcmc", 2, 3, 0.6, ("gamma", [0.5, 2.5], [1.0, 1.5]), ("gamma", [2.0, 2.0], [1.0, 1.0]), 300, 120),       # shape < 1: the boost draw
    ("glmcmc", 1, 16, 0.9, ("gamma", [3.0], [2.0]), None, 200, 80),
    ("glmcmc", 4, 4, 0.7, ("gamma", [4.0, 4.0, 4.0, 4.0], [3.0, 3.0, 3.0, 3.0]), ("gamma", [2.0] * 4, [1.0] * 4), 130, 80),
    ("glmcmc", 2, 40, 0.8, ("gamma", [4.0, 4.0], [3.0, 3.0]), ("gamma", [2.0, 3.0], [1.5, 2.0]), 200, 60),         # wide kernel
    ("glmcmc", 3, 100, 1.0, ("gamma", [4.0, 2.0, 1.0], [3.0, 1.0, 1.0]), None, 70, 40),                            # wide, 16 lanes
    ("globalmcmc", 2, 1, 0.5, ("gamma", [4.0, 4.0], [3.0, 3.0]), ("gamma", [2.0, 3.0], [1.5, 2.0]), 640, 200),
]


@pytest.mark.parametrize("case", GAMMA_CASES, ids=lambda c: "%s-d%d-N%d-%s-%s" % (c[0], c[1], c[2], c[4][0], c[5][0] if c[5] else "gaussprior"))
def test_gamma_inside_the_fused_kernels(hip, oracle, case):
    """GLABC_DIST_GAMMA as importance / global proposal and as prior in sampler_kernel (VAR_GAMMA), wide_kernel and
    init_weights (include/glabc.h; distribution.py:90-137): histories, states, weights, counters and sums equal the CPU
    checker's bit for bit; the chains live on the Gamma's support."""
    from glabcmcmc_amd import _capi as A
    from glabcmcmc_amd import distribution
    algo, d, N, gf, gspec, pspec, n, T = case
    model, local, glob = descriptors(dict(epsilon=0.3, local=("gauss", [0] * 2, [0.3] * 2), **{"global": ("gauss", [0] * 2, [1] * 2)}))
    noise = distribution.DiagGaussian(d, torch.zeros(d), torch.log(torch.full((d,), 0.05).sqrt())).descriptor()
    model.theta_dim = model.y_dim = d
    model.noise = noise
    for j in range(d):
        model.y_obs[j] = 1.5 - 0.25 * j
    model.prior = _gamma_desc(*pspec[1:]) if pspec else distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d)).descriptor()
    local = make_dist(("gauss", [0.0] * d, [0.3] * d)).descriptor()
    glob = _gamma_desc(*gspec[1:]) if gspec[0] == "gamma" else make_dist((gspec[0], gspec[1][:d], gspec[2][:d])).descriptor()
    rng = np.random.default_rng(17 * N + d)
    theta0 = (np.abs(rng.standard_normal((n, d))) + 0.2).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((n, d))).astype(np.float32)
    seed, chain0 = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40))
    hist, chains, mom = hip_run(algo, model, local, glob, theta0, y0, T, seed, gf, N, chain0=chain0, moments=True,
                                steps_per_launch=33)
    hh, hc, hm = oracle_run(oracle, algo, model, local, glob, theta0, y0, T, seed, gf, N, chain0=chain0, moments=True)
    same = bits(hist) == bits(hh)
    assert same.all(), "first mismatch at (t, dim, chain) = %s" % (np.argwhere(~same)[0],)
    assert_same_state(chains, hc, algo == "glmcmc")
    assert np.array_equal(mom.sum_jump.cpu().numpy(), hm.sum_jump)
    assert hc.n_moves.sum() > n // 4
    if pspec:
        assert (hist[T // 2:] >= 0).all()                   # a Gamma prior: no state outside its support survives
    if algo == "glmcmc" and 2 <= N <= 16:
        # ... and in the team geometry (csrc/glabc_team.h: two / three wavefronts per 64 chains, what a launch of 16 384 .. 131 072
        # chains gets): the helpers draw their Gamma candidates from the same slots -- the same bits again
        for waves in ("2", "3"):
            os.environ["GLABC_TEAM_WAVES"] = waves
            try:
                h2, c2, m2 = hip_run(algo, model, local, glob, theta0, y0, T, seed, gf, N, chain0=chain0, moments=True,
                                     steps_per_launch=33, debug_flags=A.DEBUG_TEAM)
            finally:
                del os.environ["GLABC_TEAM_WAVES"]
            assert (bits(h2) == bits(hh)).all(), waves
            assert_same_state(c2, hc, True)
            assert np.array_equal(m2.sum_jump.cpu().numpy(), hm.sum_jump)


def test_gamma_split_phase_equals_fused(hip):
    """The same iteration cut at the Model's callbacks: glabc_propose draws the Gamma candidates from the same slots, the
    Model's prior_log_prob is the Gamma prior through the row-wise kernel, glabc_select decides -- the chains equal the fused
    kernel's bit for bit (GLMCMC and GlobalMCMC), through the package's own functions."""
    import glabcmcmc_amd as g_
    from glabcmcmc_amd import distribution, engine
    from glabcmcmc_amd.examples.Mixture import Mixture_set
    prior = distribution.Gamma(torch.tensor([2.0, 3.0]), torch.tensor([1.5, 2.0]))
    m = Mixture_set(0.3, prior=prior)
    lp = distribution.DiagGaussian(2, torch.zeros(1, 2), torch.log(torch.tensor([0.3, 0.3])))
    ip = distribution.Gamma(torch.tensor([4.0, 4.0]), torch.tensor([3.0, 3.0]))
    n, T = 1500, 60
    gen = torch.Generator().manual_seed(3)
    th0 = torch.randn(n, 2, generator=gen).abs() + 0.2
    y0 = th0 + 0.2236 * torch.randn(n, 2, generator=gen)
    dev = torch.device("cuda", 0)
    for fn, args in ((g_.GLMCMC, (lp, None, 0.8, ip, 5)), (g_.GlobalMCMC, (ip, None, 0.5, lp))):
        outs = []
        for path in ("fused", "generic"):
            mom = engine.Moments(n, 2, dev)
            h = fn(m, T + 1, th0, y0, *args, seed=11, stats=mom, return_device=True, verbose=False, path=path)
            outs.append((h.cpu().numpy(), mom.sum_jump.cpu().numpy()))
        assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])), fn.__name__
        assert np.array_equal(outs[0][1].view(np.uint64), outs[1][1].view(np.uint64))
        assert (np.diff(outs[0][0], axis=0) != 0).any(-1).mean() > 0.02
    # `auto` picks the fused kernels for this configuration, and refuses nothing
    from glabcmcmc_amd import generic
    assert generic.fused_supported(m, (lp, ip), 5, gamma_ok=True) and not generic.fused_supported(m, (lp, ip), 5)
    assert not generic.fused_supported(m, (ip, ip), 5, gamma_ok=True)          # a Gamma local increment is a callback


def test_gamma_descriptor_entry_points(hip, oracle):
    """glabc_dist_log_prob / the row-wise prior with a Gamma descriptor == the CPU checker bit for bit (the reference-pinned
    values: tests/test_oracle_golden.py); what the ABI refuses: a Gamma local increment, Gamma in GLMALA and the pool kernels"""
    from glabcmcmc_amd import _capi as A
    from glabcmcmc_amd import engine
    g = load_golden("gamma_candidates")
    dev = torch.device("cuda", 0)
    for i in range(5):
        d = _gamma_desc(g["gc_%d_shape" % i].tolist(), g["gc_%d_rate" % i].tolist())
        pts = g["gc_%d_pts" % i]
        want = np.empty(len(pts), np.float32)
        assert oracle.oracle_dist_log_prob(C.byref(d), pts.ctypes.data, len(pts), want.ctypes.data) == 0
        z = torch.from_numpy(pts).to(dev)
        out = torch.empty(len(pts), dtype=torch.float32, device=dev)
        assert hip.glabc_dist_log_prob(C.byref(d), z.data_ptr(), len(pts), out.data_ptr(), None) == 0
        assert np.array_equal(bits(out.cpu().numpy()), bits(want)), i
    model, local, glob = descriptors(dict(epsilon=0.3, local=("gauss", [0, 0], [0.3, 0.3]), **{"global": ("gauss", [0, 0], [1, 1])}))
    gam = _gamma_desc([2.0, 2.0], [1.0, 1.0])
    chains = engine.ChainBatch(torch.ones(8, 2), torch.ones(8, 2), dev).add_mala_state()
    cs = chains.struct()
    run = A.Run()
    run.seed, run.step0, run.n_steps, run.global_frequency, run.batch_size = 1, 1, 2, 0.5, 5
    assert hip.glabc_glmcmc_steps(C.byref(model), C.byref(gam), C.byref(glob), C.byref(cs), C.byref(run), None) == -3      # local
    assert hip.glabc_glmcmc_steps(C.byref(model), C.byref(local), C.byref(gam), C.byref(cs), C.byref(run), None) == 0
    mala = A.Mala(0.3, 0.09, 0.09, 10, 0)
    assert hip.glabc_glmala_steps(C.byref(model), C.byref(gam), C.byref(mala), C.byref(cs), C.byref(run), None) == -3
    bad = _gamma_desc([2.0, 2.0], [1.0, 1.0])
    bad.p0[1] = -1.0
    assert hip.glabc_glmcmc_steps(C.byref(model), C.byref(local), C.byref(bad), C.byref(cs), C.byref(run), None) == -4
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------- the drop-in return path
@pytest.mark.parametrize("sampler", ["glmcmc", "globalmcmc", "glmala"])
def test_large_histories_reach_the_host_while_the_kernels_run(hip, sampler, monkeypatch, tmp_path):
    """The reference returns Theta_Re as a CPU tensor (GLMCMC.py:137).  A history of 16 MiB and more of many chains is copied to
    pinned host memory launch by launch on a second stream WHILE the next launch computes (_host.HostMirror) instead of after the
    run: same rows, bit for bit, as the device-resident history of the same seed -- also when the run is cut into many short
    launches -- and the CSV file written from it equals the one written from the device copy."""
    import glabcmcmc_amd as g_
    from glabcmcmc_amd import _host, distribution
    from glabcmcmc_amd.examples.Mixture import Mixture_set
    n, T = 4096, 520                                                    # 521 x 2 x 4096 floats = 16.3 MiB
    gen = torch.Generator().manual_seed(3)
    theta0 = torch.randn(n, 2, generator=gen)
    y0 = theta0.abs() + (0.05 ** 0.5) * torch.randn(n, 2, generator=gen)
    lp = distribution.DiagGaussian(2, torch.zeros(2), torch.log(torch.tensor([0.35, 0.35])))
    ip = distribution.DiagGaussian(2, torch.zeros(2), torch.zeros(2))
    model = Mixture_set(0.05)

    def run(**kw):
        if sampler == "glmcmc":
            return g_.GLMCMC(model, T + 1, theta0, y0, lp, kw.pop("file", None), 0.9, ip, 5, seed=11, verbose=False, **kw)
        if sampler == "globalmcmc":
            return g_.GlobalMCMC(model, T + 1, theta0, y0, ip, kw.pop("file", None), 0.5, lp, seed=11, verbose=False, **kw)
        return g_.GLMALA(model, T + 1, theta0, y0, 0.3, 20, kw.pop("file", None), 0.8, ip, 5, seed=11, verbose=False, **kw)

    made = []
    real = _host.HostMirror.__init__

    def spy(self, hist):
        made.append(self)
        real(self, hist)

    monkeypatch.setattr(_host.HostMirror, "__init__", spy)
    want = run(return_device=True)                                      # (T+1, n, 2) view of the device history
    assert not made and want.is_cuda
    got = run()
    assert len(made) == 1 and not got.is_cuda and got.shape == want.shape
    assert np.array_equal(bits(got.numpy()), bits(want.cpu().numpy()))
    monkeypatch.setattr(_host.HostMirror, "LAUNCH_BYTES", 1 << 20)      # 32 rows per launch: 17 launches, 17 copies behind them
    f1, f2 = str(tmp_path / "a.csv"), str(tmp_path / "b.csv")
    got2 = run(file=f1)
    assert len(made) == 2 and np.array_equal(bits(got2.numpy()), bits(want.cpu().numpy()))
    if sampler == "glmcmc":
        run(file=f2, return_device=True)
        assert open(f1, "rb").read() == open(f2, "rb").read()


# ---------------------------------------------------------------------------------- BASELINE configs[0], literally
def test_config_1_runner_global_mcmc_one_chain_10000_iterations(hip, oracle, tmp_path, capsys):
    """BASELINE.json configs[0]: Mixture_set eps 0.05, dim 2, ONE chain x 10 000 iterations through MCMCRunner.run_global_mcmc
    with the CSV side effect, on the GPU.  The returned Theta_Re is the reference's shape and dtype ((num_ite, 2) float32 on
    the CPU, row 0 = theta_0), equals the CPU checker's chain bit for bit, and the file is what the reference's dump schedule
    (GlobalMCMC.py:70-76: header = theta_0, a block at i % 10000 == 0 and at the last iteration -- here no duplicated tail,
    num_ite - 1 = 9 999) writes for that chain: csv.writer rows of numpy float32 values."""
    import csv as csvmod
    import glabcmcmc_amd as g_
    from glabcmcmc_amd import _host
    from glabcmcmc_amd.examples.Mixture import Mixture_set
    num_ite, seed, gf = 10_000, 20261004, 0.5
    m = Mixture_set(0.05)
    lp = g_.DiagGaussian(2, loc=torch.zeros(1, 2), log_scale=torch.log(torch.tensor([0.35, 0.35])))
    gp = g_.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.tensor([0.0, 0.0]))
    theta0 = torch.tensor([0.0, 0.0])
    y0 = torch.tensor([[0.21, -0.13]])
    runner = g_.MCMCRunner(m, output_dir=str(tmp_path / "out"))
    out = runner.run_global_mcmc(num_ite, theta0, y0, gf, lp, gp, output_file="global_mcmc_results.csv", seed=seed)
    assert out.shape == (num_ite, 2) and out.dtype == torch.float32 and out.device.type == "cpu"
    assert torch.equal(out[0], theta0)
    assert capsys.readouterr().out.strip() != ""                              # the end-of-run summary print (GlobalMCMC.py:92-96)
    # the checker's chain
    model, local, glob = m.descriptor(), lp.descriptor(), gp.descriptor()
    hh, hc, _ = oracle_run(oracle, "globalmcmc", model, local, glob, theta0.view(1, 2).numpy(), y0.numpy(), num_ite - 1, seed, gf, 1)
    want = np.concatenate([theta0.view(1, 2).numpy(), hh[:, :, 0]], axis=0)
    assert np.array_equal(bits(out.numpy()), bits(want))
    moves = int((np.diff(want, axis=0) != 0).any(1).sum())
    assert 30 < moves < 2000, moves                                           # eps 0.05: about one move in a hundred iterations
    # the CSV: the file the run wrote == the reference schedule applied to the chain
    path = tmp_path / "out" / "global_mcmc_results.csv"
    rows = list(csvmod.reader(open(path)))
    assert len(rows) == num_ite                                               # header (theta_0) + rows 1 .. 9999, no duplicated block
    got = np.array(rows, dtype=np.float32)
    assert np.array_equal(bits(got), bits(want))
    ref_file = tmp_path / "ref.csv"
    _host.write_csv(torch.from_numpy(want), str(ref_file), "global")
    assert open(path, "rb").read() == open(ref_file, "rb").read()


# ---------------------------------------------------------------------------------- GLABC_MATH_FAST (opt-in), teacher-forced parity
TAPE_GUARD = 256                # canary elements in front of and behind every tape buffer


def _fast_run(model, local, glob, theta0, y0, T, seed, gf, N, chain0=0, dump=True, moments=False, step0=1, chains=None):
    """One GLABC_MATH_FAST launch of T iterations from iteration step0 -> (history, chains, moments, tape).  chains: the
    ChainBatch an earlier launch left (None: a fresh one from theta0 / y0 after init_weights); moments: True, or the
    engine.Moments an earlier launch filled.  The tape buffers start as NaN and lie inside larger canary buffers: the guards
    must come back untouched (checked here), and whatever the kernel does not write stays NaN for the caller to find."""
    from glabcmcmc_amd import _capi as A
    from glabcmcmc_amd import engine
    import helpers as H
    dev = torch.device("cuda", 0)
    if chains is None:
        chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev, chain0=chain0)
        engine.init_weights(model, glob, chains)
    n, d, yd = chains.n, chains.d, chains.yd
    hist = torch.empty(T, d, n, dtype=torch.float32, device=dev)
    tape, whole = None, []
    if dump:
        def guarded(canary, *shape):
            size = int(np.prod(shape))
            flat = H.dev(canary(size + 2 * TAPE_GUARD))
            body = flat[TAPE_GUARD:TAPE_GUARD + size].view(*shape)
            body.fill_(float("nan"))
            whole.append((flat, size))
            return body
        tape = (guarded(H.canary_f32, n, T, 2), guarded(H.canary_f64, n, T), guarded(H.canary_f32, n, T, N, d + yd))
    mom = engine.Moments(n, d, dev) if moments is True else (moments or None)
    engine.run_steps("glabc_glmcmc_steps", model, local, glob, chains, T, step0, seed, gf, N, history=hist, moments=mom,
                     math_mode=A.MATH_FAST, dump_draws=tape)
    torch.cuda.synchronize()
    for flat, size in whole:
        edge = flat.cpu().numpy()
        H.assert_untouched(edge[:TAPE_GUARD], edge[TAPE_GUARD + size:])
    return hist.cpu().numpy(), chains, mom, None if tape is None else tuple(t.cpu().numpy() for t in tape)


def fast_replay(oracle, model, local, glob, theta0, y0, gf, N, tapes, idx=None, chain0=0, seed=0, moments=False):
    """The CPU checker, in exact arithmetic, on the draws a fast kernel recorded.  tapes: one (u, r, z) per launch, in order;
    launch k starts at iteration 1 + (the lengths before it) from the state the replay of launch k - 1 left, the first from
    (theta0, y0) after oracle_init_weights.  idx: the chains to replay (None: all).  -> (history (T, d, len(idx)), HostChains,
    HostMoments or None)"""
    idx = np.arange(theta0.shape[0]) if idx is None else np.asarray(idx)
    d = theta0.shape[1]
    hc = oracle_lib.HostChains(theta0[idx], y0[idx], chain0=chain0)
    mom = oracle_lib.HostMoments(len(idx), d) if moments else None
    cs = hc.struct()
    assert oracle.oracle_init_weights(C.byref(model), C.byref(glob), C.byref(cs)) == 0
    rows, step0 = [], 1
    for u, r, z in tapes:
        T = u.shape[1]
        hh = np.zeros((T, d, len(idx)), np.float32)
        run, keep = oracle_lib.make_run(seed=seed, step0=step0, n_steps=T, gf=gf, batch=N, history=hh, moments=mom,
                                        tape=(np.ascontiguousarray(u[idx]), np.ascontiguousarray(r[idx]),
                                              np.ascontiguousarray(z[idx]), N))
        assert oracle.oracle_glmcmc_steps(C.byref(model), C.byref(local), C.byref(glob), C.byref(cs), C.byref(run)) == 0
        rows.append(hh)
        step0 += T
    return np.concatenate(rows, axis=0), hc, mom


def fast_flips(oracle, model, local, glob, theta0, y0, gf, N, tapes, hist, hh, **kw):
    """Chains whose kernel history `hist` leaves the checker's replay `hh` of the kernel's own draws (fast_replay of `tapes`), and
    which of them the perturbation replay does NOT explain: a chain is explained when replaying it with the resampling uniform
    of its first differing iteration moved by +-1e-5, or that iteration's accept uniform scaled by exp(+-2e-3), gives the
    kernel's state of that iteration.  -> (flipped chain indices, [(chain, first differing iteration)] unexplained)"""
    flipped = np.flatnonzero((bits(hist) != bits(hh)).any(axis=(0, 1)))
    starts = np.cumsum([0] + [t[0].shape[1] for t in tapes])
    unexplained = []
    for c in flipped:
        t0 = int(np.flatnonzero((bits(hist[:, :, c]) != bits(hh[:, :, c])).any(axis=1))[0])
        k = int(np.searchsorted(starts, t0, side="right")) - 1              # the launch of iteration t0 and its row there
        tl = t0 - int(starts[k])
        ok = False
        for dr, fu in ((1e-5, 1.0), (-1e-5, 1.0), (0.0, float(np.exp(2e-3))), (0.0, float(np.exp(-2e-3)))):
            mine = [tuple(a[c:c + 1].copy() for a in t) for t in tapes]
            u2, r2, _ = mine[k]
            r2[0, tl] = min(max(r2[0, tl] + dr, 0.0), 1.0 - 2 ** -53)
            u2[0, tl, 1] = np.float32(min(u2[0, tl, 1] * fu, 1.0 - 2 ** -24))
            h2, _, _ = fast_replay(oracle, model, local, glob, theta0[c:c + 1], y0[c:c + 1], gf, N, mine, **kw)
            ok = ok or np.array_equal(bits(h2[t0, :, 0]), bits(hist[t0, :, c]))
        if not ok:
            unexplained.append((int(c), t0))
    return flipped, unexplained


def assert_same_fast_state(chains, hc, keep):
    """theta, y, n_moves and flags of the chains `keep` equal the replay's bit for bit (assert_same_state on that subset; log_w is
    a function of the fast kernel's own K(y) and is compared within a bound by the callers that look at it)"""
    from types import SimpleNamespace
    k = torch.from_numpy(np.asarray(keep))
    got = SimpleNamespace(theta=chains.theta.cpu()[:, k], y=chains.y.cpu()[:, k], n_moves=chains.n_moves.cpu()[k])
    want = SimpleNamespace(theta=hc.theta[:, keep], y=hc.y[:, keep], n_moves=hc.n_moves[keep])
    assert_same_state(got, want, False)
    assert np.array_equal(chains.flags.cpu().numpy().astype(np.uint32)[keep], hc.flags[keep])


FAST_CASES = [
    # d, N, gf, eps, local, global
    (2, 5, 0.9, 0.05, ("gauss", [0, 0], [0.35, 0.35]), ("gauss", [0, 0], [1, 1])),                # the bench configuration
    (2, 8, 0.6, 0.3, ("gauss", [0, 0], [0.35, 0.35]), ("gauss", [0.1, -0.1], [1.0, 1.25])),       # VAR_GENERIC
    (3, 4, 0.7, 0.3, ("uniform", [-0.4] * 3, [0.4] * 3), ("uniform", [-3] * 3, [3] * 3)),
    (1, 16, 0.8, 0.2, ("gauss", [0], [0.4]), ("gauss", [0], [1])),
]


@pytest.mark.parametrize("case", FAST_CASES, ids=lambda c: "d%d-N%d-%s" % (c[0], c[1], c[5][0]))
def test_fast_math_decisions_follow_the_checker_on_the_kernels_own_draws(hip, oracle, case):
    """glabc_run.math_mode = GLABC_MATH_FAST (opt-in, include/glabc.h), parity the teacher-forced way: the
    kernel records every uniform and normal it drew; the CPU checker replays that tape through the EXACT arithmetic.  Candidates
    are IEEE functions of the draws, so a chain's states are bit-identical as long as the decisions agree; a chain may leave the
    checker's path only at a decision that lies within rounding of its threshold -- shown by replaying that chain with the
    step's resampling uniform moved by 1e-5 or its accept uniform scaled by exp(+-2e-3) and finding the kernel's state.  Such
    chains must be rare."""
    from glabcmcmc_amd import _capi as A
    from glabcmcmc_amd import distribution
    d, N, gf, eps, lspec, gspec = case
    if d == 2:
        model, local, glob = descriptors(dict(epsilon=eps, local=lspec, **{"global": gspec}))
    else:
        prior = distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d)).descriptor()
        noise = distribution.DiagGaussian(d, torch.zeros(d), torch.log(torch.full((d,), 0.05).sqrt())).descriptor()
        kern = distribution.DiagGaussian(1, torch.tensor([0.0]), torch.log(torch.tensor([eps]))).descriptor()
        model = A.Model()
        model.sim_kind, model.theta_dim, model.y_dim = A.SIM_ABS_GAUSS, d, d
        model.prior, model.noise = prior, noise
        for j in range(d):
            model.y_obs[j] = 1.5 - 0.25 * j
        model.kern_log_scale, model.kern_scale, model.kern_c0, model.epsilon = kern.p1[0], kern.p2[0], kern.c0, eps
        local, glob = make_dist(lspec).descriptor(), make_dist(gspec).descriptor()
    n, T, seed = 4096, 40, 20261004
    rng = np.random.default_rng(7 * N + d)
    theta0 = rng.standard_normal((n, d)).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((n, d))).astype(np.float32)
    hist, chains, _, (tu, tr, tz) = _fast_run(model, local, glob, theta0, y0, T, seed, gf, N, chain0=77)
    assert np.isfinite(tu).all() and np.isfinite(tr).all()                       # the tape starts as NaN: every slot was written
    assert np.isfinite(tz).all() and abs(tz.mean()) < 0.05 if gspec[0] == "gauss" else True
    assert np.isfinite(tz).all()

    hh, hc, _ = fast_replay(oracle, model, local, glob, theta0, y0, gf, N, [(tu, tr, tz)], chain0=77, seed=seed)
    moved = (np.diff(hist, axis=0) != 0).any(axis=1).sum()
    assert moved > n                                                             # the run does something
    flipped, unexplained = fast_flips(oracle, model, local, glob, theta0, y0, gf, N, [(tu, tr, tz)], hist, hh,
                                      chain0=77, seed=seed)
    assert len(flipped) <= max(4, n // 200), "%d of %d chains leave the checker's path" % (len(flipped), n)
    assert not unexplained, "decisions that differ beyond rounding of their threshold: %s" % unexplained[:5]
    assert_same_fast_state(chains, hc, np.setdiff1d(np.arange(n), flipped))      # what the kernel leaves behind, where it followed
    print("fast math d=%d N=%d: %d of %d chains take a within-rounding decision the other way in %d iterations"
          % (d, N, len(flipped), n, T))


def test_fast_math_team_of_two_follows_the_checker(hip, oracle, monkeypatch):
    """launches of the cases above are small, so they run as teams of three wavefronts (tests/test_launch_plan.py
    test_fast_math); GLABC_TEAM_WAVES = 2 takes the same case through the other fast instantiation, team_sampler_kernel<..., NW = 2,
    FAST>, which a default launch reaches only above 65 536 chains"""
    monkeypatch.setenv("GLABC_TEAM_WAVES", "2")
    test_fast_math_decisions_follow_the_checker_on_the_kernels_own_draws(hip, oracle, FAST_CASES[1])


def test_fast_math_samples_the_same_law(hip):
    """65 536 chains x 1000 iterations of the bench configuration, exact and fast kernel: E theta^2 (analytic 2.081014), E|theta|
    and ESJD agree within 1e-3 relative plus four combined standard errors (north_star's tolerance for posterior moments / ESJD)"""
    from glabcmcmc_amd import _capi as A
    from glabcmcmc_amd import engine
    model, local, glob = descriptors(dict(epsilon=0.05, local=("gauss", [0, 0], [0.35, 0.35]), **{"global": ("gauss", [0, 0], [1, 1])}))
    n, burn, T = 65536, 300, 1000
    dev = torch.device("cuda", 0)
    stats = {}
    for mode in (A.MATH_EXACT, A.MATH_FAST):
        g = torch.Generator().manual_seed(5)
        chains = engine.ChainBatch(torch.zeros(n, 2), (0.05 ** 0.5) * torch.randn(n, 2, generator=g), dev)
        engine.init_weights(model, glob, chains)
        engine.run_steps("glabc_glmcmc_steps", model, local, glob, chains, burn, 1, 99, 0.9, 5, math_mode=mode)
        mom = engine.Moments(n, 2, dev)
        hist = torch.empty(T, 2, n, dtype=torch.float32, device=dev)
        engine.run_steps("glabc_glmcmc_steps", model, local, glob, chains, T, 1 + burn, 99, 0.9, 5, moments=mom, history=hist,
                         math_mode=mode)
        torch.cuda.synchronize()
        sq = (mom.sum_outer[0] / T).cpu().numpy()
        ab = hist[:, 0, :].abs().double().mean(0).cpu().numpy()
        es = mom.esjd().double().cpu().numpy()
        es = es[np.isfinite(es)]                          # a chain whose jump matrix is singular in float32 has no ESJD (bench.py: esjd_nan_frac)
        assert len(es) > 0.99 * n
        stats[mode] = {k: (v.mean(), v.std(ddof=1) / np.sqrt(len(v))) for k, v in (("sq", sq), ("abs", ab), ("esjd", es))}
    for k in ("sq", "abs", "esjd"):
        (a, sa), (b, sb) = stats[A.MATH_EXACT][k], stats[A.MATH_FAST][k]
        assert abs(a - b) <= 1e-3 * abs(a) + 4 * np.hypot(sa, sb), (k, a, b, sa, sb)
    assert abs(stats[A.MATH_FAST]["sq"][0] - 2.081014) < 1e-3 * 2.081014 + 4 * stats[A.MATH_FAST]["sq"][1]


def test_fast_math_is_refused_where_it_does_not_exist(hip):
    from glabcmcmc_amd import _capi as A
    from glabcmcmc_amd import engine
    model, local, glob = descriptors(dict(epsilon=0.3, local=("gauss", [0, 0], [0.3, 0.3]), **{"global": ("gauss", [0, 0], [1, 1])}))
    dev = torch.device("cuda", 0)
    chains = engine.ChainBatch(torch.zeros(8, 2), torch.ones(8, 2), dev).add_mala_state()
    cs = chains.struct()

    def call(fn=hip.glabc_glmcmc_steps, **kw):
        run = A.Run()
        run.seed, run.step0, run.n_steps, run.global_frequency, run.batch_size, run.math_mode = 1, 1, 2, 0.5, 5, A.MATH_FAST
        for k, v in kw.items():
            setattr(run, k, v)
        return fn(C.byref(model), C.byref(local), C.byref(glob), C.byref(cs), C.byref(run), None)

    assert call() == 0
    assert call(batch_size=1) == -4 and call(batch_size=17) == -4 and call(lanes_per_chain=2) == -4 and call(math_mode=2) == -4
    assert call(fn=hip.glabc_globalmcmc_steps) == -4
    do = A.DrawsOut(None, None, None)
    assert call(dump_draws=C.pointer(do)) == -1 and call(math_mode=A.MATH_EXACT, dump_draws=C.pointer(do)) == -4
    torch.cuda.synchronize()
