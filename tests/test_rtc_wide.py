"""User simulators in the lane-group GLMCMC kernel (glabc_rtc_compile_wide, CompiledModel at batch sizes 17..4096).

One run-time compiled program holds wide_kernel (csrc/glabc_wide.h) at 8 / 16 / 32 / 64 lanes per chain around the user's source;
the CPU checker runs the same source through gcc, so kernel and checker are compared bit for bit -- histories, final states,
log-weights, flags, move counts and streamed sums -- at every lane count, at the LDS edge and with the user's hooks.
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import oracle_lib
from helpers import bits, descriptors, load_golden, make_dist
from glabcmcmc_amd import _capi as A
from test_rtc import ALL_USER, NONLINEAR, PRIOR_ONLY, FixedPrior, host_hooks, host_simulator, mixture_source, user_model_desc, wide_source

NL_PRIOR = ("gauss", [0.0, 0.5, 0.0], [1.5, 1.0, 2.0])


def nonlinear_model():
    import glabcmcmc_amd as g_
    return g_.CompiledModel(3, 2, NONLINEAR, make_dist(NL_PRIOR), [0.9, 0.6], 0.15, noise_dim=4)


# ---------------------------------------------------------------------------------------------------------- CPU
def test_compile_wide_reports_errors_and_needs_a_device():
    """hiprtc cross-compiles the four lane counts without a GPU: a valid source compiles and then fails to LOAD here (no
    device); a broken one is refused with the compiler's message; bad dimensions and a NULL source are refused up front"""
    lib = A.lib()
    handle, log = C.c_void_p(), C.create_string_buffer(1 << 14)
    rc = lib.glabc_rtc_compile_wide(NONLINEAR.encode(), 3, 2, 4, C.byref(handle), log, len(log))
    if torch.cuda.is_available():
        assert rc == A.OK, log.value.decode()
        lib.glabc_rtc_release(handle)
    else:
        assert rc == -6, log.value.decode()                                                        # GLABC_ERR_NO_DEVICE
    rc = lib.glabc_rtc_compile_wide(b"GLABC_SIMULATOR void glabc_user_simulate(const float* t, const float* e, float* y) { y[0] = t[0] + ; }",
                                    1, 1, 1, C.byref(handle), log, len(log))
    assert rc == -4 and b"error" in log.value and b"user_simulator" in log.value                   # GLABC_ERR_ARG + the log
    assert lib.glabc_rtc_compile_wide(NONLINEAR.encode(), 9, 2, 4, C.byref(handle), log, len(log)) == -2      # GLABC_ERR_DIM
    assert lib.glabc_rtc_compile_wide(NONLINEAR.encode(), 3, 2, 0, C.byref(handle), log, len(log)) == -2
    assert lib.glabc_rtc_compile_wide(None, 3, 2, 4, C.byref(handle), log, len(log)) == -1                    # GLABC_ERR_NULL


def test_fused_supported_takes_compiled_models_above_16_proposals():
    """GLMCMC's dispatch (max_batch = GLABC_MAX_BATCH_WIDE): a CompiledModel with a descriptor prior runs fused at 17..4096; one
    with a user prior stays split-phase above 16 (only that path redraws the prior sentinel); the other samplers stop at 16"""
    import glabcmcmc_amd as g_
    from glabcmcmc_amd import generic
    lp, ip = make_dist(("gauss", [0.0] * 3, [0.3] * 3)), make_dist(("gauss", [0.0] * 3, [1.5] * 3))
    cm = nonlinear_model()
    for n in (1, 16, 17, 100, 4096):
        assert generic.fused_supported(cm, (lp, ip), n, A.MAX_BATCH_WIDE, gamma_ok=True)
    assert not generic.fused_supported(cm, (lp, ip), 4097, A.MAX_BATCH_WIDE, gamma_ok=True)
    assert not generic.fused_supported(cm, (lp, ip), 17)
    up = g_.CompiledModel(2, 3, PRIOR_ONLY, make_dist(("gauss", [0.0, 0.0], [1.5, 1.5])), [1.0, 0.5, 0.7], 0.4, noise_dim=3)
    lp2, ip2 = make_dist(("gauss", [0.0] * 2, [0.3] * 2)), make_dist(("gauss", [0.0] * 2, [1.5] * 2))
    assert generic.fused_supported(up, (lp2, ip2), 16, A.MAX_BATCH_WIDE, gamma_ok=True)
    assert not generic.fused_supported(up, (lp2, ip2), 17, A.MAX_BATCH_WIDE, gamma_ok=True)


# ---------------------------------------------------------------------------------------------------------- GPU
def run_and_check(oracle, cm, src, N, *, n=1000, T=20, lanes=0, flags=0, seed=11, gf=0.7, chain0=10 ** 10 + 3, glob=None,
                  steps_per_launch=None):
    """cm's wide program on n chains for T iterations (lanes per chain: 0 = the library's choice) == the checker with the same
    source through gcc: histories, states, log-weights, flags, moves and sums bit for bit"""
    from glabcmcmc_amd import engine
    d, yd, nd = cm.theta_dim, cm.y_dim, cm.noise_dim
    lib, fn = host_simulator(src, d, yd, nd)
    oracle.oracle_set_user_simulator(fn)
    oracle.oracle_set_user_model(*host_hooks(lib))
    try:
        model = cm.descriptor()
        local = make_dist(("gauss", [0.0] * d, [0.3] * d)).descriptor()
        glob = glob or make_dist(("gauss", [0.0] * d, [1.5] * d)).descriptor()
        rng = np.random.default_rng(N * 7 + d)
        theta0 = rng.standard_normal((n, d)).astype(np.float32)
        y0 = rng.standard_normal((n, yd)).astype(np.float32)
        dev = torch.device("cuda", 0)
        prog = cm.program(A.ALGO_GLMCMC, N)
        chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev, chain0=chain0)
        hist = torch.empty(T, d, n, device=dev)
        mom = engine.Moments(n, d, dev)
        engine.run_steps(None, model, local, glob, chains, T, 1, seed, gf, N, history=hist, moments=mom, lanes_per_chain=lanes,
                         debug_flags=flags, rtc_program=prog, steps_per_launch=steps_per_launch)
        torch.cuda.synchronize()
        hc = oracle_lib.HostChains(theta0, y0, chain0=chain0)
        hh = np.zeros((T, d, n), np.float32)
        hm = oracle_lib.HostMoments(n, d)
        run, keep = oracle_lib.make_run(seed=seed, step0=1, n_steps=T, gf=gf, batch=N, history=hh, moments=hm)
        cs = hc.struct()
        assert oracle.oracle_glmcmc_steps(C.byref(model), C.byref(local), C.byref(glob), C.byref(cs), C.byref(run)) == 0
        same = bits(hist.cpu().numpy()) == bits(hh)
        assert same.all(), "first history mismatch at (t, dim, chain) = %s" % (np.argwhere(~same)[0],)
        assert np.array_equal(bits(chains.theta.cpu().numpy()), bits(hc.theta))
        assert np.array_equal(bits(chains.y.cpu().numpy()), bits(hc.y))
        assert np.array_equal(bits(chains.log_w.cpu().numpy()), bits(hc.log_w))
        assert np.array_equal(chains.flags.cpu().numpy().astype(np.uint32), hc.flags)
        assert np.array_equal(chains.n_moves.cpu().numpy().astype(np.uint32), hc.n_moves) and hc.n_moves.sum() > 0
        assert np.array_equal(mom.sum_theta.cpu().numpy(), hm.sum_theta)
        assert np.array_equal(mom.sum_outer.cpu().numpy(), hm.sum_outer) and np.array_equal(mom.sum_jump.cpu().numpy(), hm.sum_jump)
        return hc
    finally:
        oracle.oracle_set_user_model(None, None, None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["glmcmc_philox_n32", "glmcmc_philox_n100"])
def test_hip_compiled_model_walks_the_reference_chains_wide(hip, name):
    """The reference's example simulator as user source, through MCMCRunner with path="fused": the reference's golden chains at
    N = 32 and N = 100, bit for bit (the wide rtc path -- embedded headers, argument block, LDS, dispatch -- pinned to the reference)"""
    import glabcmcmc_amd as g_
    from test_generic_path import FixedDescriptor
    g = load_golden(name)
    cfg = g["cfg"]
    assert cfg["N"] > A.MAX_BATCH
    model, local, glob = descriptors(cfg, g)
    cm = g_.CompiledModel(2, 2, mixture_source(g["c_noise_scale"]), FixedPrior(model.prior), list(model.y_obs)[:2], cfg["epsilon"])
    cm.descriptor = lambda epsilon=None, _m=user_model_desc(model, 2): _m
    th0, y0 = torch.from_numpy(g["theta0"]), torch.from_numpy(g["y0"])
    out = g_.MCMCRunner(cm).run_glmcmc(cfg["T"] + 1, th0, y0, cfg["gf"], FixedDescriptor(local), FixedDescriptor(glob), cfg["N"],
                                       seed=cfg["seed"], chain0=cfg.get("chain0", 0), output_file=None, verbose=False, path="fused")
    assert (A.ALGO_GLMCMC, cm.WIDE) in cm._programs
    same = bits(out.numpy()) == bits(g["chains"])
    assert same.all(), "first mismatch at (t, chain, dim) = %s" % (np.argwhere(~same)[0],)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [17, 31, 32, 33, 64, 65, 100, 256, 1000, 4096])
def test_hip_wide_nonlinear_user_simulator_equals_oracle(hip, oracle, N):
    """theta 3, y 2, 4 normals, exp / log / sqrt / fma in the simulator; 1000 chains (a multiple of no group count), chain0 != 0,
    gf 0.7: kernel == checker at every default lane count, N = 4096 (L = 64, 66 KB of LDS: above the 48 KB default) included"""
    T = 20 if N <= 256 else (4 if N <= 1000 else 2)
    run_and_check(oracle, nonlinear_model(), NONLINEAR, N, T=T, seed=4242 + N)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [100, 300])
@pytest.mark.parametrize("lanes", [8, 16, 32, 64])
def test_hip_wide_every_lane_group_equals_oracle(hip, oracle, N, lanes):
    """every instantiation of the program (forced L), and the sequential index redo (GLABC_DEBUG_EXACT_INDEX), == the checker"""
    cm = nonlinear_model()
    run_and_check(oracle, cm, NONLINEAR, N, n=600, T=10, lanes=lanes, seed=N + lanes)
    run_and_check(oracle, cm, NONLINEAR, N, n=300, T=6, lanes=lanes, flags=A.DEBUG_EXACT_INDEX, seed=N + lanes)


@pytest.mark.gpu
@pytest.mark.parametrize("source,N", [(ALL_USER, 32), (ALL_USER, 257), (PRIOR_ONLY, 32)], ids=["all-32", "all-257", "prior-32"])
def test_hip_wide_user_hooks_equal_oracle(hip, oracle, source, N):
    """a Laplace prior, a weighted L1 discrepancy and an Epanechnikov kernel as user source inside the wide kernel == the
    checker with the same hooks; path="fused" runs the Model (user-prior Models stay split-phase under "auto") and its
    self-check passed"""
    import glabcmcmc_amd as g_
    cm = g_.CompiledModel(2, 3, source, make_dist(("gauss", [0.0, 0.0], [1.5, 1.5])), [1.0, 0.5, 0.7], 0.4, noise_dim=3)
    run_and_check(oracle, cm, source, N, T=15, seed=777 + N, glob=make_dist(("gauss", [0.0, 0.0], [1.6, 1.6])).descriptor())
    lp, ip = make_dist(("gauss", [0.0] * 2, [0.3] * 2)), make_dist(("gauss", [0.0] * 2, [1.6] * 2))
    th0 = torch.randn(300, 2, generator=torch.Generator().manual_seed(N))
    y0 = cm.generate_samples(th0)
    fused = g_.GLMCMC(cm, 21, th0, y0, lp, None, 0.6, ip, N, seed=5, verbose=False, path="fused")
    split = g_.GLMCMC(cm, 21, th0, y0, lp, None, 0.6, ip, N, seed=5, verbose=False, path="generic", sentinel_redraw=False)
    assert np.array_equal(bits(fused.numpy()), bits(split.numpy())) and (fused[1:] != fused[:-1]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("d,yd,nd", [(1, 1, 1), (8, 8, 8), (2, 5, 7), (8, 1, 3), (4, 8, 8)])
def test_hip_wide_user_simulators_of_every_shape_equal_oracle(hip, oracle, d, yd, nd):
    """theta / y / noise dimensions 1..8 (noise count != y_dim: the Philox layout of chain_step with ND normals) at N = 24"""
    import glabcmcmc_amd as g_
    src = wide_source(d, yd, nd)
    cm = g_.CompiledModel(d, yd, src, make_dist(("gauss", [0.0] * d, [1.5] * d)), [0.8] * yd, 0.4, noise_dim=nd)
    run_and_check(oracle, cm, src, 24, n=500, T=12, seed=99 + d * 10 + nd, glob=make_dist(("gauss", [0.0] * d, [1.2] * d)).descriptor())


@pytest.mark.gpu
def test_hip_wide_dispatch(hip, monkeypatch):
    """path="auto": a descriptor prior at N = 48 runs the wide program (the Model's program cache holds it, one launch per
    steps_per_launch went to glabc_rtc_steps) and equals the split-phase path without the sentinel redraw; a user prior stays
    split-phase; one iteration per launch == every iteration in one launch"""
    import glabcmcmc_amd as g_
    from glabcmcmc_amd import engine
    cm = nonlinear_model()
    lp, ip = make_dist(("gauss", [0.0] * 3, [0.3] * 3)), make_dist(("gauss", [0.0] * 3, [1.5] * 3))
    th0 = torch.randn(700, 3, generator=torch.Generator().manual_seed(3))
    y0 = cm.generate_samples(th0)
    calls = []
    real = engine.run_steps
    monkeypatch.setattr(engine, "run_steps", lambda *a, **k: (calls.append(k.get("rtc_program")), real(*a, **k))[1])
    auto = g_.GLMCMC(cm, 31, th0, y0, lp, None, 0.7, ip, 48, seed=21, verbose=False)
    assert (A.ALGO_GLMCMC, cm.WIDE) in cm._programs and (A.ALGO_GLMCMC, 48) in cm._checked
    assert calls and calls[-1] is cm._programs[(A.ALGO_GLMCMC, cm.WIDE)]
    monkeypatch.setattr(engine, "run_steps", real)
    split = g_.GLMCMC(cm, 31, th0, y0, lp, None, 0.7, ip, 48, seed=21, verbose=False, path="generic", sentinel_redraw=False)
    assert np.array_equal(bits(auto.numpy()), bits(split.numpy())) and (auto[1:] != auto[:-1]).any()
    one = g_.GLMCMC(cm, 31, th0, y0, lp, None, 0.7, ip, 48, seed=21, verbose=False, path="fused", steps_per_launch=1)
    assert np.array_equal(bits(auto.numpy()), bits(one.numpy()))

    up = g_.CompiledModel(2, 3, PRIOR_ONLY, make_dist(("gauss", [0.0, 0.0], [1.5, 1.5])), [1.0, 0.5, 0.7], 0.4, noise_dim=3)
    lp2, ip2 = make_dist(("gauss", [0.0] * 2, [0.3] * 2)), make_dist(("gauss", [0.0] * 2, [1.6] * 2))
    th2 = torch.randn(200, 2, generator=torch.Generator().manual_seed(4))
    y2 = up.generate_samples(th2)
    a = g_.GLMCMC(up, 11, th2, y2, lp2, None, 0.6, ip2, 40, seed=8, verbose=False)
    assert (A.ALGO_GLMCMC, up.WIDE) not in up._programs
    b = g_.GLMCMC(up, 11, th2, y2, lp2, None, 0.6, ip2, 40, seed=8, verbose=False, path="generic")
    assert np.array_equal(bits(a.numpy()), bits(b.numpy()))


@pytest.mark.gpu
def test_hip_wide_self_check_refuses_a_mismatch(hip, monkeypatch):
    """a wide program whose self-check sees a mismatch (here: the split-phase run it compares against is perturbed) is never
    handed out: path="fused" raises SimulatorSelfCheckError, path="auto" warns and returns the split-phase result"""
    import glabcmcmc_amd as g_
    from glabcmcmc_amd import generic
    from glabcmcmc_amd.compiled import SimulatorSelfCheckError
    real = generic.run

    def perturbed(*a, **k):
        out = real(*a, **k)
        # the self-check's split-phase run of a GLMCMC program above 16 proposals only
        if a[0] == A.ALGO_GLMCMC and int(a[9]) > A.MAX_BATCH and k.get("sentinel_redraw") is False and k.get("graph") is False:
            out = out.clone()
            out[1, 0, 0] += 1.0
        return out

    monkeypatch.setattr(generic, "run", perturbed)
    cm = nonlinear_model()
    lp, ip = make_dist(("gauss", [0.0] * 3, [0.3] * 3)), make_dist(("gauss", [0.0] * 3, [1.5] * 3))
    th0 = torch.randn(64, 3, generator=torch.Generator().manual_seed(5))
    y0 = cm.generate_samples(th0)
    with pytest.raises(SimulatorSelfCheckError):
        g_.GLMCMC(cm, 6, th0, y0, lp, None, 0.5, ip, 40, seed=1, verbose=False, path="fused")
    assert (A.ALGO_GLMCMC, cm.WIDE) not in cm._programs
    with pytest.raises(SimulatorSelfCheckError):
        cm.program(A.ALGO_GLMCMC, 100)                                         # the verdict covers the one wide program
    cm2 = nonlinear_model()
    with pytest.warns(RuntimeWarning, match="split-phase"):
        got = g_.GLMCMC(cm2, 6, th0, y0, lp, None, 0.5, ip, 40, seed=1, verbose=False)
    assert (A.ALGO_GLMCMC, cm2.WIDE) not in cm2._programs
    want = g_.GLMCMC(cm2, 6, th0, y0, lp, None, 0.5, ip, 40, seed=1, verbose=False, path="generic")
    assert np.array_equal(bits(got.numpy()), bits(want.numpy()))
    monkeypatch.setattr(generic, "run", real)
    assert cm2.program(A.ALGO_GLMCMC, 12)                                      # register programs are untouched by the verdict


@pytest.mark.gpu
def test_hip_wide_lds_edge(hip, oracle):
    """N = 4096 at the default L = 64 needs 66 KB of LDS and runs (== the checker); a forced L = 8 there would need 528 KB: it is
    refused with GLABC_ERR_ARG before anything runs -- the chains, history and sums are left as they were"""
    from glabcmcmc_amd import engine
    cm = nonlinear_model()
    run_and_check(oracle, cm, NONLINEAR, 4096, n=300, T=2, seed=1)
    model = cm.descriptor()
    local = make_dist(("gauss", [0.0] * 3, [0.3] * 3)).descriptor()
    glob = make_dist(("gauss", [0.0] * 3, [1.5] * 3)).descriptor()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    theta0, y0 = rng.standard_normal((256, 3)).astype(np.float32), rng.standard_normal((256, 2)).astype(np.float32)
    chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev)
    hist = torch.full((3, 3, 256), float("nan"), device=dev)
    mom = engine.Moments(256, 3, dev)
    for lanes, N in ((8, 4096), (16, 4096), (8, 2000)):
        with pytest.raises(RuntimeError, match=re.escape("status -4")):
            engine.run_steps(None, model, local, glob, chains, 3, 1, 7, 0.7, N, history=hist, moments=mom, lanes_per_chain=lanes,
                             rtc_program=cm.program(A.ALGO_GLMCMC, N))
    torch.cuda.synchronize()
    assert torch.isnan(hist).all() and float(mom.sum_outer.abs().sum()) == 0.0
    assert np.array_equal(bits(chains.theta.cpu().numpy()), bits(np.ascontiguousarray(theta0.T)))
    assert int(chains.n_moves.sum()) == 0


@pytest.mark.gpu
def test_hip_wide_program_refuses_register_batch_sizes(hip):
    """the wide program takes 17..4096 proposals and lanes per chain 0 / 8 / 16 / 32 / 64 only"""
    from glabcmcmc_amd import engine
    cm = nonlinear_model()
    prog = cm.program(A.ALGO_GLMCMC, 20)
    model = cm.descriptor()
    d = make_dist(("gauss", [0.0] * 3, [1.0] * 3)).descriptor()
    chains = engine.ChainBatch(torch.zeros(64, 3), torch.zeros(64, 2), torch.device("cuda", 0))
    for N, lanes in ((16, 0), (5, 0), (4097, 0), (20, 1), (20, 4), (20, 128)):
        with pytest.raises(RuntimeError, match=re.escape("status -4")):
            engine.run_steps(None, model, d, d, chains, 2, 1, 7, 0.7, N, lanes_per_chain=lanes, rtc_program=prog)
    assert int(chains.n_moves.sum()) == 0
