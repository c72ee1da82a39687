"""glabc_propose_mix -- the split-phase twin of the mixture kernels: glabc_propose(algo, local, NULL) plus, in the same launch, the
global candidates and their log q from a GaussianMixture on the kernel's Philox stream, and q_cur for every chain.

Against the checker, bit for bit: oracle_propose(algo, local, NULL) gives the head draws, is_global, the local move's row and sim_noise;
the numpy restatement (tests/mixture_ref.py) gives the rows the mixture fills and q_cur.  Every io buffer sits between canary guard
bands.  Then whole chains: glabc_propose_mix -> the checker's Model callbacks on the device's candidates -> glabc_select against the
reference chain of tests/test_rtc_mix.py; generic.run(kernel_stream=True) on a built-in Model against the fused mixture kernels; and
the self-check of a mixture program, which runs on this path.  CPU: the argument checks, in their order.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mixture_ref
import oracle_lib
from helpers import CANARY_BITS, bits, make_dist
from test_arg_checks import ARG, DIM, KIND, NULL, OK, check_table
from test_mix_arg_checks import MIX
from test_mixture_host import make_mixture
from test_rtc import NONLINEAR, host_hooks, host_simulator
from glabcmcmc_amd import _capi as A

SEED, CHAIN0, GF, GUARD = 31, 2 ** 32 + 7, 0.6, 64
ALGO = {"glmcmc": A.ALGO_GLMCMC, "globalmcmc": A.ALGO_GLOBALMCMC}


# ---- CPU: check_propose_mix ---------------------------------------------------------------------------------------------------
def test_check_propose_mix(tmp_path_factory):
    base = ("glabc_dist lo = dist3(GLABC_DIST_DIAG_GAUSS); " + MIX + "glabc_step_io io; std::memset(&io, 0, sizeof io); io.n_prop = 5; "
            "io.theta_dim = 3; io.y_dim = 2; io.noise_dim = 4; io.q_cur = b.f; glabc_tape tp; std::memset(&tp, 0, sizeof tp); (void)tp; "
            "int algo = GLABC_ALGO_GLMCMC; ")
    call = "check_propose_mix(algo, &lo, &g, &b.c, &b.r, &io)"
    rows = [(base + spoil, c, want) for spoil, want, c in (
        ("", OK, call), ("algo = GLABC_ALGO_GLOBALMCMC;", OK, call), ("", OK, "check_propose_mix(algo, nullptr, &g, &b.c, &b.r, &io)"),
        ("", NULL, "check_propose_mix(algo, &lo, &g, &b.c, &b.r, nullptr)"),
        ("algo = GLABC_ALGO_GLMALA;", KIND, call), ("algo = 7; io.theta_dim = 9;", KIND, call),
        ("io.theta_dim = 9;", DIM, call), ("io.theta_dim = 0; g.n_modes = 0;", DIM, call),
        ("", NULL, "check_propose_mix(algo, &lo, nullptr, &b.c, &b.r, &io)"),
        ("g.n_modes = 9;", ARG, call), ("g.dim = 2;", DIM, call), ("g.n_modes = 0; g.dim = 2;", ARG, call), ("g.scale[0][1] = 0.0;", ARG, call),
        ("g.cum_weight[2] = 1.5;", ARG, call), ("g.dim = 2; lo.dim = 2;", DIM, call), ("g.c0 = NaN; lo.p2[0] = NaN;", ARG, call),
        ("lo.dim = 2;", DIM, call), ("lo = dist3(GLABC_DIST_GAMMA);", KIND, call), ("lo.p2[1] = -1.0f;", ARG, call),
        ("lo.dim = 2;", DIM, "check_propose_mix(algo, &lo, &g, nullptr, &b.r, &io)"),
        ("", NULL, "check_propose_mix(algo, &lo, &g, nullptr, &b.r, &io)"), ("", NULL, "check_propose_mix(algo, &lo, &g, &b.c, nullptr, &io)"),
        ("b.r.tape = &tp;", ARG, call), ("b.r.tape = &tp; io.q_cur = nullptr;", ARG, call), ("io.q_cur = nullptr;", NULL, call))]
    check_table(tmp_path_factory, "propose_mix", rows, flags=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


# ---- GPU: one launch against the checker --------------------------------------------------------------------------------------
def guarded(shape, dtype):
    """a device buffer between two guard bands of canaries -> (whole tensor, view of the interior)"""
    n = int(np.prod(shape))
    item = np.dtype(dtype).itemsize
    fill = np.full(n + 2 * GUARD, CANARY_BITS, np.uint32) if item == 4 else np.full(n + 2 * GUARD, 0xFFF8DEADC0DEDEAD, np.uint64)
    whole = torch.from_numpy(fill.view(np.int32 if item == 4 else np.int64)).cuda()
    return whole, whole[GUARD:GUARD + n]


def guards_intact(whole):
    w = whole.cpu().numpy()
    canary = np.uint32(CANARY_BITS) if w.dtype == np.int32 else np.uint64(0xFFF8DEADC0DEDEAD)
    u = w.view(np.uint32 if w.dtype == np.int32 else np.uint64)
    return bool((u[:GUARD] == canary).all() and (u[-GUARD:] == canary).all())


SHAPES = {1: (8, 40, 1, 1), 2: (3, 5, 2, 2), 3: (3, 17, 2, 4), 4: (1, 16, 4, 4), 5: (3, 1, 5, 5), 6: (8, 5, 3, 8), 7: (1, 17, 7, 7), 8: (3, 40, 8, 8)}


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["glmcmc", "globalmcmc"])
@pytest.mark.parametrize("d", range(1, 9))
def test_hip_propose_mix_equals_the_checker(hip, oracle, d, algo):
    """theta_prop, log_q, sim_noise, log_u, u_res, is_global and q_cur at 65 chains and at one; modes 1 / 3 / 8, batch sizes
    1 / 5 / 16 / 17 / 40, noise_dim != y_dim at theta_dim 3 and 6; a Uniform local increment at the even dimensions"""
    K, N, yd, nd = SHAPES[d]
    N = N if algo == "glmcmc" else 1
    mix = make_mixture(K, d, spread=1.5).descriptor()
    ref = mixture_ref.MixtureRef.from_descriptor(mix)
    lp = make_dist(("uniform", [-0.5] * d, [0.5] * d) if d % 2 == 0 else ("gauss", [0.0] * d, [0.35] * d)).descriptor()
    for n in (65, 1):
        rng = np.random.default_rng(100 * d + n)
        theta0 = (1.5 * rng.standard_normal((n, d))).astype(np.float32)
        y0 = rng.standard_normal((n, yd)).astype(np.float32)
        R = N * n
        # the checker
        hc = oracle_lib.HostChains(theta0, y0, chain0=CHAIN0)
        cs = hc.struct()
        want = dict(theta_prop=np.zeros((R, d), np.float32), log_q=np.zeros(R, np.float32), sim_noise=np.zeros((R, nd), np.float32),
                    log_u=np.zeros(n, np.float32), u_res=np.zeros(n, np.float64), is_global=np.zeros(n, np.int32))
        io = A.StepIO(N, d, yd, nd, *[want[k].ctypes.data for k in ("theta_prop", "log_q", "sim_noise", "log_u", "u_res", "is_global")])
        run, keep = oracle_lib.make_run(seed=SEED, step0=3, n_steps=1, gf=GF, batch=N)
        assert oracle.oracle_propose(ALGO[algo], C.byref(lp), None, C.byref(cs), C.byref(run), C.byref(io)) == 0
        theta_c, log_q_c = ref.candidates(SEED, np.uint64(CHAIN0) + np.arange(n, dtype=np.uint64), 3, N, nd)
        for j in range(N):
            rows = np.ones(n, bool) if j else (want["is_global"] & 1).astype(bool)
            want["theta_prop"][j * n:(j + 1) * n][rows] = theta_c[j][rows]
            want["log_q"][j * n:(j + 1) * n][rows] = log_q_c[j][rows]
        want["q_cur"] = ref.log_prob_f32(theta0)
        if n == 65:
            assert 0 < int((want["is_global"] & 1).sum()) < n                # both branches
        # the device
        from glabcmcmc_amd import engine
        chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), torch.device("cuda", 0), chain0=CHAIN0)
        dcs = chains.struct()
        buf = {k: guarded(v.shape, v.dtype) for k, v in want.items()}
        dio = A.StepIO()
        dio.n_prop, dio.theta_dim, dio.y_dim, dio.noise_dim = N, d, yd, nd
        for k in buf:
            setattr(dio, k, buf[k][1].data_ptr())
        drun = A.Run()
        drun.seed, drun.step0, drun.n_steps, drun.global_frequency, drun.batch_size = SEED, 3, 1, GF, N
        assert hip.glabc_propose_mix(ALGO[algo], C.byref(lp), C.byref(mix), C.byref(dcs), C.byref(drun), C.byref(dio), None) == 0
        torch.cuda.synchronize()
        for k, v in want.items():
            got = buf[k][1].cpu().numpy().view(v.dtype).reshape(v.shape)
            assert guards_intact(buf[k][0]), (k, n)
            same = got.view(np.uint8).reshape(v.shape[0], -1) == np.ascontiguousarray(v).view(np.uint8).reshape(v.shape[0], -1)
            assert same.all(), "%s: first differing row %d of %d (n = %d)" % (k, np.argwhere(~same.all(axis=1))[0][0], v.shape[0], n)
        assert np.array_equal(bits(chains.theta.cpu().numpy()), bits(hc.theta))  # the state is read, never written


# ---- GPU: whole chains through glabc_propose_mix -> callbacks -> glabc_select ----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("which,N", [("all_user", 5), ("nonlinear", 17)])
def test_hip_propose_mix_and_select_walk_the_reference_chain(hip, oracle, which, N):
    """theta_dim 2 at N = 5 (every Model callback user source) and theta_dim 3 at N = 17: 20 iterations, the Model callbacks the checker's
    on the device's candidates"""
    import test_rtc_mix as M
    from glabcmcmc_amd import engine
    steps, n = 20, M.N_CHAINS
    hh, hc, hm, modes = M.reference(oracle, "glmcmc", which, N, steps=steps)
    src, d, yd, nd, prior, y_obs, eps, K = M.user_case(which)
    theta0, y0, lp_o, mix_o = M.start(which, n)
    model, lp, mix = M.compiled_model(which).descriptor(), lp_o.descriptor(), mix_o.descriptor()
    lib, fn = host_simulator(src, d, yd, nd)
    oracle.oracle_set_user_simulator(fn)
    oracle.oracle_set_user_model(*host_hooks(lib))
    try:
        dev = torch.device("cuda", 0)
        chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev, chain0=M.CHAIN0)
        cs = chains.struct()
        R = N * n
        f32 = dict(dtype=torch.float32, device=dev)
        t = dict(theta_prop=torch.zeros(R, d, **f32), log_q=torch.zeros(R, **f32), sim_noise=torch.zeros(R, nd, **f32), log_u=torch.zeros(n, **f32),
                 u_res=torch.zeros(n, dtype=torch.float64, device=dev), is_global=torch.zeros(n, dtype=torch.int32, device=dev),
                 y_prop=torch.zeros(R, yd, **f32), prior_prop=torch.zeros(R, **f32), kern_prop=torch.zeros(R, **f32),
                 prior_cur=torch.zeros(n, **f32), kern_cur=torch.zeros(n, **f32), q_cur=torch.zeros(n, **f32))
        host = dict(prior=np.zeros(R, np.float32), y=np.zeros((R, yd), np.float32), kern=np.zeros(R, np.float32))
        pc, kc = np.zeros(n, np.float32), np.zeros(n, np.float32)
        assert oracle.oracle_model_prior_log_prob(C.byref(model), np.ascontiguousarray(theta0).ctypes.data, n, pc.ctypes.data) == 0
        assert oracle.oracle_model_log_kernel(C.byref(model), np.ascontiguousarray(y0).ctypes.data, n, kc.ctypes.data) == 0
        t["prior_cur"].copy_(torch.from_numpy(pc))
        t["kern_cur"].copy_(torch.from_numpy(kc))
        io = A.StepIO()
        io.n_prop, io.theta_dim, io.y_dim, io.noise_dim = N, d, yd, nd
        for k, v in t.items():
            setattr(io, k, v.data_ptr())
        hist = torch.zeros(steps, d, n, **f32)
        for i in range(steps):
            run = A.Run()
            run.seed, run.step0, run.n_steps, run.global_frequency, run.batch_size = M.SEED, 1 + i, 1, M.GF, N
            run.history, run.hist_stride = hist[i].data_ptr(), n
            assert hip.glabc_propose_mix(A.ALGO_GLMCMC, C.byref(lp), C.byref(mix), C.byref(cs), C.byref(run), C.byref(io), None) == 0
            th, noise = np.ascontiguousarray(t["theta_prop"].cpu().numpy()), np.ascontiguousarray(t["sim_noise"].cpu().numpy())
            assert oracle.oracle_model_prior_log_prob(C.byref(model), th.ctypes.data, R, host["prior"].ctypes.data) == 0
            M.simulate_rows(oracle, lib, model, th, noise, host["y"])
            assert oracle.oracle_model_log_kernel(C.byref(model), host["y"].ctypes.data, R, host["kern"].ctypes.data) == 0
            t["prior_prop"].copy_(torch.from_numpy(host["prior"]))
            t["y_prop"].copy_(torch.from_numpy(host["y"]))
            t["kern_prop"].copy_(torch.from_numpy(host["kern"]))
            assert hip.glabc_select(A.ALGO_GLMCMC, None, C.byref(cs), C.byref(run), C.byref(io), None) == 0
        torch.cuda.synchronize()
    finally:
        oracle.oracle_set_user_model(None, None, None)
        oracle.oracle_set_user_simulator(None)
    assert modes == K and int((hc.n_moves > 0).sum()) >= n // 2
    same = bits(hist.cpu().numpy()) == bits(hh)
    assert same.all(), "first mismatch at (t, dim, chain) = %s" % (np.argwhere(~same)[0],)
    assert np.array_equal(bits(chains.y.cpu().numpy()), bits(hc.y))
    assert np.array_equal(chains.flags.cpu().numpy().astype(np.uint32), hc.flags)
    assert np.array_equal(chains.n_moves.cpu().numpy().astype(np.uint32), hc.n_moves)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [5, 40])
def test_hip_kernel_stream_on_a_builtin_model_equals_the_fused_kernels(hip, N):
    """GLMCMC(Mixture_set, GaussianMixture): path='generic' with kernel_stream=True (glabc_propose_mix, the row-wise Model kernels,
    glabc_select) against path='fused' (glabc_glmcmc_mix_steps / _mix_wide_steps): two device paths, one chain"""
    import glabcmcmc_amd as g_
    from glabcmcmc_amd.examples.Mixture import Mixture_set
    model, mix = Mixture_set(0.4), make_mixture(3, 2, spread=1.5)
    lp = make_dist(("gauss", [0.0] * 2, [0.35] * 2))
    rng = np.random.default_rng(N)
    theta0 = torch.from_numpy((1.5 * rng.standard_normal((96, 2))).astype(np.float32))
    y0 = (theta0.abs() + 0.2236 * torch.from_numpy(rng.standard_normal((96, 2)).astype(np.float32)))
    kw = dict(seed=SEED, chain0=CHAIN0, verbose=False)
    fused = g_.GLMCMC(model, 14, theta0, y0, lp, None, GF, mix, N, path="fused", **kw)
    state = {}
    split = g_.GLMCMC(model, 14, theta0, y0, lp, None, GF, mix, N, path="generic", kernel_stream=True, state_out=state, **kw)
    assert "callback_device" in state                                        # the split-phase path ran
    assert fused.shape == (14, 96, 2) and (fused[-1] != fused[0]).any()
    assert np.array_equal(bits(fused.numpy()), bits(split.numpy()))
    plain = g_.GLMCMC(model, 14, theta0, y0, lp, None, GF, mix, N, path="generic", **kw)       # torch's generator: another stream
    assert torch.isfinite(plain).all() and not np.array_equal(bits(plain.numpy()), bits(split.numpy()))


@pytest.mark.gpu
def test_hip_compiled_model_paths_agree_on_a_mixture(hip):
    """CompiledModel(NONLINEAR) with a three-mode mixture: path='auto' (the mixture program) equals path='generic', kernel_stream=True"""
    import glabcmcmc_amd as g_
    import test_rtc_mix as M
    cm = M.compiled_model("nonlinear")
    theta0, y0, lp, mix = M.start("nonlinear", 64)
    t0, yy0 = torch.from_numpy(theta0), torch.from_numpy(y0)
    kw = dict(seed=SEED, chain0=CHAIN0, verbose=False)
    for N in (6, 40):
        a = g_.GLMCMC(cm, 12, t0, yy0, lp, None, GF, mix, N, **kw)
        b = g_.GLMCMC(cm, 12, t0, yy0, lp, None, GF, mix, N, path="generic", kernel_stream=True, sentinel_redraw=False, **kw)
        assert np.array_equal(bits(a.numpy()), bits(b.numpy())), N
    a = g_.GlobalMCMC(cm, 12, t0, yy0, mix, None, GF, lp, **kw)
    b = g_.GlobalMCMC(cm, 12, t0, yy0, mix, None, GF, lp, path="generic", kernel_stream=True, **kw)
    assert np.array_equal(bits(a.numpy()), bits(b.numpy())) and (a[-1] != a[0]).any()


@pytest.mark.gpu
def test_hip_self_check_of_a_mixture_program(hip, monkeypatch):
    """the library's own options: checked and accepted.  With the SLP vectorizer switched back on (a debugging knob) the check either
    refuses the program, and the verdict sticks, or the toolchain compiles this configuration correctly (skip), as
    tests/test_rtc.py::test_hip_self_check_refuses_a_miscompiled_kernel"""
    import glabcmcmc_amd as g_
    from glabcmcmc_amd.compiled import SimulatorSelfCheckError
    prior = make_dist(("gauss", [0.0, 0.5, 0.0], [1.5, 1.0, 2.0]))
    cm2 = g_.CompiledModel(3, 2, NONLINEAR, prior, [0.9, 0.6], 0.15, noise_dim=4)
    assert cm2.program(A.ALGO_GLMCMC, 12, mixture=True) and (A.ALGO_GLMCMC, 12, cm2.MIXTURE) in cm2._checked
    monkeypatch.setenv("GLABC_RTC_OPTS", "-fslp-vectorize")
    monkeypatch.setenv("GLABC_RTC_LANES", "1")
    cm = g_.CompiledModel(3, 2, NONLINEAR, prior, [0.9, 0.6], 0.15, noise_dim=4)
    try:
        cm.program(A.ALGO_GLMCMC, 12, mixture=True)
    except SimulatorSelfCheckError as e:
        assert "disagrees with the split-phase path" in str(e)
    else:
        pytest.skip("this toolchain compiles the configuration correctly with the SLP vectorizer on")
    with pytest.raises(SimulatorSelfCheckError):
        cm.program(A.ALGO_GLMCMC, 12, mixture=True)
    assert (A.ALGO_GLMCMC, 12, cm.MIXTURE) not in cm._programs
