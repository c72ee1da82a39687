"""GaussianMixture proposals on run-time compiled Models: the mixture programs (glabc_rtc_compile_mix / glabc_rtc_compile_wide_mix) and
their launch glabc_rtc_mix_steps, bit for bit.

Same code, simulator inlined: the |theta| + noise simulator as user source in a mixture program equals the built-in mixture kernels.
A simulator the built-in kernels do not have: against a split-phase reference chain built the way tests/test_mixture_shapes.py builds
one -- oracle_propose(algo, local, NULL) -> the numpy restatement (tests/mixture_ref.py) fills the global candidates -> the checker's
Model callbacks, with the user's source compiled by gcc -> q_cur from the restatement -> oracle_select(algo, NULL).  Launches are cut
every 13 iterations, the chains' ids start at 2^32 + 7.  Then the refusals on the device and the package level (GLMCMC / GlobalMCMC
with path="auto" on a CompiledModel run the mixture program).

CPU: generic.fused_supported's matrix for a CompiledModel with a mixture, and the compile entry points' argument checks.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mixture_ref
import oracle_lib
from helpers import AbsGaussModel, bits, canary_f32, canary_left, make_dist
from test_mixture_host import make_mixture
from test_rtc import ALL_USER, NONLINEAR, FixedPrior, host_hooks, host_simulator, mixture_source, user_model_desc, wide_source
from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import distribution, generic

SEED, CHAIN0, GF = 23, 2 ** 32 + 7, 0.6              # the high counter word is live
N_CHAINS, T, K_LAUNCH = 96, 40, 13                    # one full and one half-filled wavefront; launches cut every 13
OK, NULL, DIM, KIND, ARG = 0, -1, -2, -3, -4
ALGO = {"glmcmc": A.ALGO_GLMCMC, "globalmcmc": A.ALGO_GLOBALMCMC}


# ---- fixtures -------------------------------------------------------------------------------------------------------------
def user_case(which):
    """(source, theta_dim, y_dim, noise_dim, prior, y_obs, epsilon, modes)"""
    if which == "nonlinear":
        return NONLINEAR, 3, 2, 4, make_dist(("gauss", [0.0, 0.5, 0.0], [1.5, 1.0, 2.0])), [0.9, 0.6], 0.15, 3
    if which == "all_user":
        return ALL_USER, 2, 3, 3, make_dist(("gauss", [0.0, 0.0], [1.5, 1.5])), [1.0, 0.5, 0.7], 0.4, 3
    d, yd, nd = (int(c) for c in which)                                       # "888", "111", "638": tests/test_rtc.py wide_source
    return wide_source(d, yd, nd), d, yd, nd, make_dist(("gauss", [0.0] * d, [1.5] * d)), [0.8] * yd, 0.4, 8 if d == 1 else 3


_MODELS = {}


def compiled_model(which):
    """one CompiledModel per fixture for the module: its wide mixture program is compiled once"""
    import glabcmcmc_amd as g_
    if which not in _MODELS:
        src, d, yd, nd, prior, y_obs, eps, K = user_case(which)
        _MODELS[which] = g_.CompiledModel(d, yd, src, prior, y_obs, eps, noise_dim=nd)
    return _MODELS[which]


def start(which, n):
    src, d, yd, nd, prior, y_obs, eps, K = user_case(which)
    rng = np.random.default_rng(7 + d + n)
    theta0 = (1.2 * rng.standard_normal((n, d))).astype(np.float32)
    y0 = (np.asarray(y_obs, np.float32) + 0.3 * rng.standard_normal((n, yd))).astype(np.float32)
    step = 0.3 if d <= 4 else 0.15                                            # the local move still accepts in 6 and 8 dimensions
    return theta0, y0, make_dist(("gauss", [0.0] * d, [step] * d)), make_mixture(K, d, spread=1.5)


def simulate_rows(L, lib, model, theta, noise, y):
    """oracle_model_simulate, which strides the noise rows by y_dim; where a simulator takes another number of normals the rows go
    to the checker's simulator (the same gcc build of the source) one by one"""
    if noise.shape[1] == y.shape[1]:
        assert L.oracle_model_simulate(C.byref(model), theta.ctypes.data, noise.ctypes.data, theta.shape[0], y.ctypes.data) == 0
        return
    sim = lib.glabc_user_simulate_host
    sim.argtypes, sim.restype = [C.c_void_p] * 3, None
    tp, ep, yp = theta.ctypes.data, noise.ctypes.data, y.ctypes.data
    ts, es, ys = theta.strides[0], noise.strides[0], y.strides[0]
    for i in range(theta.shape[0]):
        sim(tp + ts * i, ep + es * i, yp + ys * i)


_REF = {}


def reference(oracle, algo, which, N, n=N_CHAINS, steps=T):
    """the split-phase reference chain of a fixture, computed once and shared: (history [T][d][n], HostChains, HostMoments, modes drawn)"""
    key = (algo, which, N, n, steps)
    if key in _REF:
        return _REF[key]
    L = oracle
    src, d, yd, nd, prior, y_obs, eps, K = user_case(which)
    theta0, y0, lp_o, mix_o = start(which, n)
    model, lp = compiled_model(which).descriptor(), lp_o.descriptor()
    ref = mixture_ref.MixtureRef.from_descriptor(mix_o.descriptor())
    lib, fn = host_simulator(src, d, yd, nd)
    L.oracle_set_user_simulator(fn)
    L.oracle_set_user_model(*host_hooks(lib))
    try:
        Np = N if algo == "glmcmc" else 1
        R = Np * n
        hc = oracle_lib.HostChains(theta0, y0, chain0=CHAIN0)
        cs = hc.struct()
        hm = oracle_lib.HostMoments(n, d)
        buf = dict(theta_prop=np.zeros((R, d), np.float32), log_q=np.zeros(R, np.float32), sim_noise=np.zeros((R, nd), np.float32),
                   log_u=np.zeros(n, np.float32), u_res=np.zeros(n, np.float64), is_global=np.zeros(n, np.int32),
                   y_prop=np.zeros((R, yd), np.float32), prior_prop=np.zeros(R, np.float32), kern_prop=np.zeros(R, np.float32),
                   prior_cur=np.zeros(n, np.float32), kern_cur=np.zeros(n, np.float32), q_cur=np.zeros(n, np.float32))
        io = A.StepIO(Np, d, yd, nd, *[buf[k].ctypes.data for k in ("theta_prop", "log_q", "sim_noise", "log_u", "u_res", "is_global", "y_prop",
                                                                    "prior_prop", "kern_prop", "prior_cur", "kern_cur", "q_cur")], None)
        th0, yy0 = np.ascontiguousarray(theta0), np.ascontiguousarray(y0)
        assert L.oracle_model_prior_log_prob(C.byref(model), th0.ctypes.data, n, buf["prior_cur"].ctypes.data) == 0
        assert L.oracle_model_log_kernel(C.byref(model), yy0.ctypes.data, n, buf["kern_cur"].ctypes.data) == 0
        hist = np.zeros((steps, d, n), np.float32)
        ids = np.uint64(CHAIN0) + np.arange(n, dtype=np.uint64)
        modes_drawn = set()
        for t in range(steps):
            run, keep = oracle_lib.make_run(seed=SEED, step0=1 + t, n_steps=1, gf=GF, batch=Np, history=hist[t], moments=hm)
            assert L.oracle_propose(ALGO[algo], C.byref(lp), None, C.byref(cs), C.byref(run), C.byref(io)) == 0
            theta_c, log_q_c = ref.candidates(SEED, ids, 1 + t, Np, nd)
            for j in range(Np):
                rows = np.ones(n, bool) if j else (buf["is_global"] & 1).astype(bool)   # row 0 of a chain on the local branch is the local move
                buf["theta_prop"][j * n:(j + 1) * n][rows] = theta_c[j][rows]
                buf["log_q"][j * n:(j + 1) * n][rows] = log_q_c[j][rows]
            assert L.oracle_model_prior_log_prob(C.byref(model), buf["theta_prop"].ctypes.data, R, buf["prior_prop"].ctypes.data) == 0
            simulate_rows(L, lib, model, buf["theta_prop"], buf["sim_noise"], buf["y_prop"])
            assert L.oracle_model_log_kernel(C.byref(model), buf["y_prop"].ctypes.data, R, buf["kern_prop"].ctypes.data) == 0
            buf["q_cur"][:] = ref.log_prob_f32(hc.theta.T)
            assert L.oracle_select(ALGO[algo], None, C.byref(cs), C.byref(run), C.byref(io)) == 0
            if t < 4:
                modes_drawn |= set(np.argmin(((theta_c[:, :, None, :].astype(np.float64) - ref.loc) ** 2 / ref.scale ** 2).sum(-1), axis=-1).ravel())
    finally:
        L.oracle_set_user_model(None, None, None)
        L.oracle_set_user_simulator(None)
    for a in (hist, hc.theta, hc.y, hc.log_w, hc.flags, hc.n_moves, hm.sum_theta, hm.sum_outer, hm.sum_jump):
        a.setflags(write=False)
    _REF[key] = (hist, hc, hm, len(modes_drawn))
    return _REF[key]


def rtc_run(which, algo, N, n=N_CHAINS, steps=T, lanes=0, debug_flags=0):
    from glabcmcmc_amd import engine
    cm = compiled_model(which)
    theta0, y0, lp_o, mix_o = start(which, n)
    dev = torch.device("cuda", 0)
    chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev, chain0=CHAIN0)
    hist = torch.empty(steps, chains.d, chains.n, dtype=torch.float32, device=dev)
    mom = engine.Moments(chains.n, chains.d, dev)
    engine.run_steps(None, cm.descriptor(), lp_o.descriptor(), mix_o.descriptor(), chains, steps, 1, SEED, GF, N, history=hist, moments=mom,
                     steps_per_launch=K_LAUNCH, lanes_per_chain=lanes, debug_flags=debug_flags,
                     rtc_program=cm.program(ALGO[algo], N, mixture=True, proposal=mix_o))
    torch.cuda.synchronize()
    return hist.cpu().numpy(), chains, mom


def assert_equal_states(got, hh, theta, y, flags, log_w, n_moves, sums, what, isir):
    hist, chains, mom = got
    same = bits(hist) == bits(hh)
    assert same.all(), "%s: first mismatch at (t, dim, chain) = %s" % (what, np.argwhere(~same)[0])
    assert np.array_equal(bits(chains.theta.cpu().numpy()), bits(theta)), what
    assert np.array_equal(bits(chains.y.cpu().numpy()), bits(y)), what
    assert np.array_equal(chains.n_moves.cpu().numpy().astype(np.uint32), np.asarray(n_moves, np.uint32)), what
    if isir:
        assert np.array_equal(chains.flags.cpu().numpy().astype(np.uint32), flags), what
        clear = (flags & A.FLAG_LOCAL) == 0                                   # log_w is defined where the `local` flag is clear
        assert clear.any(), what
        assert np.array_equal(bits(chains.log_w.cpu().numpy()[clear]), bits(log_w[clear])), what
    for name, want in zip(("sum_theta", "sum_outer", "sum_jump"), sums):
        assert np.array_equal(getattr(mom, name).cpu().numpy().view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), (what, name)


def assert_equals_reference(got, want, what, isir, K):
    hh, hc, hm, modes = want
    assert np.isfinite(hh).all(), what
    assert int((hc.n_moves > 0).sum()) >= hc.n // 2, what                      # the comparison is not one of chains standing still
    assert modes == K, "%s: %d of %d modes drawn" % (what, modes, K)
    assert_equal_states(got, hh, hc.theta, hc.y, hc.flags, hc.log_w, hc.n_moves, (hm.sum_theta, hm.sum_outer, hm.sum_jump), what, isir)


# ---- CPU ------------------------------------------------------------------------------------------------------------------------
def test_fused_supported_takes_a_compiled_model_with_a_mixture():
    """building a CompiledModel needs no device"""
    import glabcmcmc_amd as g_
    src, d, yd, nd, prior, y_obs, eps, K = user_case("nonlinear")
    cm = g_.CompiledModel(d, yd, src, prior, y_obs, eps, noise_dim=nd)
    local, mix = make_dist(("gauss", [0.0] * 3, [0.3] * 3)), make_mixture(3, 3)

    def ok(model, proposals, N, **kw):
        kw.setdefault("mixture_ok", True)
        return generic.fused_supported(model, proposals, N, A.MAX_BATCH_WIDE, gamma_ok=True, mixture_max_batch=A.MAX_BATCH_WIDE, **kw)
    for N in (1, 16, 17, 4096):
        assert ok(cm, (local, mix), N) is True
    assert not ok(cm, (local, mix), 4097)
    assert ok(cm, (local, mix), 1) and generic.fused_supported(cm, (local, mix), 1, gamma_ok=True, mixture_ok=True)        # GlobalMCMC's call
    assert not generic.fused_supported(cm, (local, mix), 17, gamma_ok=True, mixture_ok=True)      # a caller without the wide entry point
    gamma_prior = distribution.Gamma(torch.full((3,), 4.0), torch.full((3,), 2.0))
    assert not ok(g_.CompiledModel(d, yd, src, gamma_prior, y_obs, eps, noise_dim=nd), (local, mix), 5)
    assert not ok(cm, (local, make_mixture(3, 2)), 5)                         # a mixture of the wrong dimension
    assert not ok(cm, (mix, local), 5) and not ok(cm, (mix, mix), 5)          # a mixture that is not the last proposal
    assert not ok(cm, (local, mix), 5, mixture_ok=False)
    src2, d2, yd2, nd2, prior2, y_obs2, eps2, _ = user_case("all_user")
    hooks = g_.CompiledModel(d2, yd2, src2, prior2, y_obs2, eps2, noise_dim=nd2)
    l2, m2 = make_dist(("gauss", [0.0] * 2, [0.3] * 2)), make_mixture(3, 2)
    assert ok(hooks, (l2, m2), 16) and not ok(hooks, (l2, m2), 17)            # a user prior above 16 proposals stays split-phase

    class Duck:                                                               # a SIM_USER descriptor without programs: callbacks
        def descriptor(self):
            return cm.descriptor()
    assert not ok(Duck(), (local, mix), 5)


def test_compile_mix_checks_its_arguments_and_needs_a_device():
    """hiprtc cross-compiles without a GPU: a valid mixture program compiles and then fails to LOAD where there is no device"""
    lib = A.lib()
    handle, log = C.c_void_p(), C.create_string_buffer(1 << 14)
    src = NONLINEAR.encode()
    assert lib.glabc_rtc_compile_mix(None, A.ALGO_GLMCMC, 3, 2, 4, 5, C.byref(handle), log, len(log)) == NULL
    assert lib.glabc_rtc_compile_mix(src, A.ALGO_GLMCMC, 3, 2, 4, 5, None, log, len(log)) == NULL
    assert lib.glabc_rtc_compile_mix(src, A.ALGO_GLMALA, 3, 2, 4, 5, C.byref(handle), log, len(log)) == KIND
    assert lib.glabc_rtc_compile_mix(src, A.ALGO_GLMCMC, 9, 2, 4, 5, C.byref(handle), log, len(log)) == DIM
    assert lib.glabc_rtc_compile_mix(src, A.ALGO_GLMCMC, 3, 2, 0, 5, C.byref(handle), log, len(log)) == DIM
    assert lib.glabc_rtc_compile_mix(src, A.ALGO_GLMCMC, 3, 2, 4, 17, C.byref(handle), log, len(log)) == ARG
    assert lib.glabc_rtc_compile_mix(src, A.ALGO_GLMCMC, 3, 2, 4, 0, C.byref(handle), log, len(log)) == ARG
    assert lib.glabc_rtc_compile_wide_mix(None, 3, 2, 4, C.byref(handle), log, len(log)) == NULL
    assert lib.glabc_rtc_compile_wide_mix(src, 3, 9, 4, C.byref(handle), log, len(log)) == DIM
    rc = lib.glabc_rtc_compile_mix(b"GLABC_SIMULATOR void glabc_user_simulate(const float* t, const float* e, float* y) { y[0] = t[0] + ; }",
                                   A.ALGO_GLMCMC, 1, 1, 1, 3, C.byref(handle), log, len(log))
    assert rc == ARG and b"error" in log.value and b"user_simulator" in log.value
    # theta_dim 8 (the candidates' proposal normals span two Philox blocks), GlobalMCMC whatever the batch size says
    for rc in (lib.glabc_rtc_compile_mix(wide_source(8, 8, 8).encode(), A.ALGO_GLMCMC, 8, 8, 8, 4, C.byref(handle), log, len(log)),
               lib.glabc_rtc_compile_mix(src, A.ALGO_GLOBALMCMC, 3, 2, 4, 99, C.byref(handle), log, len(log))):
        if torch.cuda.is_available():
            assert rc == OK, log.value.decode()
            lib.glabc_rtc_release(handle)
        else:
            assert rc == -6, log.value.decode()


# ---- GPU: same code, simulator inlined --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("algo,N", [("glmcmc", 1), ("glmcmc", 5), ("glmcmc", 16), ("globalmcmc", 1), ("glmcmc", 32)])
def test_hip_mix_program_equals_the_builtin_mixture_kernels(hip, algo, N):
    """y = |theta| + noise as user source in a mixture program against glabc_glmcmc_mix_steps / glabc_globalmcmc_mix_steps /
    glabc_glmcmc_mix_wide_steps on the built-in Model: history, theta, y, flags, n_moves, log_w where defined, the moment sums"""
    import glabcmcmc_amd as g_
    from glabcmcmc_amd import engine
    builtin = AbsGaussModel(0.4, [1.5, 1.5])
    model = builtin.descriptor()
    user = user_model_desc(model, 2)
    cm = g_.CompiledModel(2, 2, mixture_source([model.noise.p2[0], model.noise.p2[1]]), FixedPrior(model.prior), [1.5, 1.5], 0.4)
    cm.descriptor = lambda epsilon=None, _m=user: _m                            # the built-in Model's constants, to the bit
    lp, mix_o = make_dist(("gauss", [0.0] * 2, [0.35] * 2)).descriptor(), make_mixture(3, 2, spread=1.5)
    mix = mix_o.descriptor()
    rng = np.random.default_rng(11)
    theta0 = (1.5 * rng.standard_normal((N_CHAINS, 2))).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236 * rng.standard_normal((N_CHAINS, 2))).astype(np.float32)
    dev = torch.device("cuda", 0)
    out = []
    for rtc in (False, True):
        chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev, chain0=CHAIN0)
        hist = torch.empty(T, 2, N_CHAINS, dtype=torch.float32, device=dev)
        mom = engine.Moments(N_CHAINS, 2, dev)
        if rtc:
            entry, m, prog = None, user, cm.program(ALGO[algo], N, mixture=True, proposal=mix_o)
        else:
            entry = "glabc_globalmcmc_mix_steps" if algo == "globalmcmc" else "glabc_glmcmc_mix_wide_steps" if N > 16 else "glabc_glmcmc_mix_steps"
            m, prog = model, None
            if algo == "glmcmc":
                engine.init_weights(model, mix, chains)
        engine.run_steps(entry, m, lp, mix, chains, T, 1, SEED, GF, N, history=hist, moments=mom, steps_per_launch=K_LAUNCH, rtc_program=prog)
        torch.cuda.synchronize()
        out.append((hist.cpu().numpy(), chains, mom))
    (hh, c0, m0), got = out
    assert np.isfinite(hh).all() and int((c0.n_moves.cpu().numpy() > 0).sum()) >= N_CHAINS // 2
    assert_equal_states(got, hh, c0.theta.cpu().numpy(), c0.y.cpu().numpy(), c0.flags.cpu().numpy().astype(np.uint32), c0.log_w.cpu().numpy(),
                        c0.n_moves.cpu().numpy(), [getattr(m0, k).cpu().numpy() for k in ("sum_theta", "sum_outer", "sum_jump")],
                        (algo, N), algo == "glmcmc")


# ---- GPU: simulators the built-in kernels do not have -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("algo,N", [("glmcmc", 5), ("glmcmc", 12), ("glmcmc", 16), ("globalmcmc", 1)])
def test_hip_nonlinear_register_programs_equal_the_reference_chain(hip, oracle, algo, N):
    want = reference(oracle, algo, "nonlinear", N)
    assert_equals_reference(rtc_run("nonlinear", algo, N), want, (algo, N), algo == "glmcmc", 3)


@pytest.mark.gpu
@pytest.mark.parametrize("N,lanes", [(17, 0), (40, 0), (257, 0), (100, 8), (100, 16), (100, 32), (100, 64)])
def test_hip_nonlinear_wide_program_equals_the_reference_chain(hip, oracle, N, lanes):
    """the default lanes per chain at three batch sizes, every forced lane count at N = 100: one program, one reference per N"""
    want = reference(oracle, "glmcmc", "nonlinear", N, steps=20)
    assert_equals_reference(rtc_run("nonlinear", "glmcmc", N, steps=20, lanes=lanes), want, (N, lanes), True, 3)


@pytest.mark.gpu
def test_hip_nonlinear_wide_program_at_the_largest_batch(hip, oracle):
    want = reference(oracle, "glmcmc", "nonlinear", 4096, n=8, steps=3)
    hh, hc, hm, modes = want
    assert modes == 3 and np.isfinite(hh).all() and (hc.n_moves > 0).any()
    assert_equal_states(rtc_run("nonlinear", "glmcmc", 4096, n=8, steps=3), hh, hc.theta, hc.y, hc.flags, hc.log_w, hc.n_moves,
                        (hm.sum_theta, hm.sum_outer, hm.sum_jump), "N 4096", True)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [5, 32])
def test_hip_user_hooks_in_a_mix_program_equal_the_reference_chain(hip, oracle, N):
    """prior, discrepancy and kernel as user source next to the simulator: VAR_MIX is VAR_GENERIC plus the tables"""
    want = reference(oracle, "glmcmc", "all_user", N, steps=20)
    assert_equals_reference(rtc_run("all_user", "glmcmc", N, steps=20), want, N, True, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("which,N,K", [("888", 4, 3), ("111", 15, 8), ("638", 9, 3)])
def test_hip_mix_programs_at_the_shape_extremes(hip, oracle, which, N, K):
    want = reference(oracle, "glmcmc", which, N, steps=30)
    assert_equals_reference(rtc_run(which, "glmcmc", N, steps=30), want, (which, N), True, K)


@pytest.mark.gpu
def test_hip_mix_program_with_the_exact_index(hip, oracle):
    want = reference(oracle, "glmcmc", "nonlinear", 12)
    assert_equals_reference(rtc_run("nonlinear", "glmcmc", 12, debug_flags=A.DEBUG_EXACT_INDEX), want, "exact index", True, 3)


# ---- GPU: refusals ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_mix_steps_refusals_leave_the_state_untouched(hip):
    from glabcmcmc_amd import engine
    cm = compiled_model("nonlinear")
    theta0, y0, lp_o, mix_o = start("nonlinear", 65)
    model, lp, mix = cm.descriptor(), lp_o.descriptor(), mix_o.descriptor()
    gauss = make_dist(("gauss", [0.0] * 3, [1.5] * 3)).descriptor()
    dev = torch.device("cuda", 0)
    p_mix5 = cm.program(A.ALGO_GLMCMC, 5, mixture=True, proposal=mix_o)
    p_wide = cm.program(A.ALGO_GLMCMC, 40, mixture=True, proposal=mix_o)
    p_gauss = cm.program(A.ALGO_GLMCMC, 5)
    assert p_mix5.value != p_wide.value and cm.program(A.ALGO_GLMCMC, 257, mixture=True).value == p_wide.value     # one wide program per Model

    def call(fn, prog, m, glob, N, lanes=0):
        state = [torch.from_numpy(canary_f32(3, 65)).to(dev), torch.from_numpy(canary_f32(2, 65)).to(dev), torch.from_numpy(canary_f32(65)).to(dev)]
        hist = torch.from_numpy(canary_f32(4, 3, 65)).to(dev)
        chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev, chain0=CHAIN0)
        chains.theta, chains.y, chains.log_w = state
        cs = chains.struct()
        run = A.Run()
        run.seed, run.step0, run.n_steps, run.global_frequency, run.batch_size, run.lanes_per_chain = SEED, 1, 4, GF, N, lanes
        run.history, run.hist_stride = hist.data_ptr(), 65
        rc = fn(prog, C.byref(m), C.byref(lp), C.byref(glob), C.byref(cs), C.byref(run), None)
        torch.cuda.synchronize()
        for t in state + [hist]:
            assert canary_left(t.cpu().numpy()) == t.numel(), "a refused launch wrote to the chains"
        return rc
    assert call(hip.glabc_rtc_steps, p_mix5, model, gauss, 5) == KIND                       # a mixture program holds no generic kernel
    assert call(hip.glabc_rtc_steps, p_wide, model, gauss, 40) == KIND
    assert call(hip.glabc_rtc_mix_steps, p_gauss, model, mix, 5) == KIND                    # ... and the other way round
    gm = cm.descriptor()
    gm.prior = distribution.Gamma(torch.full((3,), 4.0), torch.full((3,), 2.0)).descriptor()
    assert call(hip.glabc_rtc_mix_steps, p_mix5, gm, mix, 5) == KIND                        # a Gamma prior
    assert call(hip.glabc_rtc_mix_steps, p_mix5, model, mix, 6) == ARG                      # a register program at another batch size
    assert call(hip.glabc_rtc_mix_steps, p_wide, model, mix, 5) == ARG
    assert call(hip.glabc_rtc_mix_steps, p_wide, model, mix, 4096, lanes=8) == ARG          # 4 * 32 * (4096 + 33) bytes of rows: beyond the LDS
    assert call(hip.glabc_rtc_mix_steps, p_wide, model, mix, 40, lanes=4) == ARG
    # the row kernels and the hooks take a mixture program unchanged
    hooks = [C.c_int32(-1) for _ in range(3)]
    assert hip.glabc_rtc_hooks(p_wide, *[C.byref(h) for h in hooks]) == OK and [h.value for h in hooks] == [0, 0, 0]
    th, eps = torch.from_numpy(theta0).to(dev), torch.randn(65, 4, device=dev)
    ya, yb = torch.empty(65, 2, device=dev), torch.empty(65, 2, device=dev)
    assert hip.glabc_rtc_simulate(p_mix5, th.data_ptr(), eps.data_ptr(), 65, ya.data_ptr(), None) == OK
    assert hip.glabc_rtc_simulate(p_gauss, th.data_ptr(), eps.data_ptr(), 65, yb.data_ptr(), None) == OK
    torch.cuda.synchronize()
    assert torch.equal(ya.view(torch.int32), yb.view(torch.int32))


# ---- GPU: the package -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_package_runs_a_mixture_on_a_compiled_model_fused(hip):
    """GLMCMC (register and wide program) and GlobalMCMC with path='auto': the fused path (no callback_device in state_out), the chains
    of the direct glabc_rtc_mix_steps call on the same seed; path='generic' still runs; one chain keeps the reference's shape"""
    import glabcmcmc_amd as g_
    from glabcmcmc_amd import engine
    cm = compiled_model("nonlinear")
    n, steps = 64, 12
    theta0, y0, lp, mix = start("nonlinear", n)
    t0, yy0 = torch.from_numpy(theta0), torch.from_numpy(y0)
    dev = torch.device("cuda", 0)
    for algo, N in (("glmcmc", 6), ("glmcmc", 40), ("globalmcmc", 1)):
        state = {}
        kw = dict(seed=SEED, chain0=CHAIN0, verbose=False, state_out=state)
        if algo == "glmcmc":
            got = g_.GLMCMC(cm, steps, t0, yy0, lp, None, GF, mix, N, **kw)
            same = g_.GLMCMC(cm, steps, t0, yy0, lp, None, GF, mix, N, path="fused", seed=SEED, chain0=CHAIN0, verbose=False)
        else:
            got = g_.GlobalMCMC(cm, steps, t0, yy0, mix, None, GF, lp, **kw)
            same = g_.GlobalMCMC(cm, steps, t0, yy0, mix, None, GF, lp, path="fused", seed=SEED, chain0=CHAIN0, verbose=False)
        assert "callback_device" not in state and "chains" in state, (algo, N)
        assert got.shape == (steps, n, 3) and np.array_equal(bits(got.numpy()), bits(same.numpy()))
        chains = engine.ChainBatch(t0, yy0, dev, chain0=CHAIN0)
        hist = torch.empty(steps - 1, 3, n, dtype=torch.float32, device=dev)
        engine.run_steps(None, cm.descriptor(), lp.descriptor(), mix.descriptor(), chains, steps - 1, 1, SEED, GF, N, history=hist,
                         rtc_program=cm.program(ALGO[algo], N, mixture=True, proposal=mix))
        torch.cuda.synchronize()
        assert np.array_equal(bits(got[1:].numpy()), bits(hist.permute(0, 2, 1).cpu().numpy())), (algo, N)
        assert (got[-1] != got[0]).any() and torch.isfinite(got).all()
    g = g_.GLMCMC(cm, steps, t0, yy0, lp, None, GF, mix, 6, path="generic", seed=SEED, verbose=False)
    assert g.shape == (steps, n, 3) and torch.isfinite(g).all() and (g[-1] != g[0]).any()
    one = g_.GLMCMC(cm, 20, t0[0], yy0[0], lp, None, GF, mix, 6, seed=SEED, verbose=False)
    assert one.shape == (20, 3) and one.dtype == torch.float32 and not one.is_cuda and torch.isfinite(one).all()
    with pytest.raises(ValueError):
        g_.GLMCMC(cm, 5, t0, yy0, lp, None, GF, mix, 6, seed=SEED, verbose=False, fast_math=True)
