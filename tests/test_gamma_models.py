"""Gamma priors and proposals inside the fused kernels on the g-and-k Model and on run-time compiled Models.

GLABC_DIST_GAMMA is the one distribution with positive support; g-and-k (A, B, g, k > 0) and a user's simulator with rates and
scales are the Models that need it.  The CPU tests hold the fixtures (the checker alone moves the chains), the dispatch
(generic.fused_supported), the C ABI's argument checks and the run-time compiler's new entry points; the GPU tests hold every
new kernel instantiation to the CPU checker bit for bit -- history, theta, y, log_w, flags, n_moves and the three moment sums.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import oracle_lib
from helpers import AbsGaussModel, bits, make_dist
from test_rtc import NONLINEAR, host_simulator
from glabcmcmc_amd import _capi as A

N_CHAINS, T, SEED = 96, 60, 11                  # one full wavefront and half of one
CHAIN0 = 2 ** 32 + 7                            # the high counter word is live
K_LAUNCH = 13                                   # launches cut at an odd number of iterations

# ---- g-and-k -------------------------------------------------------------------------------------------------------------
GK_PRIOR = ("gamma", [3.0, 2.0, 2.0, 1.5], [1.0, 2.0, 1.0, 3.0])
GK_PROP = ("gamma", [9.0, 4.0, 4.0, 2.0], [3.0, 4.0, 2.0, 4.0])
GK_BOOST = ("gamma", [9.0, 0.7, 4.0, 2.0], [3.0, 1.0, 2.0, 4.0])         # a shape below 1: the boost draw
GK_UNIFORM = ("uniform", [0.0] * 4, [10.0] * 4)
GK_MIXES = {"gamma-gamma": (GK_PRIOR, GK_PROP), "gamma-uniform": (GK_PRIOR, GK_UNIFORM), "uniform-gamma": (None, GK_PROP),
            "gamma-boost": (GK_PRIOR, GK_BOOST)}

# ---- a user's simulator: theta[2], eps[3] -> y[3] ---------------------------------------------------------------------------
USER_SRC = """
GLABC_SIMULATOR void glabc_user_simulate(const float* theta, const float* eps, float* y)
{
    y[0] = theta[1] / (theta[0] + 0.5f) + 0.2f*eps[0];
    y[1] = sqrtf(fabsf(theta[0]*theta[1])) + 0.2f*eps[1];
    y[2] = glabc_logf(1.0f + theta[0]*theta[0]) * glabc_expf(0.1f*eps[2]);
}
"""
USER_Y_OBS, USER_EPS = [1.0, 1.5, 1.2], 0.4
USER_GAMMA_PRIOR, USER_GAUSS = ("gamma", [2.0, 3.0], [1.0, 2.0]), ("gauss", [1.5, 1.5], [1.0, 1.0])
USER_GAMMA_PROP = ("gamma", [4.0, 4.0], [2.5, 2.5])
USER_MIXES = {"gamma-gamma": (USER_GAMMA_PRIOR, USER_GAMMA_PROP), "gamma-gauss": (USER_GAMMA_PRIOR, USER_GAUSS),
              "gauss-gamma": (USER_GAUSS, USER_GAMMA_PROP), "gauss-gauss": (USER_GAUSS, USER_GAUSS)}


def gk_set(prior):
    from glabcmcmc_amd.examples.GK import GK_set
    return GK_set(1.0, prior=None if prior is None else make_dist(prior))


def gk_case(mix):
    """(model, local, proposal) descriptors and the start states of the g-and-k fixture"""
    prior, prop = GK_MIXES[mix]
    rng = np.random.default_rng(5)
    theta0 = (np.array([3.0, 1.0, 2.0, 0.5]) * np.exp(0.2 * rng.standard_normal((N_CHAINS, 4)))).astype(np.float32)
    y0 = np.sort(3.0 + 2.0 * rng.standard_normal((N_CHAINS, 8)), axis=1).astype(np.float32)
    return gk_set(prior).descriptor(), make_dist(("gauss", [0.0] * 4, [0.15] * 4)).descriptor(), make_dist(prop).descriptor(), theta0, y0


_HOST_SIM = []


def user_host():
    """the user source through gcc (once): the library and the function pointer the checker calls"""
    if not _HOST_SIM:
        _HOST_SIM.append(host_simulator(USER_SRC, 2, 3, 3))
    return _HOST_SIM[0]


def user_set(prior):
    import glabcmcmc_amd as g_
    return g_.CompiledModel(2, 3, USER_SRC, make_dist(prior), USER_Y_OBS, USER_EPS, noise_dim=3)


def user_case(mix):
    prior, prop = USER_MIXES[mix]
    lib, _ = user_host()
    rng = np.random.default_rng(5)
    theta0 = (np.abs(rng.standard_normal((N_CHAINS, 2))) + 0.5).astype(np.float32)
    eps = rng.standard_normal((N_CHAINS, 3)).astype(np.float32)
    y0 = np.empty((N_CHAINS, 3), np.float32)
    for r in range(N_CHAINS):
        lib.glabc_user_simulate_host(theta0[r].ctypes.data_as(C.c_void_p), eps[r].ctypes.data_as(C.c_void_p), y0[r].ctypes.data_as(C.c_void_p))
    return user_set(prior).descriptor(), make_dist(("gauss", [0.0] * 2, [0.3] * 2)).descriptor(), make_dist(prop).descriptor(), theta0, y0


_CHECKER = {}


def checker(oracle, which, mix, algo, N):
    """The CPU checker's run of a fixture, computed once and shared: (history, chains, moments, gamma prior?)"""
    key = (which, mix, algo, N)
    if key not in _CHECKER:
        model, local, prop, theta0, y0 = gk_case(mix) if which == "gk" else user_case(mix)
        if which == "user":
            oracle.oracle_set_user_simulator(user_host()[1])
            oracle.oracle_set_user_model(None, None, None)
        d = theta0.shape[1]
        hc = oracle_lib.HostChains(theta0, y0, chain0=CHAIN0)
        hh = np.zeros((T, d, N_CHAINS), np.float32)
        hm = oracle_lib.HostMoments(N_CHAINS, d)
        gf = 0.8 if algo == "glmcmc" else 0.5
        run, keep = oracle_lib.make_run(seed=SEED, step0=1, n_steps=T, gf=gf, batch=N, history=hh, moments=hm)
        cs = hc.struct()
        if algo == "glmcmc":
            if which == "gk":                   # a run-time compiled Model computes log_w at its first global move
                assert oracle.oracle_init_weights(C.byref(model), C.byref(prop), C.byref(cs)) == 0
            rc = oracle.oracle_glmcmc_steps(C.byref(model), C.byref(local), C.byref(prop), C.byref(cs), C.byref(run))
        else:
            rc = oracle.oracle_globalmcmc_steps(C.byref(model), C.byref(local), C.byref(prop), C.byref(cs), C.byref(run))
        assert rc == 0, key
        for a in (hh, hc.theta, hc.y, hc.log_w, hm.sum_theta, hm.sum_outer, hm.sum_jump):
            a.setflags(write=False)
        _CHECKER[key] = (hh, hc, hm, model.prior.kind == A.DIST_GAMMA)
    return _CHECKER[key]


def assert_fixture_moves(res, key):
    """at least three quarters of the chains have moved, every recorded state is finite, and under a Gamma prior no state
    outside its support is left from the midpoint on"""
    hh, hc, hm, gamma_prior = res
    assert int((hc.n_moves > 0).sum()) >= (3 * N_CHAINS) // 4, key
    assert np.isfinite(hh).all() and np.isfinite(hc.y).all(), key
    if gamma_prior:
        assert (hh[T // 2:] >= 0).all(), key


# ============================================================================================================ CPU
GK_CPU = [(m, "glmcmc", n) for m in ("gamma-gamma",) for n in (5, 16, 40)] + [("gamma-gamma", "globalmcmc", 1)] + \
         [(m, "glmcmc", 5) for m in ("gamma-uniform", "uniform-gamma", "gamma-boost")]
USER_CPU = [(m, "glmcmc", n) for m in ("gamma-gamma", "gamma-gauss", "gauss-gamma") for n in (1, 5, 12, 16, 17, 100)] + \
           [(m, "globalmcmc", 1) for m in ("gamma-gamma", "gamma-gauss", "gauss-gamma")]


@pytest.mark.parametrize("mix,algo,N", GK_CPU)
def test_checker_moves_the_gk_fixture(oracle, mix, algo, N):
    assert_fixture_moves(checker(oracle, "gk", mix, algo, N), (mix, algo, N))


@pytest.mark.parametrize("mix,algo,N", USER_CPU)
def test_checker_moves_the_user_fixture(oracle, mix, algo, N):
    assert_fixture_moves(checker(oracle, "user", mix, algo, N), (mix, algo, N))


def test_dispatch_takes_gamma_on_gk_and_compiled_models():
    from glabcmcmc_amd import generic
    local, gamma = make_dist(("gauss", [0.0] * 4, [0.15] * 4)), make_dist(GK_PROP)
    for model in (gk_set(GK_PRIOR), gk_set(None)):
        for N in (1, 16, 17, 4096):
            assert generic.fused_supported(model, (local, gamma), N, A.MAX_BATCH_WIDE, gamma_ok=True), N
            assert not generic.fused_supported(model, (local, gamma), N, A.MAX_BATCH_WIDE), N
            assert not generic.fused_supported(model, (gamma, gamma), N, A.MAX_BATCH_WIDE, gamma_ok=True), N     # a Gamma local increment
        assert not generic.fused_supported(model, (local, gamma), 4097, A.MAX_BATCH_WIDE, gamma_ok=True)
        assert generic.fused_supported(model, (local, gamma), 1, gamma_ok=True)                                  # GlobalMCMC
    assert gk_set(GK_PRIOR).descriptor().prior.kind == A.DIST_GAMMA and gk_set(None).descriptor().prior.kind == A.DIST_UNIFORM
    assert torch.equal(gk_set(GK_PRIOR).prior_log_prob(torch.tensor([[1.0, 1.0, 1.0, 1.0]])),
                       make_dist(GK_PRIOR).log_prob(torch.tensor([[1.0, 1.0, 1.0, 1.0]])))                        # _prior() on CPU tensors
    local, gamma = make_dist(("gauss", [0.0] * 2, [0.3] * 2)), make_dist(USER_GAMMA_PROP)
    for prior in (USER_GAMMA_PRIOR, USER_GAUSS):
        cm = user_set(prior)
        for N in (1, 16, 17, 4096):
            assert generic.fused_supported(cm, (local, gamma), N, A.MAX_BATCH_WIDE, gamma_ok=True), N
            assert not generic.fused_supported(cm, (local, gamma), N, A.MAX_BATCH_WIDE), N
            assert not generic.fused_supported(cm, (gamma, gamma), N, A.MAX_BATCH_WIDE, gamma_ok=True), N
    cm = user_set(USER_GAMMA_PRIOR)
    cm.user_prior = True                        # the existing rule: a user prior stays split-phase above 16 proposals
    assert generic.fused_supported(cm, (local, gamma), 16, A.MAX_BATCH_WIDE, gamma_ok=True)
    assert not generic.fused_supported(cm, (local, gamma), 17, A.MAX_BATCH_WIDE, gamma_ok=True)
    # what stays split-phase: theta_dim 5 on the |theta| + noise Model
    m5 = AbsGaussModel(0.3, [1.5] * 5)
    g5 = make_dist(("gamma", [4.0] * 5, [3.0] * 5))
    assert not generic.fused_supported(m5, (make_dist(("gauss", [0.0] * 5, [0.3] * 5)), g5), 5, A.MAX_BATCH_WIDE, gamma_ok=True)


def _host_call(hip, entry, model, local, prop, N=5, math_mode=0, d=4, yd=8):
    """the entry point with host arrays for the pointers and no chains: every argument check, no launch"""
    theta, y = np.zeros((d, 1), np.float32), np.zeros((yd, 1), np.float32)
    log_w, flags, n_moves = np.zeros(1, np.float32), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    cs = A.Chains(0, CHAIN0, 0, theta.ctypes.data, y.ctypes.data, log_w.ctypes.data, flags.ctypes.data, n_moves.ctypes.data)
    run = A.Run()
    run.seed, run.step0, run.n_steps, run.global_frequency, run.batch_size, run.math_mode = SEED, 1, T, 0.8, N, math_mode
    return getattr(hip, entry)(C.byref(model), C.byref(local), C.byref(prop), C.byref(cs), C.byref(run), None)


def test_abi_admits_gamma_on_gk_without_a_device(hip):
    for entry in ("glabc_glmcmc_steps", "glabc_globalmcmc_steps"):
        for mix in ("gamma-gamma", "gamma-uniform", "uniform-gamma"):
            model, local, prop, _, _ = gk_case(mix)
            for N in (1, 5, 16, 17, 4096):
                assert _host_call(hip, entry, model, local, prop, N) == 0, (entry, mix, N)
        model, local, prop, _, _ = gk_case("gamma-gamma")
        assert _host_call(hip, entry, model, prop, prop) == -3                                  # a Gamma local increment
        assert _host_call(hip, entry, model, local, prop, math_mode=A.MATH_FAST) == -4
        m5 = AbsGaussModel(0.3, [1.5] * 5).descriptor()
        g5, l5 = make_dist(("gamma", [4.0] * 5, [3.0] * 5)).descriptor(), make_dist(("gauss", [0.0] * 5, [0.3] * 5)).descriptor()
        assert _host_call(hip, entry, m5, l5, g5, d=5, yd=5) == -3                              # theta_dim 5..8 with a Gamma
        assert _host_call(hip, entry, m5, l5, l5, d=5, yd=5) == 0
    # GLMALA still refuses the g-and-k Model
    model, local, prop, _, _ = gk_case("uniform-gamma")
    arr = [np.zeros((8, 1), np.float64) for _ in range(4)]
    theta, y, flags = np.zeros((4, 1), np.float32), np.zeros((8, 1), np.float32), np.zeros(1, np.uint32)
    cs = A.Chains(0, 0, 0, theta.ctypes.data, y.ctypes.data, None, flags.ctypes.data, None, *[a.ctypes.data for a in arr])
    run = A.Run()
    run.n_steps, run.batch_size = 1, 5
    mala = A.Mala(0.3, 0.09, 1.0, 100, 0)
    uni = make_dist(GK_UNIFORM).descriptor()
    assert hip.glabc_glmala_steps(C.byref(model), C.byref(uni), C.byref(mala), C.byref(cs), C.byref(run), None) == -3


def test_rtc_gamma_entry_points_without_a_device(hip, tmp_path, monkeypatch):
    """hiprtc cross-compiles without a GPU: a Gamma program compiles and then fails to LOAD where there is no device; the
    translation unit (GLABC_RTC_DUMP) asks for the Gamma teams that fit: three and two wavefronts at N = 5, two at 12, none at 16"""
    want = 0 if torch.cuda.is_available() else -6
    src = USER_SRC.encode()
    handle, log = C.c_void_p(), C.create_string_buffer(1 << 14)

    def done(rc):
        assert rc == want, log.value.decode()
        if rc == 0:
            hip.glabc_rtc_release(handle)

    dump = tmp_path / "unit.hip"
    monkeypatch.setenv("GLABC_RTC_DUMP", str(dump))
    monkeypatch.setenv("GLABC_RTC_LANES", "1")                    # one compile per program
    for N, flags, teams in ((5, A.RTC_GAMMA, (True, True)), (12, A.RTC_GAMMA, (False, True)), (16, A.RTC_GAMMA, (False, False)),
                            (5, 0, (False, False))):
        done(hip.glabc_rtc_compile_ex(src, A.ALGO_GLMCMC, 2, 3, 3, N, flags, C.byref(handle), log, len(log)))
        unit = dump.read_text()
        assert ("#define GLABC_RTC_WITH_GAMMA 1" in unit) == bool(flags), N
        assert ("#define GLABC_RTC_GAMMA_TEAM3 1" in unit, "#define GLABC_RTC_GAMMA_TEAM2 1" in unit) == teams, N
    monkeypatch.delenv("GLABC_RTC_DUMP")
    monkeypatch.delenv("GLABC_RTC_LANES")

    done(hip.glabc_rtc_compile_ex(src, A.ALGO_GLMCMC, 2, 3, 3, 5, A.RTC_GAMMA, C.byref(handle), log, len(log)))
    done(hip.glabc_rtc_compile_ex(src, A.ALGO_GLOBALMCMC, 2, 3, 3, 1, A.RTC_GAMMA, C.byref(handle), log, len(log)))
    done(hip.glabc_rtc_compile_wide_ex(src, 2, 3, 3, A.RTC_GAMMA, C.byref(handle), log, len(log)))
    done(hip.glabc_rtc_compile_ex(src, A.ALGO_GLMCMC, 2, 3, 3, 5, 0, C.byref(handle), log, len(log)))
    assert hip.glabc_rtc_compile_ex(src, A.ALGO_GLMCMC, 2, 3, 3, 5, 2, C.byref(handle), log, len(log)) == -4
    assert hip.glabc_rtc_compile_ex(src, A.ALGO_GLMCMC, 2, 3, 3, 5, 3, C.byref(handle), log, len(log)) == -4
    assert hip.glabc_rtc_compile_wide_ex(src, 2, 3, 3, 2, C.byref(handle), log, len(log)) == -4
    assert hip.glabc_rtc_compile_ex(src, A.ALGO_GLMCMC, 2, 3, 3, 17, A.RTC_GAMMA, C.byref(handle), log, len(log)) == -4
    assert hip.glabc_rtc_compile_ex(src, A.ALGO_GLMCMC, 9, 3, 3, 5, A.RTC_GAMMA, C.byref(handle), log, len(log)) == -2
    assert hip.glabc_rtc_compile_wide_ex(None, 2, 3, 3, A.RTC_GAMMA, C.byref(handle), log, len(log)) == -1
    # the entry points without flags: what tests/test_rtc.py::test_compile_reports_errors_and_needs_a_device expects
    done(hip.glabc_rtc_compile(NONLINEAR.encode(), A.ALGO_GLMCMC, 3, 2, 4, 5, C.byref(handle), log, len(log)))
    assert hip.glabc_rtc_compile(NONLINEAR.encode(), A.ALGO_GLMCMC, 3, 2, 4, 17, C.byref(handle), log, len(log)) == -4
    assert hip.glabc_rtc_compile(NONLINEAR.encode(), A.ALGO_GLMCMC, 9, 2, 4, 5, C.byref(handle), log, len(log)) == -2
    assert hip.glabc_rtc_compile(None, A.ALGO_GLMCMC, 3, 2, 4, 5, C.byref(handle), log, len(log)) == -1


# ============================================================================================================ GPU
def device_run(which, mix, algo, N, lanes=0, debug_flags=0, program=None):
    from glabcmcmc_amd import engine
    model, local, prop, theta0, y0 = gk_case(mix) if which == "gk" else user_case(mix)
    dev = torch.device("cuda", 0)
    chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev, chain0=CHAIN0)
    if which == "gk" and algo == "glmcmc":
        engine.init_weights(model, prop, chains)
    hist = torch.empty(T, chains.d, chains.n, dtype=torch.float32, device=dev)
    mom = engine.Moments(chains.n, chains.d, dev)
    entry = "glabc_glmcmc_steps" if algo == "glmcmc" else "glabc_globalmcmc_steps"
    engine.run_steps(entry, model, local, prop, chains, T, 1, SEED, 0.8 if algo == "glmcmc" else 0.5, N, history=hist, moments=mom,
                     steps_per_launch=K_LAUNCH, lanes_per_chain=lanes, debug_flags=debug_flags, rtc_program=program)
    torch.cuda.synchronize()
    return hist.cpu().numpy(), chains, mom


def assert_equals_checker(got, want, what):
    hist, chains, mom = got
    hh, hc, hm, _ = want
    same = bits(hist) == bits(hh)
    assert same.all(), "%s: first mismatch at (t, dim, chain) = %s" % (what, np.argwhere(~same)[0])
    assert np.array_equal(bits(chains.theta.cpu().numpy()), bits(hc.theta)), what
    assert np.array_equal(bits(chains.y.cpu().numpy()), bits(hc.y)), what
    assert np.array_equal(bits(chains.log_w.cpu().numpy()), bits(hc.log_w)), what
    assert np.array_equal(chains.flags.cpu().numpy().astype(np.uint32), hc.flags), what
    assert np.array_equal(chains.n_moves.cpu().numpy().astype(np.uint32), hc.n_moves), what
    for name in ("sum_theta", "sum_outer", "sum_jump"):
        assert np.array_equal(getattr(mom, name).cpu().numpy().view(np.uint64), getattr(hm, name).view(np.uint64)), (what, name)


GK_ONE_LANE = [("gamma-gamma", "glmcmc", n) for n in range(1, 17)] + [("gamma-gamma", "globalmcmc", 1)] + \
              [(m, "glmcmc", 5) for m in ("gamma-uniform", "uniform-gamma", "gamma-boost")]


@pytest.mark.gpu
@pytest.mark.parametrize("mix,algo,N", GK_ONE_LANE)
def test_hip_gk_gamma_one_lane(hip, oracle, mix, algo, N):
    """sampler_kernel<.., 4, 8, N, 1, VAR_GAMMA> at every batch size and in GlobalMCMC"""
    want = checker(oracle, "gk", mix, algo, N)
    assert_fixture_moves(want, (mix, algo, N))
    assert_equals_checker(device_run("gk", mix, algo, N, debug_flags=A.DEBUG_NO_TEAM), want, (mix, algo, N))
    if algo == "globalmcmc":                    # GLABC_DEBUG_TEAM: still one lane per chain, the plan sends no Gamma to the global team
        assert_equals_checker(device_run("gk", mix, algo, N, debug_flags=A.DEBUG_TEAM), want, "under TEAM")


@pytest.mark.gpu
@pytest.mark.parametrize("waves,N", [(2, n) for n in range(2, 10)] + [(3, n) for n in range(3, 8)] + [(3, 12)])
def test_hip_gk_gamma_teams(hip, oracle, waves, N):
    """team_sampler_kernel<4, 8, N, VAR_GAMMA, 2 | 3>; at N = 12 no team fits and the plan falls through to one lane"""
    want = checker(oracle, "gk", "gamma-gamma", "glmcmc", N)
    os.environ["GLABC_TEAM_WAVES"] = str(waves)
    try:
        got = device_run("gk", "gamma-gamma", "glmcmc", N, debug_flags=A.DEBUG_TEAM)
    finally:
        del os.environ["GLABC_TEAM_WAVES"]
    assert_equals_checker(got, want, (waves, N))


@pytest.mark.gpu
@pytest.mark.parametrize("N,lanes", [(17, 8), (40, 16), (100, 32), (300, 64), (40, 0), (300, 8), (17, 64)])
def test_hip_gk_gamma_lane_groups(hip, oracle, N, lanes):
    """wide_kernel<4, 8, L, true>"""
    want = checker(oracle, "gk", "gamma-gamma", "glmcmc", N)
    assert_fixture_moves(want, N)
    assert_equals_checker(device_run("gk", "gamma-gamma", "glmcmc", N, lanes=lanes), want, (N, lanes))


def _package_runs(fn, model, args, d, case):
    """the sampler on a fixture through path='fused' and path='generic': equal histories and jump sums; the fused history"""
    from glabcmcmc_amd import engine
    theta0, y0 = case[3], case[4]
    outs = []
    for path in ("fused", "generic"):
        mom = engine.Moments(N_CHAINS, d, torch.device("cuda", 0))
        extra = dict(steps_per_launch=K_LAUNCH) if path == "fused" else {}
        h = fn(model, T + 1, torch.from_numpy(theta0), torch.from_numpy(y0), *args, seed=SEED, chain0=CHAIN0, stats=mom,
               return_device=True, verbose=False, path=path, **extra)
        outs.append((h.cpu().numpy(), mom.sum_jump.cpu().numpy()))
    assert np.array_equal(bits(outs[0][0]), bits(outs[1][0])), fn.__name__
    assert np.array_equal(outs[0][1].view(np.uint64), outs[1][1].view(np.uint64)), fn.__name__
    assert (np.diff(outs[0][0], axis=0) != 0).any(-1).mean() > 0.02
    return outs[0][0]


@pytest.mark.gpu
def test_hip_gk_gamma_through_the_package(hip, oracle):
    """GLMCMC / GlobalMCMC on GK_set(prior=Gamma): the fused kernels equal the split-phase path, and the checker"""
    import glabcmcmc_amd as g_
    from glabcmcmc_amd import generic
    model = gk_set(GK_PRIOR)
    lp, ip = make_dist(("gauss", [0.0] * 4, [0.15] * 4)), make_dist(GK_PROP)
    case = gk_case("gamma-gamma")
    for fn, args, algo, N in ((g_.GLMCMC, (lp, None, 0.8, ip, 5), "glmcmc", 5), (g_.GlobalMCMC, (ip, None, 0.5, lp), "globalmcmc", 1)):
        h = _package_runs(fn, model, args, 4, case=case)
        assert np.array_equal(bits(h[1:].transpose(0, 2, 1)), bits(checker(oracle, "gk", "gamma-gamma", algo, N)[0])), algo
        assert generic.fused_supported(model, (lp, ip), N, A.MAX_BATCH_WIDE, gamma_ok=True)
        with pytest.raises(TypeError):          # `auto` is the fused kernel: it takes no keyword of the split-phase path
            fn(model, 3, torch.from_numpy(case[3]), torch.from_numpy(case[4]), *args, seed=SEED, verbose=False, callback_device="cuda")


_PROGRAMS = {}


def rtc_program(hip, algo, N, flags):
    """a register (N <= 16) or wide program of the user source, compiled once per module through the C ABI"""
    key = (algo, "wide" if N > 16 else N, flags)
    if key not in _PROGRAMS:
        handle, log = C.c_void_p(), C.create_string_buffer(1 << 16)
        src = USER_SRC.encode()
        if N > 16:
            rc = hip.glabc_rtc_compile_wide_ex(src, 2, 3, 3, flags, C.byref(handle), log, len(log))
        else:
            rc = hip.glabc_rtc_compile_ex(src, A.ALGO_GLMCMC if algo == "glmcmc" else A.ALGO_GLOBALMCMC, 2, 3, 3, N, flags, C.byref(handle),
                                          log, len(log))
        assert rc == 0, log.value.decode()
        _PROGRAMS[key] = (handle, log.value.decode())
    return _PROGRAMS[key][0]


@pytest.mark.gpu
@pytest.mark.parametrize("algo,N", [("glmcmc", 1), ("glmcmc", 5), ("glmcmc", 12), ("glmcmc", 16), ("globalmcmc", 1)])
def test_hip_rtc_gamma_register_programs(hip, oracle, algo, N):
    """a GLABC_RTC_GAMMA program: the Gamma entry (one lane) and its teams -- three wavefronts at N = 5, two at N = 12, none at
    N = 16 -- for the three prior / proposal mixes, and the generic kernels of the same program with Gaussian descriptors"""
    prog = rtc_program(hip, algo, N, A.RTC_GAMMA)
    for mix in ("gamma-gamma", "gamma-gauss", "gauss-gamma", "gauss-gauss"):
        want = checker(oracle, "user", mix, algo, N)
        assert_fixture_moves(want, (mix, algo, N))
        for flags in (A.DEBUG_NO_TEAM, A.DEBUG_TEAM):
            assert_equals_checker(device_run("user", mix, algo, N, debug_flags=flags, program=prog), want, (mix, algo, N, flags))


@pytest.mark.gpu
def test_hip_rtc_program_without_the_flag_refuses_gamma(hip):
    prog = rtc_program(hip, "glmcmc", 5, 0)
    for mix in ("gamma-gamma", "gamma-gauss", "gauss-gamma"):
        with pytest.raises(RuntimeError, match="status -4"):
            device_run("user", mix, "glmcmc", 5, program=prog)
    device_run("user", "gauss-gauss", "glmcmc", 5, program=prog)


@pytest.mark.gpu
@pytest.mark.parametrize("N,lanes,mix", [(17, 8, "gamma-gamma"), (17, 64, "gauss-gamma"), (100, 16, "gamma-gamma"), (100, 0, "gamma-gauss"),
                                         (300, 32, "gamma-gamma"), (300, 64, "gamma-gamma"), (100, 16, "gauss-gauss")])
def test_hip_rtc_gamma_wide_program(hip, oracle, N, lanes, mix):
    """wide_kernel<2, 3, L, true> of a GLABC_RTC_GAMMA wide program (and <.., false> of the same program)"""
    prog = rtc_program(hip, "glmcmc", N, A.RTC_GAMMA)
    want = checker(oracle, "user", mix, "glmcmc", N)
    assert_fixture_moves(want, (mix, N))
    assert_equals_checker(device_run("user", mix, "glmcmc", N, lanes=lanes, program=prog), want, (mix, N, lanes))


@pytest.mark.gpu
@pytest.mark.parametrize("mix", ["gamma-gamma", "gauss-gamma"])
def test_hip_compiled_model_gamma_through_the_package(hip, oracle, mix):
    """CompiledModel with a Gamma in play: GLMCMC / GlobalMCMC fused == split-phase == the checker; the Gamma program was
    self-checked; `auto` is the fused kernel"""
    import glabcmcmc_amd as g_
    from glabcmcmc_amd import generic
    prior, prop = USER_MIXES[mix]
    cm = user_set(prior)
    lp, ip = make_dist(("gauss", [0.0] * 2, [0.3] * 2)), make_dist(prop)
    case = user_case(mix)
    runs = [(g_.GLMCMC, (lp, None, 0.8, ip, 5), "glmcmc", 5)]
    if mix == "gamma-gamma":
        runs += [(g_.GLMCMC, (lp, None, 0.8, ip, 40), "glmcmc", 40), (g_.GlobalMCMC, (ip, None, 0.5, lp), "globalmcmc", 1)]
    for fn, args, algo, N in runs:
        h = _package_runs(fn, cm, args, 2, case=case)
        if N != 40:
            assert np.array_equal(bits(h[1:].transpose(0, 2, 1)), bits(checker(oracle, "user", mix, algo, N)[0])), algo
        a = A.ALGO_GLMCMC if algo == "glmcmc" else A.ALGO_GLOBALMCMC
        assert (a, N, cm.GAMMA) in cm._checked and (a, cm.WIDE if N > 16 else N, cm.GAMMA) in cm._programs
        assert generic.fused_supported(cm, (lp, ip), N, A.MAX_BATCH_WIDE, gamma_ok=True)
        with pytest.raises(TypeError):
            fn(cm, 3, torch.from_numpy(case[3]), torch.from_numpy(case[4]), *args, seed=SEED, verbose=False, callback_device="cuda")
