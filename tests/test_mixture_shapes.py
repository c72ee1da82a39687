"""The GaussianMixture kernels (glabc_mixture, include/glabc.h) against the numpy restatement of tests/mixture_ref.py, bit for bit.

Row-wise: glabc_mixture_log_prob / glabc_mixture_forward at every dimension.  Samplers: glabc_glmcmc_mix_steps /
glabc_globalmcmc_mix_steps (every instantiation of the VAR_MIX kernels) against a split-phase reference chain built the
way tests/test_generic_path.py builds one, per iteration
    oracle_propose(algo, local, NULL) -> the restatement fills the global candidates' theta_prop / log_q ->
    oracle_model_simulate on sim_noise -> oracle_model_prior_log_prob / oracle_model_log_kernel ->
    q_cur = (float) log_prob((double) theta_old) from the restatement -> oracle_select(algo, NULL)
so the checker moves the chains and only the mixture's numbers come from the restatement.  Compared: the history, the final
theta, y, flags and n_moves, log_w where the reference defines it (chains whose `local` flag is clear: GLMCMC.py:60-64
recomputes it otherwise), and the three moment sums.  Package level: MCMCRunner with a GaussianMixture equals the direct C
calls; path="generic" still runs; one chain keeps the reference's shapes.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mixture_ref
import oracle_lib
from helpers import AbsGaussModel, bits, make_dist
from test_mixture_host import make_mixture
from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import distribution

SEED, CHAIN0, GF = 11, 2 ** 32 + 7, 0.6              # the high counter word is live
N_CHAINS, T, K_LAUNCH = 96, 60, 13                    # one full and one half-filled wavefront; launches cut every 13
N_SMALL, T_SMALL = 65, 8                              # the every-instantiation sweep
ALGO = {"glmcmc": A.ALGO_GLMCMC, "globalmcmc": A.ALGO_GLOBALMCMC}


# ---- fixtures -------------------------------------------------------------------------------------------------------------
def gk_mixture(K):
    """modes around the g-and-k fixture's true parameters (3, 1, 2, 0.5), apart enough that each is drawn"""
    rng = np.random.default_rng(40 + K)
    loc = np.array([3.0, 1.0, 2.0, 0.5]) + 0.6 * rng.standard_normal((K, 4)) * np.array([1.0, 0.4, 0.8, 0.2])
    return distribution.GaussianMixture(K, 4, loc=loc, scale=0.15 + 0.2 * rng.random((K, 4)), weights=0.5 + rng.random(K))


def case(kind, d, K, local="gauss", prior="gauss", n=N_CHAINS):
    """(model object, local object, mixture object, theta0, y0)"""
    rng = np.random.default_rng(5 + d)
    if kind == "gk":
        from glabcmcmc_amd.examples.GK import GK_set
        model, mix = GK_set(1.0), gk_mixture(K)
        theta0 = (np.array([3.0, 1.0, 2.0, 0.5]) * np.exp(0.2 * rng.standard_normal((n, 4)))).astype(np.float32)
        y0 = np.sort(3.0 + 2.0 * rng.standard_normal((n, 8)), axis=1).astype(np.float32)
        lp = make_dist(("gauss", [0.0] * 4, [0.15] * 4))
        return model, lp, mix, theta0, y0
    model = AbsGaussModel(0.4, [1.5] * d)
    if prior == "uniform":
        model._prior = lambda: make_dist(("uniform", [-6.0] * d, [6.0] * d))
    # spread 1.5: centres at -1.5 / 0 / 1.5 per coordinate, among them the posterior's modes |theta| = 1.5
    mix = make_mixture(K, d, spread=1.5)
    lp = make_dist(("uniform", [-0.5] * d, [0.5] * d)) if local == "uniform" else make_dist(("gauss", [0.0] * d, [0.35] * d))
    theta0 = (1.5 * rng.standard_normal((n, d))).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236 * rng.standard_normal((n, d))).astype(np.float32)
    return model, lp, mix, theta0, y0


_REF = {}


def reference(oracle, algo, kind, d, N, K, local="gauss", prior="gauss", n=N_CHAINS, steps=T):
    """the split-phase reference chain of a fixture, computed once and shared: (history [T][d][n], HostChains, HostMoments)"""
    key = (algo, kind, d, N, K, local, prior, n, steps)
    if key in _REF:
        return _REF[key]
    L = oracle
    model_o, lp_o, mix_o, theta0, y0 = case(kind, d, K, local, prior, n)
    model, lp = model_o.descriptor(), lp_o.descriptor()
    ref = mixture_ref.MixtureRef.from_descriptor(mix_o.descriptor())
    yd = y0.shape[1]
    Np = N if algo == "glmcmc" else 1
    R = Np * n
    hc = oracle_lib.HostChains(theta0, y0, chain0=CHAIN0)
    cs = hc.struct()
    hm = oracle_lib.HostMoments(n, d)
    buf = dict(theta_prop=np.zeros((R, d), np.float32), log_q=np.zeros(R, np.float32), sim_noise=np.zeros((R, yd), np.float32),
               log_u=np.zeros(n, np.float32), u_res=np.zeros(n, np.float64), is_global=np.zeros(n, np.int32),
               y_prop=np.zeros((R, yd), np.float32), prior_prop=np.zeros(R, np.float32), kern_prop=np.zeros(R, np.float32),
               prior_cur=np.zeros(n, np.float32), kern_cur=np.zeros(n, np.float32), q_cur=np.zeros(n, np.float32))
    io = A.StepIO(Np, d, yd, yd, *[buf[k].ctypes.data for k in ("theta_prop", "log_q", "sim_noise", "log_u", "u_res", "is_global", "y_prop",
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
        theta_c, log_q_c = ref.candidates(SEED, ids, 1 + t, Np, yd)
        for j in range(Np):
            rows = np.ones(n, bool) if j else (buf["is_global"] & 1).astype(bool)       # row 0 of a chain on the local branch is the local move
            buf["theta_prop"][j * n:(j + 1) * n][rows] = theta_c[j][rows]
            buf["log_q"][j * n:(j + 1) * n][rows] = log_q_c[j][rows]
        assert L.oracle_model_prior_log_prob(C.byref(model), buf["theta_prop"].ctypes.data, R, buf["prior_prop"].ctypes.data) == 0
        assert L.oracle_model_simulate(C.byref(model), buf["theta_prop"].ctypes.data, buf["sim_noise"].ctypes.data, R,
                                       buf["y_prop"].ctypes.data) == 0
        assert L.oracle_model_log_kernel(C.byref(model), buf["y_prop"].ctypes.data, R, buf["kern_prop"].ctypes.data) == 0
        buf["q_cur"][:] = ref.log_prob_f32(hc.theta.T)
        assert L.oracle_select(ALGO[algo], None, C.byref(cs), C.byref(run), C.byref(io)) == 0
        if t < 4:
            modes_drawn |= set(np.argmin(((theta_c[:, :, None, :].astype(np.float64) - ref.loc) ** 2 / ref.scale ** 2).sum(-1), axis=-1).ravel())
    for a in (hist, hc.theta, hc.y, hc.log_w, hc.flags, hc.n_moves, hm.sum_theta, hm.sum_outer, hm.sum_jump):
        a.setflags(write=False)
    _REF[key] = (hist, hc, hm, len(modes_drawn))
    return _REF[key]


def device_run(algo, kind, d, N, K, local="gauss", prior="gauss", n=N_CHAINS, steps=T, debug_flags=0, lanes=0):
    from glabcmcmc_amd import engine
    model_o, lp_o, mix_o, theta0, y0 = case(kind, d, K, local, prior, n)
    model, lp, mix = model_o.descriptor(), lp_o.descriptor(), mix_o.descriptor()
    dev = torch.device("cuda", 0)
    chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev, chain0=CHAIN0)
    if algo == "glmcmc":
        engine.init_weights(model, mix, chains)
    hist = torch.empty(steps, chains.d, chains.n, dtype=torch.float32, device=dev)
    mom = engine.Moments(chains.n, chains.d, dev)
    entry = "glabc_glmcmc_mix_steps" if algo == "glmcmc" else "glabc_globalmcmc_mix_steps"
    engine.run_steps(entry, model, lp, mix, chains, steps, 1, SEED, GF, N, history=hist, moments=mom, steps_per_launch=K_LAUNCH,
                     debug_flags=debug_flags, lanes_per_chain=lanes)
    torch.cuda.synchronize()
    return hist.cpu().numpy(), chains, mom


def assert_equals_reference(got, want, what, isir):
    hist, chains, mom = got
    hh, hc, hm, _ = want
    same = bits(hist) == bits(hh)
    assert same.all(), "%s: first mismatch at (t, dim, chain) = %s" % (what, np.argwhere(~same)[0])
    assert np.array_equal(bits(chains.theta.cpu().numpy()), bits(hc.theta)), what
    assert np.array_equal(bits(chains.y.cpu().numpy()), bits(hc.y)), what
    assert np.array_equal(chains.n_moves.cpu().numpy().astype(np.uint32), hc.n_moves), what
    if isir:
        flags = chains.flags.cpu().numpy().astype(np.uint32)
        assert np.array_equal(flags, hc.flags), what
        clear = (hc.flags & A.FLAG_LOCAL) == 0
        assert clear.any(), what
        assert np.array_equal(bits(chains.log_w.cpu().numpy()[clear]), bits(hc.log_w[clear])), what
    for name in ("sum_theta", "sum_outer", "sum_jump"):
        assert np.array_equal(getattr(mom, name).cpu().numpy().view(np.uint64), getattr(hm, name).view(np.uint64)), (what, name)


def assert_fixture_moves(want, what, K):
    hh, hc, hm, modes = want
    assert np.isfinite(hh).all(), what
    assert int((hc.n_moves > 0).sum()) >= hc.n // 2, what                  # the comparison is not one of chains standing still
    assert modes == K, "%s: %d of %d modes drawn" % (what, modes, K)


# ---- row-wise -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 8])
@pytest.mark.parametrize("d", range(1, 9))
def test_hip_mixture_rows(hip, oracle, d, K):
    """glabc_mixture_log_prob / glabc_mixture_forward: one row per lane, tail lanes masked, 64-bit row ids"""
    gm = make_mixture(K, d)
    desc = gm.descriptor()
    ref = mixture_ref.MixtureRef.from_descriptor(desc)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(d + 10 * K)
    for n in (1, 63, 64, 65, 257):
        z = np.concatenate([ref.loc[rng.integers(0, K, n)] + rng.standard_normal((n, d)) * rng.choice([0.5, 5.0, 40.0], (n, 1)) * ref.scale[0]])
        zt = torch.from_numpy(z).to(dev)
        out = torch.full((n + 1,), 7.0, dtype=torch.float64, device=dev)
        assert hip.glabc_mixture_log_prob(C.byref(desc), zt.data_ptr(), n, out.data_ptr(), None) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.array_equal(got[:n].view(np.uint64), ref.log_prob(z).view(np.uint64)), (n, "log_prob")
        assert got[n] == 7.0                                                  # nothing past the last row
        for row0 in (0, 2 ** 32 + 5):
            zo = torch.full((n + 1, d), 7.0, dtype=torch.float64, device=dev)
            lp = torch.full((n + 1,), 7.0, dtype=torch.float64, device=dev)
            assert hip.glabc_mixture_forward(C.byref(desc), n, SEED, row0, zo.data_ptr(), lp.data_ptr(), None) == 0
            torch.cuda.synchronize()
            zw, lw, _ = ref.forward_rows(n, SEED, row0)
            assert np.array_equal(zo.cpu().numpy()[:n].view(np.uint64), zw.view(np.uint64)), (n, row0, "z")
            assert np.array_equal(lp.cpu().numpy()[:n].view(np.uint64), lw.view(np.uint64)), (n, row0, "log_p")
            assert (zo.cpu().numpy()[n] == 7.0).all() and lp.cpu().numpy()[n] == 7.0
    # the class: log_prob on a CUDA tensor and forward with a CUDA device run these kernels; rows are counted across calls
    on_dev = make_mixture(K, d, device=dev)                                   # the same mixture; make_mixture's own seed names the fixture
    on_dev.seed = SEED
    z1, l1 = on_dev.forward(65)
    z2, l2 = on_dev.forward(64)
    zw, lw, _ = ref.forward_rows(129, SEED, 0)
    assert z1.dtype == torch.float64 and z1.shape == (65, d) and l2.shape == (64,)
    assert np.array_equal(torch.cat([z1, z2]).cpu().numpy().view(np.uint64), zw.view(np.uint64))
    assert np.array_equal(torch.cat([l1, l2]).cpu().numpy().view(np.uint64), lw.view(np.uint64))
    with pytest.raises(ValueError):
        gm.log_prob(torch.zeros(4, d + 1, dtype=torch.float64, device=dev))   # a column count the descriptor does not have
    lp = gm.log_prob(z1[:, 0] if d == 1 else z1)
    assert lp.dtype == torch.float64 and np.array_equal(lp.cpu().numpy().view(np.uint64), lw[:65].view(np.uint64))


# ---- fused GLMCMC ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("N", [1, 2, 5, 16])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_hip_glmcmc_mixture(hip, oracle, d, N, K):
    want = reference(oracle, "glmcmc", "abs", d, N, K)
    assert_fixture_moves(want, (d, N, K), K)
    assert_equals_reference(device_run("glmcmc", "abs", d, N, K), want, (d, N, K), True)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 5])
def test_hip_glmcmc_mixture_gk(hip, oracle, N):
    want = reference(oracle, "glmcmc", "gk", 4, N, 3)
    assert_fixture_moves(want, ("gk", N), 3)
    assert_equals_reference(device_run("glmcmc", "gk", 4, N, 3), want, ("gk", N), True)


@pytest.mark.gpu
@pytest.mark.parametrize("local,prior", [("uniform", "gauss"), ("gauss", "uniform")])
def test_hip_glmcmc_mixture_uniform_local_and_prior(hip, oracle, local, prior):
    want = reference(oracle, "glmcmc", "abs", 3, 5, 3, local, prior)
    assert_fixture_moves(want, (local, prior), 3)
    assert_equals_reference(device_run("glmcmc", "abs", 3, 5, 3, local, prior), want, (local, prior), True)
    # execution strategy only: the reference's index search always, and one lane per chain asked for by name
    got = device_run("glmcmc", "abs", 3, 5, 3, local, prior, debug_flags=A.DEBUG_EXACT_INDEX, lanes=1)
    assert_equals_reference(got, want, (local, prior, "exact index"), True)


@pytest.mark.gpu
@pytest.mark.parametrize("N", range(1, 17))
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_hip_glmcmc_mixture_every_instantiation(hip, oracle, d, N):
    want = reference(oracle, "glmcmc", "abs", d, N, 3, n=N_SMALL, steps=T_SMALL)
    assert np.isfinite(want[0]).all() and want[1].n_moves.sum() > 0
    assert_equals_reference(device_run("glmcmc", "abs", d, N, 3, n=N_SMALL, steps=T_SMALL), want, (d, N), True)


# ---- fused GlobalMCMC ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("kind,d", [("abs", 1), ("abs", 2), ("abs", 3), ("abs", 4), ("gk", 4)])
def test_hip_globalmcmc_mixture(hip, oracle, kind, d, K):
    want = reference(oracle, "globalmcmc", kind, d, 1, K)
    assert np.isfinite(want[0]).all() and int((want[1].n_moves > 0).sum()) >= N_CHAINS // 2
    assert_equals_reference(device_run("globalmcmc", kind, d, 1, K), want, (kind, d, K), False)


# ---- package level -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_hip_mixture_through_the_package(hip, oracle, tmp_path):
    """MCMCRunner.run_glmcmc / run_global_mcmc with a GaussianMixture: path='auto' runs the mixture kernels -- the bits of the
    direct C calls with the same seed; path='generic' still runs; one chain in, one chain out"""
    import glabcmcmc_amd as g_
    from glabcmcmc_amd import engine
    model, lp, mix, theta0, y0 = case("abs", 2, 3)
    runner = g_.MCMCRunner(model, str(tmp_path))
    t0, yy0 = torch.from_numpy(theta0), torch.from_numpy(y0)
    for algo, N in (("glmcmc", 5), ("globalmcmc", 1)):
        direct = device_run(algo, "abs", 2, N, 3)
        mom, state = engine.Moments(N_CHAINS, 2, torch.device("cuda", 0)), {}
        kw = dict(seed=SEED, chain0=CHAIN0, stats=mom, return_device=True, verbose=False, state_out=state, steps_per_launch=K_LAUNCH,
                  output_file=None)
        if algo == "glmcmc":
            h = runner.run_glmcmc(T + 1, t0, yy0, GF, lp, mix, N, **kw)
        else:
            h = runner.run_global_mcmc(T + 1, t0, yy0, GF, lp, mix, **kw)
        h = h.cpu().numpy()
        assert h.shape == (T + 1, N_CHAINS, 2) and np.array_equal(bits(h[0]), bits(theta0))
        assert np.array_equal(bits(h[1:].transpose(0, 2, 1)), bits(direct[0])), algo
        assert np.array_equal(bits(state["chains"].y.cpu().numpy()), bits(direct[1].y.cpu().numpy())), algo
        assert np.array_equal(mom.sum_jump.cpu().numpy().view(np.uint64), direct[2].sum_jump.cpu().numpy().view(np.uint64)), algo
        assert_equals_reference(direct, reference(oracle, algo, "abs", 2, N, 3), algo, algo == "glmcmc")
        kw = dict(seed=SEED, return_device=True, verbose=False, output_file=None, path="generic")
        if algo == "glmcmc":
            g = runner.run_glmcmc(12, t0, yy0, GF, lp, mix, N, **kw)
        else:
            g = runner.run_global_mcmc(12, t0, yy0, GF, lp, mix, **kw)
        assert g.shape == (12, N_CHAINS, 2) and torch.isfinite(g).all() and (g[-1] != g[0]).any()
    one = runner.run_glmcmc(30, t0[0], yy0[0], GF, lp, mix, 5, seed=SEED, verbose=False, output_file=None)
    assert one.shape == (30, 2) and one.dtype == torch.float32 and not one.is_cuda and torch.isfinite(one).all()
    one = runner.run_global_mcmc(30, t0[:1], yy0[:1], GF, lp, mix, seed=SEED, verbose=False, output_file=None)
    assert one.shape == (30, 2) and torch.isfinite(one).all()
