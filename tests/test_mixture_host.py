"""GaussianMixture on the host: the descriptor's constants, the dispatch, the numpy restatement (tests/mixture_ref.py) against the
host class's torch float64 arithmetic and against itself, and the argument checks of the mixture entry points.

The restatement is what tests/test_mixture_shapes.py holds the kernels to bit for bit, so it is checked here first: the two
pieces it restates for speed against the CPU checker's exports, and its log_prob against torch within
1e-12 * max(1, |value|) -- the bound the project holds its float64 Gamma density to.  (Not bitwise: the specification
multiplies by a host-formed reciprocal where the reference divides, include/glabc.h.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mixture_ref
import oracle_lib
from helpers import make_dist
from test_arg_checks import ARG, DIM, KIND, NULL, OK, check_table
from test_stream_independence import abs_gauss_model
from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import distribution, generic


def make_mixture(K, d, seed=0, spread=3.0, **kw):
    """K modes in d dimensions: centres `spread` apart on a grid, in shuffled order, unequal scales and weights"""
    rng = np.random.default_rng(1000 * K + 10 * d + seed)
    idx = rng.permutation(K)
    cell = (idx[:, None] // 3 ** np.arange(d)[None, :]) % 3 - 1.0
    cell[:, 0] += 3.0 * (idx // 3 ** d)                       # more modes than grid cells: further out along the first axis
    loc = spread * cell + 0.1 * rng.standard_normal((K, d))
    scale = 0.3 + 0.5 * rng.random((K, d))
    weights = 0.5 + rng.random(K)
    return distribution.GaussianMixture(K, d, loc=loc, scale=scale, weights=weights, **kw)


# ---- the restatement's own pieces ------------------------------------------------------------------------------------------
def test_vectorised_philox_equals_the_checkers(oracle):
    rng = np.random.default_rng(1)
    ctr = rng.integers(0, 2 ** 32, (200, 4), dtype=np.uint64).astype(np.uint32)
    ctr[:3] = [[0, 0, 0, 0], [0xFFFFFFFF] * 4, [7, 1, 60, mixture_ref.SLOT_MIX + 15]]
    key = np.array([0x9E3779B9, 0xFFFFFFFE], np.uint32)
    got = np.stack(mixture_ref.philox4x32_10(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], key[0], key[1]), axis=1)
    want = np.empty((200, 4), np.uint32)
    for i in range(200):
        oracle.oracle_philox4x32_10(ctr[i].ctypes.data, key.ctypes.data, want[i].ctypes.data)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("n", range(1, 9))
def test_vectorised_rowsum_equals_the_checkers(oracle, n):
    rng = np.random.default_rng(n)
    x = np.ascontiguousarray(rng.standard_normal((300, n)) * 10.0 ** rng.integers(-8, 8, (300, n)))
    want = np.array([oracle.oracle_aten_rowsum_f64(x[i].ctypes.data, n) for i in range(300)])
    assert np.array_equal(mixture_ref.rowsum_f64(x).view(np.uint64), want.view(np.uint64))


# ---- packing -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("d", [1, 2, 4, 8])
def test_descriptor_packs_the_listed_constants(K, d):
    gm = make_mixture(K, d)
    m = gm.descriptor()
    assert isinstance(m, A.Mixture) and (m.n_modes, m.dim) == (K, d)
    with torch.no_grad():
        scale = torch.exp(gm.log_scale)[0].numpy()
        weights = torch.softmax(gm.weight_scores, 1)
        want = dict(loc=gm.loc[0].numpy(), scale=scale, inv_scale=1.0 / scale, log_weight=torch.log(weights)[0].numpy(),
                    cum_weight=np.cumsum(weights[0].numpy()), sum_log_scale=torch.sum(gm.log_scale, 2)[0].numpy())
    ref = mixture_ref.MixtureRef.from_descriptor(m)
    for name, w in want.items():
        assert w.dtype == np.float64
        assert np.array_equal(getattr(ref, name).view(np.uint64), w.view(np.uint64)), name
    assert m.c0 == -0.5 * d * np.log(2 * np.pi)
    # what lies beyond the modes and coordinates in use is zero
    assert all(m.loc[k][q] == 0.0 for k in range(A.MAX_MODES) for q in range(A.MAX_DIM) if k >= K or q >= d)


def test_descriptor_refuses_what_the_struct_cannot_hold():
    with pytest.raises(ValueError):
        distribution.GaussianMixture(9, 2, loc=np.zeros((9, 2))).descriptor()
    with pytest.raises(ValueError):
        distribution.GaussianMixture(2, 9, loc=np.zeros((2, 9))).descriptor()
    assert generic.try_descriptor(distribution.GaussianMixture(9, 2, loc=np.zeros((9, 2)))) is None
    assert generic.dist_descriptor(make_mixture(3, 2), 2) is None            # everywhere else it stays a callback


def test_dispatch_takes_a_mixture_inside_the_support_matrix_only():
    from helpers import AbsGaussModel
    from glabcmcmc_amd.examples.GK import GK_set

    def ok(model, d, N, K=3, **kw):
        local = make_dist(("gauss", [0.0] * d, [0.3] * d))
        return generic.fused_supported(model, (local, make_mixture(K, d)), N, A.MAX_BATCH_WIDE, gamma_ok=True, mixture_ok=True, **kw)

    for d in (1, 2, 3, 4):
        for N in (1, 5, 16):
            assert ok(AbsGaussModel(0.3, [1.5] * d), d, N)
    assert ok(GK_set(1.0), 4, 5) and ok(AbsGaussModel(0.3, [1.5] * 2), 2, 16, K=8)
    assert not ok(AbsGaussModel(0.3, [1.5] * 2), 2, 17)                      # batch sizes above 16: lane groups, a callback
    assert not ok(AbsGaussModel(0.3, [1.5] * 5), 5, 5)                       # theta_dim 5..8
    assert not ok(GK_set(1.0, prior=make_dist(("gamma", [3.0, 2.0, 2.0, 1.5], [1.0, 2.0, 1.0, 3.0]))), 4, 5)     # a Gamma prior
    model, local, mix = AbsGaussModel(0.3, [1.5] * 2), make_dist(("gauss", [0.0] * 2, [0.3] * 2)), make_mixture(3, 2)
    assert not generic.fused_supported(model, (local, mix), 5, gamma_ok=True)                    # an entry point without the variant
    assert not generic.fused_supported(model, (mix, mix), 1, gamma_ok=True, mixture_ok=True)     # a mixture as the local increment
    assert not generic.fused_supported(model, (local, make_mixture(3, 3)), 5, mixture_ok=True)   # dimension mismatch


# ---- the restatement against the host class ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,d", [(1, 1), (2, 1), (3, 2), (8, 4), (5, 8), (8, 8), (4, 3)])
def test_restatement_log_prob_equals_torch_float64(oracle, K, d):
    """4096 points: draws of the mixture itself, points around each centre out to 50 scales, and a wide uniform cloud"""
    gm = make_mixture(K, d)
    ref = mixture_ref.MixtureRef.from_descriptor(gm.descriptor())
    rng = np.random.default_rng(K + d)
    own = gm.forward(1024)[0].detach().numpy()
    k = rng.integers(0, K, 2048)
    reach = np.concatenate([np.linspace(0.0, 50.0, 1024), rng.uniform(0.0, 50.0, 1024)])
    direction = rng.standard_normal((2048, d))
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    tails = ref.loc[k] + reach[:, None] * direction * ref.scale[k]
    cloud = rng.uniform(-40.0, 40.0, (1024, d))
    z = np.concatenate([own, tails, cloud])
    assert z.shape == (4096, d)
    with torch.no_grad():
        zt = torch.from_numpy(z)
        want = gm.log_prob(zt[:, 0] if d == 1 else zt).numpy()
    got = ref.log_prob(z)
    assert want.dtype == np.float64 and np.isfinite(want).all()
    gap = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    print("K=%d d=%d: worst |restatement - torch| / max(1, |value|) = %.3e" % (K, d, gap.max()))
    assert gap.max() <= 1e-12


# ---- the restatement against itself --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,d", [(1, 1), (3, 2), (8, 5)])
def test_forward_log_p_is_log_prob_at_its_own_z(oracle, K, d):
    ref = mixture_ref.MixtureRef.from_descriptor(make_mixture(K, d).descriptor())
    z, log_p, mode = ref.forward_rows(500, seed=12345, row0=2 ** 32 + 5)
    assert np.array_equal(log_p.view(np.uint64), ref.log_prob(z).view(np.uint64))
    assert len(np.unique(mode)) == K
    theta, log_q = ref.candidates(77, np.arange(40, dtype=np.uint64) + 2 ** 32, 9, 4, d)
    assert theta.shape == (4, 40, d) and np.isfinite(log_q).all()


def test_a_uniform_on_a_cumulative_weight_picks_the_next_mode(oracle):
    ref = mixture_ref.MixtureRef.from_descriptor(make_mixture(3, 2).descriptor())
    c = ref.cum_weight
    assert list(ref.mode(np.array([0.0, np.nextafter(c[0], 0.0), c[0], np.nextafter(c[1], 0.0), c[1], 1.0, 2.0]))) == [0, 0, 1, 1, 2, 2, 2]
    one = mixture_ref.MixtureRef.from_descriptor(make_mixture(1, 2).descriptor())
    assert list(one.mode(np.array([0.0, 0.999, 1.0]))) == [0, 0, 0]
    # and the variate of a draw that lands there is the next mode's
    z, _, k = ref.draw(np.array([c[0]]), np.zeros((1, 2), np.float32))
    assert k[0] == 1 and np.array_equal(z[0], ref.loc[1])


# ---- argument checks (csrc/glabc_check.h on the CPU, as tests/test_arg_checks.py does) -------------------------------------------
MIX_PRELUDE = """
static glabc_mixture mix3(int dim)
{
    glabc_mixture g;
    std::memset(&g, 0, sizeof g);
    g.n_modes = 3;
    g.dim = dim;
    for (int k = 0; k < 3; ++k) {
        for (int q = 0; q < dim; ++q) { g.loc[k][q] = k - 1.0; g.scale[k][q] = 0.5; g.inv_scale[k][q] = 2.0; }
        g.log_weight[k] = -1.0986122886681098;
        g.cum_weight[k] = (k + 1) / 3.0;
        g.sum_log_scale[k] = -0.6931471805599453 * dim;
    }
    g.c0 = -0.9189385332046727 * dim;
    return g;
}
"""
RUN = "check_mix_run(&b.m, &b.g, &x, &b.c, &b.r, %s)"


def mix_rows():
    rows = []
    for isir in ("true", "false"):
        call = RUN % isir

        def row(spoil, want, dim=3, call=call):
            rows.append(("glabc_mixture x = mix3(%d); glabc_tape tp; std::memset(&tp, 0, sizeof tp); (void)tp; %s" % (dim, spoil), call, want))

        row("", OK)
        row("b.r.lanes_per_chain = 1;", OK)
        row("b.r.debug_flags = GLABC_DEBUG_EXACT_INDEX; b.r.history = b.f; b.r.hist_stride = 65; b.r.moments = &b.mo; "
            "b.r.global_frequency_per_chain = b.f;", OK)
        row("b.m.prior = dist3(GLABC_DIST_DIAG_GAUSS); b.g = dist3(GLABC_DIST_UNIFORM);", OK)
        row("make_gk(b); b.g.dim = 4; b.g.p2[3] = 0.5f;", OK, dim=4)
        # the support matrix
        row("b.m.theta_dim = b.m.y_dim = 5; b.m.prior.dim = b.m.noise.dim = b.g.dim = 5; b.m.prior.p1[3] = b.m.prior.p1[4] = 3.0f; "
            "b.g.p2[3] = b.g.p2[4] = 0.5f; b.m.noise.p2[3] = b.m.noise.p2[4] = 0.5f;", KIND, dim=5)
        row("b.m.prior = dist3(GLABC_DIST_GAMMA);", KIND)
        row("make_gk(b); b.g.dim = 4; b.g.p2[3] = 0.5f; b.m.prior = dist3(GLABC_DIST_GAMMA); b.m.prior.dim = 4; b.m.prior.p0[3] = 2.0f; "
            "b.m.prior.p1[3] = 0.5f; b.m.prior.p2[3] = 2.0f;", KIND, dim=4)
        row("b.r.tape = &tp;", ARG)
        row("b.r.math_mode = GLABC_MATH_FAST;", ARG)
        row("b.g = dist3(GLABC_DIST_GAMMA);", KIND)                             # the local increment is never a Gamma
        row("b.r.lanes_per_chain = 2;", ARG)
        row("b.r.lanes_per_chain = 4;", ARG)
        # the mixture itself
        row("x.n_modes = 0;", ARG)
        row("x.n_modes = 9;", ARG)
        row("", DIM, dim=2)
        row("x.dim = 0;", DIM)
        row("x.dim = 9;", DIM)
        for field in ("scale", "inv_scale"):
            for bad in ("0.0", "-1.0", "Inf", "NaN"):
                row("x.%s[2][1] = %s;" % (field, bad), ARG)
        row("x.loc[0][2] = NaN;", ARG)
        row("x.cum_weight[1] = 0.2;", ARG)                                      # not monotone
        row("x.cum_weight[1] = NaN;", ARG)
        row("x.cum_weight[2] = 1.0 + 1e-8;", ARG)
        row("x.cum_weight[2] = 1.0 + 5e-10;", OK)
        row("x.cum_weight[0] = x.cum_weight[1] = x.cum_weight[2] = 0.0;", ARG)
        row("x.cum_weight[0] = 0.0; x.log_weight[0] = -Inf;", OK)               # a mode of weight zero
        row("x.log_weight[1] = NaN;", ARG)
        row("x.sum_log_scale[1] = Inf;", ARG)
        row("x.c0 = NaN;", ARG)
        row("x.scale[5][1] = -1.0; x.cum_weight[7] = NaN;", OK)                 # beyond n_modes nothing is read
        # what every stepping entry point asks
        row("b.r.n_steps = -1;", ARG)
        row("b.r.global_frequency = NaN;", ARG)
        row("b.r.step0_device = b.u;", ARG)
        row("b.r.history = b.f; b.r.hist_stride = 64;", ARG)
        row("b.c.theta = nullptr;", NULL)
        row("b.c.chain0 = -1;", ARG)
        if isir == "true":
            row("b.r.batch_size = 0;", ARG)
            row("b.r.batch_size = 17;", ARG)
            row("b.r.batch_size = 16;", OK)
            row("b.c.log_w = nullptr;", NULL)
        else:
            row("b.r.batch_size = 4096; b.c.log_w = nullptr; b.c.flags = nullptr;", OK)     # GlobalMCMC ignores both
    rows.append(("", "check_mix_run(&b.m, &b.g, nullptr, &b.c, &b.r, true)", NULL))
    rows.append(("glabc_mixture x = mix3(3);", "check_mix_run(&b.m, &b.g, &x, &b.c, nullptr, true)", NULL))
    rows.append(("glabc_mixture x = mix3(3);", "check_mix_run(nullptr, &b.g, &x, &b.c, &b.r, true)", NULL))
    # glabc_init_weights_mix and the row-wise entry points
    rows.append(("glabc_mixture x = mix3(3);", "check_mix_model(&b.m, &x)", OK))
    rows.append(("glabc_mixture x = mix3(3); b.m.prior = dist3(GLABC_DIST_GAMMA);", "check_mix_model(&b.m, &x)", KIND))
    rows.append(("glabc_mixture x = mix3(2);", "check_mix_model(&b.m, &x)", DIM))
    for dim in range(1, 9):
        rows.append(("glabc_mixture x = mix3(%d);" % dim, "check_mixture(&x, 0)", OK))
    rows.append(("", "check_mixture(nullptr, 0)", NULL))
    return rows


def test_mixture_argument_checks(tmp_path_factory, monkeypatch):
    import test_arg_checks
    monkeypatch.setattr(test_arg_checks, "PRELUDE", test_arg_checks.PRELUDE.replace("struct Base {", MIX_PRELUDE + "struct Base {"))
    check_table(tmp_path_factory, "mixture", mix_rows())


def test_entry_points_refuse_before_touching_a_device():
    """the library itself (it loads without a GPU): a refused call returns its status with no device present"""
    lib = A.bind(A.LIB_PATH)
    model = abs_gauss_model(3, 0.3)
    local = make_dist(("gauss", [0.0] * 3, [0.3] * 3)).descriptor()
    buf = np.zeros(256, np.float64)
    chains = A.Chains(65, 0, 65, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None, None, None, None, None)
    run = A.Run()
    run.step0, run.n_steps, run.global_frequency, run.batch_size = 1, 3, 0.5, 5

    def mix(**spoil):
        m = make_mixture(3, 3).descriptor()
        for k, v in spoil.items():
            setattr(m, k, v)
        return m

    call = lambda m, r=run, mod=model: lib.glabc_glmcmc_mix_steps(C.byref(mod), C.byref(local), C.byref(m), C.byref(chains), C.byref(r), None)   # noqa: E731
    assert call(mix(n_modes=0)) == ARG and call(mix(n_modes=9)) == ARG and call(mix(dim=2)) == DIM
    bad = mix()
    bad.inv_scale[1][1] = float("inf")
    assert call(bad) == ARG
    fast = A.Run()
    fast.step0, fast.n_steps, fast.global_frequency, fast.batch_size, fast.math_mode = 1, 3, 0.5, 5, A.MATH_FAST
    assert call(mix(), r=fast) == ARG
    tape = A.Tape(buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 5, 0)
    taped = A.Run()
    taped.step0, taped.n_steps, taped.global_frequency, taped.batch_size, taped.tape = 1, 3, 0.5, 5, C.pointer(tape)
    assert call(mix(), r=taped) == ARG
    gamma_model = abs_gauss_model(3, 0.3)
    gamma_model.prior = make_dist(("gamma", [2.0] * 3, [1.0] * 3)).descriptor()
    assert call(mix(), mod=gamma_model) == KIND
    m5, l5 = abs_gauss_model(5, 0.3), make_dist(("gauss", [0.0] * 5, [0.3] * 5)).descriptor()
    x5 = make_mixture(3, 5).descriptor()
    assert lib.glabc_glmcmc_mix_steps(C.byref(m5), C.byref(l5), C.byref(x5), C.byref(chains), C.byref(run), None) == KIND
    assert lib.glabc_globalmcmc_mix_steps(C.byref(m5), C.byref(l5), C.byref(x5), C.byref(chains), C.byref(run), None) == KIND
    assert lib.glabc_init_weights_mix(C.byref(m5), C.byref(x5), C.byref(chains), None) == KIND
    assert lib.glabc_init_weights_mix(C.byref(model), C.byref(mix(n_modes=9)), C.byref(chains), None) == ARG
    assert lib.glabc_mixture_log_prob(C.byref(mix(n_modes=9)), buf.ctypes.data, 4, buf.ctypes.data, None) == ARG
    assert lib.glabc_mixture_log_prob(C.byref(mix()), None, 4, buf.ctypes.data, None) == NULL
    assert lib.glabc_mixture_forward(C.byref(mix(dim=9)), 4, 1, 0, buf.ctypes.data, buf.ctypes.data, None) == DIM
    assert lib.glabc_mixture_forward(C.byref(mix()), 4, 1, -1, buf.ctypes.data, buf.ctypes.data, None) == ARG
    assert lib.glabc_mixture_forward(C.byref(mix()), 0, 1, 0, buf.ctypes.data, buf.ctypes.data, None) == OK      # nothing to do
