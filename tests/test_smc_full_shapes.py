"""glabc_smc_draws_full / glabc_kde_sample_full (csrc/glabc_smc.hip, csrc/glabc_kde.hip) and ``smc.sample(perturbation="full")`` on the GPU.

Bit for bit: the fused kernel against (a) the on-device composition glabc_kde_sample_full -> transpose -> glabc_model_prior_log_prob ->
glabc_model_simulate(eps = NULL, seed ^ GLABC_ABC_NOISE_KEY) -> glabc_model_discrepancy -> where(log_prior == -inf, inf, distance) and
(b) the restatement in NumPy float32 from the CPU checker's ancestor and normals (tests/smc_full_ref.py), the acceptance included, on
|theta| + noise at every theta_dim 1 .. 8 with a DiagGaussian and with a Uniform prior and on g-and-k.  The factor is dense: the
marginal scales are the bandwidths of tests/test_smc_shapes.py's populations, neighbouring coordinates correlate at +-0.95, so the
Uniform-prior populations again hold rows inside and rows outside the support (asserted).  Shapes: n around the wavefront and the
workgroup, row0 across the counter's low word and past it, listed ids out of order with a repeat and a value >= 2^32, stride = n + 5,
each output alone, n = 0, the refusals in their order; populations of 1 .. 4097 centres with uniform, random (exact zeros) and one-hot
weights.  Every buffer lies between guard bands of canaries.  A diagonal factor gives glabc_smc_draws' bits.

The density.  ``smc._FullKernel`` evaluates log q by whitening around the weighted mean and glabc_kde_log_prob in float32; it is held
to the float64 restatement (smc_full_ref.log_q) on populations of 1000 centres at theta_dim 2, 4 and 8, one of them with centres
near 1000 and spread 0.01.  Largest differences measured on an MI355X over 512 points each: 5.2e-7 (D = 2), 9.6e-7 (D = 4),
1.6e-6 (D = 8), 1.7e-6 (D = 4, centres near 1000); LOGQ_TOL = 6.8e-6 is 4 times the largest, because the kernel's float32 terms
depend on the points.  A NumPy float32 emulation of the same path without the centring is off by 3.9e-2 in the last case.

smc.sample(perturbation="full"): the same call under two launch sizes, the first full generation against the restated loop, the law
against the analytic posterior of Mixture_set, and the correlated linear Model as a CompiledModel: self-check of the three draw
kernels, the closed-form Gaussian posterior within 5 standard errors, and at most half the diagonal kernel's simulations under
bandwidth="beaumont".
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rejection_ref as R
import smc_full_ref as F
import smc_ref as S
from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import distribution, rejection, smc
from glabcmcmc_amd.examples import Correlated_smc
from glabcmcmc_amd.examples.Mixture import Mixture_set
from helpers import bits, canary_left, dev, host
from test_rejection_shapes import ERR_ARG, ERR_DIM, ERR_KIND, ERR_NULL, MODELS, ROW0S, SEED, Guarded, model_of
from test_smc_shapes import DevicePopulation, population_of
from test_smc_shapes import call as call_diagonal

pytestmark = pytest.mark.gpu

N_REF = 1000
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
NAMES = ("theta", "y", "distance", "log_prior", "accept")
LOGQ_TOL = 6.8e-6                       # 4 x 1.7e-6, the largest difference measured (module docstring)


@functools.lru_cache(maxsize=None)
def factor_of(key):
    """a dense factor with the marginal scales of the population's bandwidth"""
    L = F.dense_factor(population_of(key).host.bandwidth, seed=key[1])
    L.setflags(write=False)
    return L


def restated(model, hostpop, L, ids):
    theta, y, lp, dis, acc = F.restate(model, hostpop, L, SEED, ids)
    return {"theta": theta, "y": y, "distance": dis, "log_prior": lp, "accept": acc}


@functools.lru_cache(maxsize=None)
def reference(key, row0):
    """the restated draws row0 .. row0 + N_REF - 1 of a Model, its population and factor: computed once, never modified"""
    out = restated(model_of(key), population_of(key).host, factor_of(key), np.arange(N_REF, dtype=np.int64) + row0)
    for a in out.values():
        a.setflags(write=False)
    return out


def call(hip, model, pop, L, row0, ids, n, stride, want=NAMES, seed=SEED, expect=0, chol=None):
    """one glabc_smc_draws_full call into guarded buffers -> {name: host array}; theta / y come back as [n][dim].  `chol` overrides
    the packed factor (a host array, or 0 for NULL)"""
    buf = {"theta": Guarded(model.theta_dim, stride), "y": Guarded(model.y_dim, stride), "distance": Guarded(1, stride),
           "log_prior": Guarded(1, stride), "accept": Guarded(1, stride, u8=True)}
    idt = None if ids is None else dev(np.asarray(ids, np.int64))
    packed = F.pack(L) if chol is None else chol
    p = lambda name: buf[name].ptr if name in want else None          # noqa: E731
    rc = hip.glabc_smc_draws_full(C.byref(model), None if pop is None else C.byref(pop.struct), None if packed is None or isinstance(packed, int) else packed.ctypes.data,
                                  seed, row0, None if idt is None else idt.data_ptr(), n, stride, p("theta"), p("y"), p("distance"), p("log_prior"),
                                  p("accept"), None)
    torch.cuda.synchronize()
    assert rc == expect, rc
    out = {}
    for name, b in buf.items():
        if name in want and rc == 0 and n > 0:
            a = b.read(n)
            out[name] = np.ascontiguousarray(a.T) if name in ("theta", "y") else a[0].copy()
        else:
            b.untouched()
    if "accept" in out:
        assert np.isin(out["accept"], (0, 1)).all()
    for name in ("theta", "y", "distance", "log_prior"):
        if name in out:
            assert canary_left(out[name]) == 0, "%s: an element the call owns was never written" % name
    return out


def assert_equals(got, ref, rows, what):
    for name in NAMES:
        if name in got:
            same = np.array_equal(got[name], ref[name][rows]) if name == "accept" else np.array_equal(bits(got[name]), bits(ref[name][rows]))
            assert same, "%s: %s differs from the restatement" % (what, name)


def composed(hip, model, pop, L, row0, n):
    """the twin: glabc_kde_sample_full, then the row-wise entry points, theta and y through device memory"""
    d, yd = model.theta_dim, model.y_dim
    z = torch.empty(d, n, device="cuda")
    packed = F.pack(L)
    assert hip.glabc_kde_sample_full(C.byref(pop.struct), packed.ctypes.data, n, SEED, row0, z.data_ptr(), None) == 0
    theta = z.t().contiguous()
    lp, y, dis = torch.empty(n, device="cuda"), torch.empty(n, yd, device="cuda"), torch.empty(n, device="cuda")
    assert hip.glabc_model_prior_log_prob(C.byref(model), theta.data_ptr(), n, lp.data_ptr(), None) == 0
    assert hip.glabc_model_simulate(C.byref(model), theta.data_ptr(), None, n, SEED ^ R.NOISE_KEY, row0, y.data_ptr(), None) == 0
    assert hip.glabc_model_discrepancy(C.byref(model), y.data_ptr(), n, dis.data_ptr(), None) == 0
    dis = torch.where(lp == -np.inf, torch.full_like(dis, np.inf), dis)
    return {"theta": host(theta), "y": host(y), "distance": host(dis), "log_prior": host(lp)}


# ---------------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("key", MODELS, ids=lambda k: "%s%d" % k)
def test_fused_equals_composition_and_restatement(hip, key):
    model, pop, L = model_of(key), population_of(key), factor_of(key)
    if key[1] > 1:                                                         # dense, and correlated as announced
        corr = (np.float64(L) @ np.float64(L).T) / np.outer(pop.host.bandwidth, pop.host.bandwidth).astype(np.float64)
        assert L[np.tril_indices(key[1])].all() and np.allclose(np.abs(np.diagonal(corr, 1)), 0.95, atol=1e-5) and np.allclose(np.diagonal(corr), 1.0, atol=1e-5)
    for row0 in ROW0S:
        ref = reference(key, row0)
        if key[0] == "uniform":                                            # both classes occur, so the +inf rule is under test
            outside = np.isinf(ref["log_prior"])
            assert 20 < outside.sum() < N_REF - 20 and np.isinf(ref["distance"][outside]).all() and np.isfinite(ref["distance"][~outside]).all()
            assert not ref["accept"][outside].any() and np.isfinite(ref["y"]).all()
        got = call(hip, model, pop, L, row0, None, N_REF, N_REF + 5)
        assert_equals(got, ref, slice(None), "%r row0 %d" % (key, row0))
        twin = composed(hip, model, pop, L, row0, N_REF)
        for name, want in twin.items():
            assert np.array_equal(bits(got[name]), bits(want)), "%r row0 %d: %s differs from the composed entry points" % (key, row0, name)
        assert got["accept"].any() and (key[0] == "gk" or not got["accept"].all())


@pytest.mark.parametrize("key", MODELS, ids=lambda k: "%s%d" % k)
def test_a_diagonal_factor_gives_the_diagonal_kernels_bits(hip, key):
    model, pop = model_of(key), population_of(key)
    assert not (bits(pop.host.xs) == 0x80000000).any()                     # no centre is -0: the one corner where the two differ
    L = np.diag(pop.host.bandwidth).astype(np.float32)
    for row0 in ROW0S[:2]:
        got = call(hip, model, pop, L, row0, None, 257, 262)
        want = call_diagonal(hip, model, pop, row0, None, 257, 262)
        for name in NAMES:
            assert np.array_equal(got[name].view(np.uint8), want[name].view(np.uint8)), "%r: %s" % (key, name)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_wavefront_and_the_workgroup(hip, n):
    for key in (("gauss", 2), ("uniform", 5), ("gk", 4)):
        for row0 in ROW0S[:2]:
            got = call(hip, model_of(key), population_of(key), factor_of(key), row0, None, n, n + 5)
            assert_equals(got, reference(key, row0), slice(0, n), "%r n %d" % (key, n))
    got = call(hip, model_of(("gauss", 2)), population_of(("gauss", 2)), factor_of(("gauss", 2)), 0, None, n, n)          # no padding column
    assert_equals(got, reference(("gauss", 2), 0), slice(0, n), "stride = n")


@pytest.mark.parametrize("key", [("gauss", 1), ("uniform", 3), ("gauss", 8), ("gk", 4)], ids=lambda k: "%s%d" % k)
def test_listed_ids(hip, key):
    model, pop, L = model_of(key), population_of(key), factor_of(key)
    base = 2 ** 32 - 3
    ids = np.array([base + 700, 5, base + 2, 5, 2 ** 40 + 999, 0, base + 3, 999, base + 2], np.int64)          # unsorted, repeats, >= 2^32
    got = call(hip, model, pop, L, 0, ids, ids.size, ids.size + 5)
    assert_equals(got, restated(model, pop.host, L, ids), slice(None), "ids")
    n = 300                                                                # more than a workgroup of listed ids, permuted
    perm = np.random.default_rng(1).permutation(n).astype(np.int64) + base
    got = call(hip, model, pop, L, 0, perm, n, n + 5)
    assert_equals(got, reference(key, base), perm - base, "permuted ids")


@pytest.mark.parametrize("key", [("gauss", 2), ("uniform", 7), ("gk", 4)], ids=lambda k: "%s%d" % k)
def test_each_output_alone_gives_the_same_bits(hip, key):
    model, pop, L, n, row0 = model_of(key), population_of(key), factor_of(key), 257, ROW0S[1]
    ref = reference(key, row0)
    for want in (("theta",), ("y",), ("distance",), ("log_prior",), ("accept",), ("theta", "accept"), ("y", "log_prior"), ("y", "distance")):
        got = call(hip, model, pop, L, row0, None, n, n + 5, want=want)    # call() checks that the other buffers keep their canaries
        assert set(got) == set(want)
        assert_equals(got, ref, slice(0, n), "want %r" % (want,))


def test_nothing_is_written_for_n_0_and_by_a_refused_call(hip):
    key = ("gauss", 2)
    model, pop, L = model_of(key), population_of(key), factor_of(key)
    assert call(hip, model, pop, L, 0, None, 0, 0) == {} and call(hip, model, pop, L, 7, None, 0, 5) == {} and call(hip, model, pop, L, 0, [], 0, 0) == {}
    nan, zero, neg, inf = (F.pack(L) for _ in range(4))
    nan[1], zero[0], neg[2], inf[2] = np.nan, 0.0, -neg[2], np.inf
    # the factor: NULL, then its values
    call(hip, model, pop, L, 0, None, 10, 10, chol=0, expect=ERR_NULL)
    for bad in (nan, zero, neg, inf):
        call(hip, model, pop, L, 0, None, 10, 10, chol=bad, expect=ERR_ARG)
    # ... after the Model and the population
    call(hip, model, pop, L, 0, None, 10, 10, want=(), chol=zero, expect=ERR_NULL)
    call(hip, model, None, L, 0, None, 10, 10, chol=zero, expect=ERR_NULL)
    user = model_of(key)
    user.sim_kind = A.SIM_USER
    call(hip, user, pop, L, 0, None, 10, 10, chol=0, expect=ERR_KIND)
    gamma = Mixture_set(0.05, prior=distribution.Gamma(torch.tensor([2.0, 2.0]), torch.tensor([1.0, 1.0]))).descriptor()
    call(hip, gamma, pop, L, 0, None, 10, 10, chol=zero, expect=ERR_KIND)
    odd = model_of(key)
    odd.y_dim = 3
    call(hip, odd, pop, L, 0, None, 10, 10, chol=0, expect=ERR_DIM)
    call(hip, model, population_of(("gauss", 3)), L, 0, None, 10, 10, chol=0, expect=ERR_DIM)          # a population of another dimension
    for spoil, want in ((lambda k: setattr(k, "cum_q", None), ERR_NULL), (lambda k: setattr(k, "x", None), ERR_NULL),
                        (lambda k: setattr(k, "n_samples", 0), ERR_ARG), (lambda k: k.bandwidth.__setitem__(1, 0.0), ERR_ARG)):
        bad = DevicePopulation(pop.host)
        spoil(bad.struct)
        call(hip, model, bad, L, 0, None, 10, 10, chol=zero, expect=want)
    # ... and before the range of draws
    call(hip, model, pop, L, 0, None, 10, 9, chol=0, expect=ERR_NULL)
    call(hip, model, pop, L, -1, None, 10, 10, chol=zero, expect=ERR_ARG)
    call(hip, model, pop, L, 0, None, 10, 9, expect=ERR_ARG)
    call(hip, model, pop, L, -1, None, 10, 10, expect=ERR_ARG)
    call(hip, model, pop, L, 3, [1, 2, 3], 3, 3, expect=ERR_ARG)
    call(hip, model, pop, L, 0, None, -1, 10, expect=ERR_ARG)
    # glabc_kde_sample_full: glabc_kde_sample's refusals with the factor's behind the population's
    out = Guarded(2, 10)
    packed = F.pack(L)
    sample = lambda k, chol, n, row0, o: hip.glabc_kde_sample_full(None if k is None else C.byref(k), chol, n, SEED, row0, o, None)          # noqa: E731
    assert sample(None, packed.ctypes.data, 10, 0, out.ptr) == ERR_NULL and sample(pop.struct, None, 10, 0, out.ptr) == ERR_NULL
    assert sample(pop.struct, zero.ctypes.data, 10, 0, out.ptr) == ERR_ARG and sample(pop.struct, nan.ctypes.data, -1, 0, out.ptr) == ERR_ARG
    assert sample(pop.struct, packed.ctypes.data, -1, 0, out.ptr) == ERR_ARG and sample(pop.struct, packed.ctypes.data, 10, -1, out.ptr) == ERR_ARG
    assert sample(pop.struct, packed.ctypes.data, 0, 0, None) == 0 and sample(pop.struct, packed.ctypes.data, 10, 0, None) == ERR_NULL
    torch.cuda.synchronize()
    out.untouched()


# ---------------------------------------------------------------------------------- the ancestor search
def grid_population(n_centres, weights):
    """centre i sits at (i, -i); under the factor below theta_0 - theta_1 = 2 i + O(1e-3), so rint of half of it names the ancestor"""
    i = np.arange(n_centres, dtype=np.float32)
    return DevicePopulation(S.HostPopulation(np.stack([i, -i], axis=1), weights, bw=[1e-3, 1e-3]))


@pytest.mark.parametrize("n_centres", [1, 2, 1000, 4097])
def test_population_sizes_and_weights(hip, n_centres):
    model, n, row0 = model_of(("gauss", 2)), 300, ROW0S[1]
    L = F.dense_factor([1e-3, 1e-3], seed=1)
    rng = np.random.default_rng(n_centres)
    random = rng.random(n_centres).astype(np.float32)
    random[rng.random(n_centres) < 0.3] = 0.0
    random[n_centres // 2] = 0.5                                           # not all zero
    cases = [("uniform", None), ("random", random)]
    for hot in sorted({0, n_centres // 2, n_centres - 1}):
        one = np.zeros(n_centres, np.float32)
        one[hot] = 1.0
        cases.append(("one-hot %d" % hot, one))
    ids = np.arange(n, dtype=np.int64) + row0
    for name, w in cases:
        pop = grid_population(n_centres, w)
        got = call(hip, model, pop, L, row0, None, n, n + 5)
        assert_equals(got, restated(model, pop.host, L, ids), slice(None), "%d centres, %s weights" % (n_centres, name))
        ancestor = np.rint(0.5 * (got["theta"][:, 0].astype(np.float64) - got["theta"][:, 1])).astype(np.int64)
        assert (ancestor >= 0).all() and (ancestor < n_centres).all()
        assert (pop.host.weights[ancestor] > 0).all(), "a centre of weight 0 was chosen"
        # the ancestors are the diagonal kernel's: no random number moved
        same = call_diagonal(hip, model, pop, row0, None, n, n + 5, want=("theta",))["theta"]
        assert np.array_equal(ancestor, np.rint(same[:, 0]).astype(np.int64))
        if name.startswith("one-hot"):
            assert (ancestor == int(np.argmax(w))).all()
        elif n_centres >= 1000 and name == "uniform":
            assert np.unique(ancestor).size > min(n_centres, n) // 3        # the whole table is reached
            assert ancestor.min() < n_centres // 8 + 1 and ancestor.max() >= n_centres - n_centres // 8 - 1


# ---------------------------------------------------------------------------------- the density
def density_case(d, centre, spread, seed):
    rng = np.random.default_rng(seed)
    mix = rng.standard_normal((d, d)) * 0.5 + np.eye(d)
    X = (centre + spread * rng.standard_normal((1000, d)) @ mix.T).astype(np.float32)
    w = rng.random(1000) + 0.05
    return X, w / w.sum()


@pytest.mark.parametrize("d,centre,spread", [(2, 0.0, 1.0), (4, 0.0, 1.0), (8, 0.0, 1.0), (4, 1000.0, 0.01)], ids=["D2", "D4", "D8", "D4-near-1000"])
def test_whitened_density_against_the_float64_restatement(hip, d, centre, spread):
    X, w = density_case(d, centre, spread, d)
    theta, weights = dev(X), torch.from_numpy(w).cuda()
    L = smc.full_factor(theta, weights, "beaumont")
    kernel = smc._FullKernel(theta, weights, L, theta.device)
    rng = np.random.default_rng(d + 100)
    pts = (X[rng.integers(0, 1000, 512)].astype(np.float64) + rng.standard_normal((512, d)) @ np.float64(L).T).astype(np.float32)
    got = host(kernel.log_prob_soa(dev(np.ascontiguousarray(pts.T))))
    want = F.log_q(pts, X, w, L)
    assert got.dtype == np.float64 and np.isfinite(got).all()
    print("log q, D = %d, centres near %g: largest difference from float64 %.3g (values %.3g .. %.3g)"
          % (d, centre, np.abs(got - want).max(), want.min(), want.max()))
    assert np.abs(got - want).max() <= LOGQ_TOL
    # the draws' side of the same object: the particles as a glabc_kde with the marginal scales, the packed factor
    assert np.allclose(host(kernel.kde.bandwidth), np.sqrt((np.float64(L) ** 2).sum(axis=1)), rtol=1e-6) and list(kernel.chol) == list(F.pack(L))


# ---------------------------------------------------------------------------------- smc.draws and smc.sample
def test_draws_wrapper(hip):
    m = R.abs_gauss_model(3, distribution.DiagGaussian(3, torch.zeros(3), torch.zeros(3)), epsilon=0.7)
    rng = np.random.default_rng(5)
    X, w = rng.standard_normal((200, 3)).astype(np.float32), rng.random(200).astype(np.float32)
    kde = smc.KernelDensity("scott").fit(torch.from_numpy(X), torch.from_numpy(w))
    pop = S.HostPopulation(X, w, h=200 ** (-1.0 / 7.0))
    L = F.dense_factor([0.4, 0.3, 0.5], seed=2)
    ref = restated(m.descriptor(), pop, L, np.arange(100, 365))
    d = smc.draws(m, kde, 265, seed=SEED, row0=100, cholesky=torch.from_numpy(L))
    assert d.theta.shape == (265, 3) and d.y.shape == (265, 3) and d.accept.dtype == torch.uint8 and d.log_prior.shape == (265,)
    assert_equals({k: host(v) for k, v in d._asdict().items()}, ref, slice(None), "draws(cholesky=)")
    d = smc.draws(m, kde, 3, seed=SEED, ids=[364, 100, 364], want="theta", cholesky=L)
    assert np.array_equal(bits(host(d.theta)), bits(ref["theta"][[264, 0, 264]]))
    with pytest.raises(ValueError, match="cholesky"):
        smc.draws(m, kde, 3, seed=SEED, cholesky=L.T)
    with pytest.raises(ValueError, match="cholesky"):
        smc.draws(m, kde, 3, seed=SEED, cholesky=L[:2, :2])


def test_sample_does_not_depend_on_the_launch_size(hip, monkeypatch):
    model = Mixture_set(0.05)
    a = smc.sample(model, 512, kernel="model", seed=SEED, perturbation="full")
    monkeypatch.setattr(smc, "MIN_LAUNCH", 1)
    monkeypatch.setattr(rejection, "MAX_LAUNCH", 777)
    b = smc.sample(model, 512, kernel="model", seed=SEED, perturbation="full")
    assert a.generations == b.generations and a.epsilon == b.epsilon == 0.05 and a.ess == b.ess
    for x, y in ((a.theta, b.theta), (a.y, b.y), (a.distance, b.distance), (a.weights, b.weights)):
        assert torch.equal(x, y)
    assert all(np.float32(g["cholesky"]).shape == (2, 2) for g in a.generations[1:]) and "cholesky" not in a.generations[0]
    c = smc.sample(model, 512, kernel="model", seed=SEED)                  # the default stays the diagonal kernel
    assert all("cholesky" not in g for g in c.generations) and not torch.equal(a.theta, c.theta)
    assert a.generations[0] == c.generations[0]                            # generation 0 knows no perturbation


def test_first_full_generation_is_the_restated_loop(hip):
    model, N, q, stop = Mixture_set(0.05), 256, 0.5, 1.0
    p = smc.sample(model, N, kernel="hard", epsilon=stop, quantile=q, seed=SEED, perturbation="full")
    desc = model.descriptor()
    theta0, dis0, eps0, n0 = S.first_generation(desc, N, q, SEED)
    eps1 = S.next_epsilon(dis0, q, stop)
    assert eps1 < eps0 and len(p.generations) == 2
    g0, g1 = p.generations
    assert g0["epsilon"] == eps0 and g0["n_draws"] == n0 and g1["epsilon"] == eps1 == p.epsilon
    # the factor: Silverman's factor squared times the unbiased weighted covariance of generation 0, in float64, rounded to float32
    L = np.float32(g1["cholesky"])
    x = theta0.astype(np.float64)
    cov = np.cov(x.T, bias=True) / (1.0 - 1.0 / N) * smc.rule_factor("silverman", N, 2) ** 2
    assert np.allclose(L, np.linalg.cholesky(cov), rtol=1e-6, atol=0) and np.allclose(g1["bandwidth"], np.sqrt(np.diagonal(cov)), rtol=1e-6)
    pop = S.HostPopulation(theta0, np.full(N, 1.0 / N, np.float32), bw=np.float32(g1["bandwidth"]))
    ids, (theta, y, lp, dis, _) = F.hard_generation(desc, pop, L, N, eps1, SEED, 1, block=1024)
    assert g1["n_draws"] == ids[-1] + 1 and (dis <= np.float32(eps1)).all()
    assert np.array_equal(bits(host(p.theta)), bits(theta)) and np.array_equal(bits(host(p.y)), bits(y))
    assert np.array_equal(bits(host(p.distance)), bits(dis))
    # the weights: prior density over the restated float64 mixture density
    lw = lp.astype(np.float64) - F.log_q(theta, theta0, np.full(N, 1.0 / N), L)
    w = np.exp(lw - lw.max())
    assert np.allclose(host(p.weights), w / w.sum(), rtol=1e-4, atol=0)


def test_fused_full_kernel_samples_the_analytic_posterior(hip):
    N = 4096
    p = smc.sample(Mixture_set(0.05), N, kernel="model", seed=SEED, path="fused", perturbation="full")
    assert p.theta.shape == (N, 2) and not torch.isnan(p.weights).any() and p.ess > N / 4 and p.epsilon == 0.05
    rate, m2, _ = R.analytic(0.05)
    mu, se = S.weighted_second_moment(host(p.theta), host(p.weights))
    print("E theta_j^2 %r, analytic %.5f, %r SE; ess %.0f of %d" % (mu, m2, (mu - m2) / se, p.ess, N))
    assert (np.abs(mu - m2) <= 5.0 * se).all()


def test_run_time_compiled_entry_point_refuses_the_factor_where_the_built_in_does(hip):
    model = Correlated_smc.build()
    handle, desc = model.draws_program(), model.descriptor()
    rng = np.random.default_rng(9)
    kde = smc.KernelDensity("scott").fit(torch.from_numpy(rng.standard_normal((100, 2)).astype(np.float32)))
    L = F.dense_factor([0.4, 0.3], seed=4)
    good, zero, nan = F.pack(L), F.pack(L), F.pack(L)
    zero[2], nan[1] = 0.0, np.nan
    out = Guarded(1, 16)

    def f(chol, n=10, stride=16, pop=kde.descriptor()):
        rc = hip.glabc_rtc_smc_draws_full(handle, C.byref(desc), None if pop is None else C.byref(pop), None if chol is None else chol.ctypes.data,
                                          SEED, 0, None, n, stride, None, None, out.ptr, None, None, None)
        torch.cuda.synchronize()
        return rc
    assert f(None) == ERR_NULL and f(zero) == ERR_ARG and f(nan) == ERR_ARG
    assert f(None, stride=9) == ERR_NULL and f(zero, n=-1) == ERR_ARG and f(good, stride=9) == ERR_ARG          # the factor before the range
    assert f(zero, pop=None) == ERR_NULL                                   # ... and behind the population
    out.untouched()
    assert f(good) == 0
    want = smc.draws(model, kde, 10, seed=SEED, want="distance", cholesky=L).distance
    assert np.array_equal(bits(out.read(10)[0]), bits(host(want)))
    # the same population and factor under the diagonal entry point give other draws: the factor is read
    assert not np.array_equal(bits(host(smc.draws(model, kde, 10, seed=SEED, want="distance").distance)), bits(host(want)))


def test_correlated_compiled_model(hip):
    N = 2000
    model = Correlated_smc.build()
    handle = model.draws_program()                                         # compiled, and self-checked before it is handed out
    assert (model.DRAWS,) in model._checked and model.self_check_draws(handle) is True
    mean, cov = F.correlated_posterior()
    runs = {}
    for name in ("full", "diagonal"):
        p = smc.sample(model, N, kernel="model", bandwidth="beaumont", seed=SEED, path="fused", perturbation=name)
        m, c, se_m, se_c = F.weighted_moments(host(p.theta), host(p.weights))
        runs[name] = sum(g["n_draws"] for g in p.generations)
        print("%s: %d simulations, %d generations, ess %.0f; mean %r (%r SE), covariance %r (%r SE)"
              % (name, runs[name], len(p.generations), p.ess, m, (m - mean) / se_m, c.tolist(), ((c - cov) / se_c).tolist()))
        assert p.theta.is_cuda and p.epsilon == 0.05 and p.ess > N / 4
        assert (np.abs(m - mean) <= 5.0 * se_m).all() and (np.abs(c - cov) <= 5.0 * se_c).all()
    assert 2 * runs["full"] <= runs["diagonal"], runs
