"""glabc_smc_draws (csrc/glabc_smc.hip) and glabcmcmc_amd.smc on the GPU.

Bit for bit: the fused kernel against (a) the on-device composition of the entry points it fuses -- glabc_kde_sample -> transpose ->
glabc_model_prior_log_prob -> glabc_model_simulate(eps = NULL, seed ^ GLABC_ABC_NOISE_KEY) -> glabc_model_discrepancy ->
where(log_prior == -inf, inf, distance) -- and (b) the restatement from the CPU checker's functions (tests/smc_ref.py), the
acceptance included, on |theta| + noise at every theta_dim 1 .. 8 with a DiagGaussian and with a Uniform prior and on g-and-k.
Shapes: n around the wavefront (64) and the workgroup (256: one draw per lane), row0 across the counter's low word and past it, a
list of ids out of order with a repeat and a value >= 2^32, stride = n + 5, each output alone, n = 0, the refusals; populations of
1 .. 4097 centres with uniform, random (exact zeros) and one-hot weights.  Every buffer lies between guard bands of canaries, and
the padding columns n .. stride - 1 must keep theirs.

The Uniform-prior populations have a bandwidth of 1.5 around centres inside the support, so that the restated draws hold rows
inside and rows outside it (asserted): the +inf rule is exercised at every theta_dim.  The g-and-k population stays inside the
support, where the simulator is finite.

smc.sample: the same call under two launch sizes, the first generation's ids against the restated loop, the law of the fused
path against the analytic posterior of Mixture_set (5 standard errors, tests/test_smc_host.py).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import rejection_ref as R
import smc_ref as S
from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import distribution, rejection, smc
from glabcmcmc_amd.examples.Mixture import Mixture_set
from helpers import bits, canary_left, dev, host
from test_rejection_shapes import ERR_ARG, ERR_DIM, ERR_KIND, ERR_NULL, MODELS, ROW0S, SEED, Guarded, model_of

pytestmark = pytest.mark.gpu

N_REF = 1000
SIZES = (1, 63, 64, 65, 255, 256, 257, 513, 1000)
NAMES = ("theta", "y", "distance", "log_prior", "accept")


class DevicePopulation:
    """a smc_ref.HostPopulation and its glabc_kde over device copies of the same arrays"""

    def __init__(self, hostpop):
        self.host = hostpop
        self.x, self.log_w, self.cum_q = dev(hostpop.xs), dev(hostpop.log_w), dev(hostpop.cum_q)
        k = A.Kde()
        k.dim, k.n_samples = hostpop.dim, hostpop.S
        k.x, k.log_w, k.cum_q = self.x.data_ptr(), self.log_w.data_ptr(), self.cum_q.data_ptr()
        for j in range(hostpop.dim):
            k.bandwidth[j] = float(hostpop.consts[j])
        k.sum_log_bw, k.c_2pi = float(hostpop.consts[hostpop.dim]), float(hostpop.consts[hostpop.dim + 1])
        self.struct = k


@functools.lru_cache(maxsize=None)
def population_of(key):
    """1000 centres with random weights holding exact zeros; Uniform priors: centres inside the support, bandwidth 1.5"""
    kind, d = key
    rng = np.random.default_rng(100 + d)
    w = rng.random(1000).astype(np.float32)
    w[rng.random(1000) < 0.1] = 0.0
    if kind == "gk":
        X = np.array([3.0, 1.0, 2.0, 0.5], np.float32) + 0.05 * rng.standard_normal((1000, 4)).astype(np.float32)
        return DevicePopulation(S.HostPopulation(X, w, bw=[0.05, 0.02, 0.05, 0.02]))
    X = rng.uniform(-1.5, 1.5, (1000, d)).astype(np.float32)
    if kind == "uniform":
        return DevicePopulation(S.HostPopulation(X, w, bw=[1.5] * d))
    return DevicePopulation(S.HostPopulation(X, w, h=0.7))


def restated(model, hostpop, ids):
    """smc_ref.restate under SEED -> {name: array}"""
    theta, y, lp, dis, acc = S.restate(model, hostpop, SEED, ids)
    return {"theta": theta, "y": y, "distance": dis, "log_prior": lp, "accept": acc}


@functools.lru_cache(maxsize=None)
def reference(key, row0):
    """the restated draws row0 .. row0 + N_REF - 1 of a Model and its population: computed once, never modified"""
    out = restated(model_of(key), population_of(key).host, np.arange(N_REF, dtype=np.int64) + row0)
    for a in out.values():
        a.setflags(write=False)
    return out


def call(hip, model, pop, row0, ids, n, stride, want=NAMES, seed=SEED, expect=0):
    """one glabc_smc_draws call into guarded buffers -> {name: host array}; theta / y come back as [n][dim]"""
    buf = {"theta": Guarded(model.theta_dim, stride), "y": Guarded(model.y_dim, stride), "distance": Guarded(1, stride),
           "log_prior": Guarded(1, stride), "accept": Guarded(1, stride, u8=True)}
    idt = None if ids is None else dev(np.asarray(ids, np.int64))
    p = lambda name: buf[name].ptr if name in want else None          # noqa: E731
    rc = hip.glabc_smc_draws(C.byref(model), None if pop is None else C.byref(pop.struct), seed, row0, None if idt is None else idt.data_ptr(),
                             n, stride, p("theta"), p("y"), p("distance"), p("log_prior"), p("accept"), None)
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


def composed(hip, model, pop, row0, n):
    """the twin: the parent commit's entry points, theta and y through device memory"""
    d, yd = model.theta_dim, model.y_dim
    z = torch.empty(d, n, device="cuda")
    assert hip.glabc_kde_sample(C.byref(pop.struct), n, SEED, row0, z.data_ptr(), None) == 0
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
    model, pop = model_of(key), population_of(key)
    for row0 in ROW0S:
        ref = reference(key, row0)
        if key[0] == "uniform":                                            # both classes occur, so the +inf rule is under test
            outside = np.isinf(ref["log_prior"])
            assert 20 < outside.sum() < N_REF - 20 and np.isinf(ref["distance"][outside]).all() and np.isfinite(ref["distance"][~outside]).all()
            assert not ref["accept"][outside].any() and np.isfinite(ref["y"]).all()
        got = call(hip, model, pop, row0, None, N_REF, N_REF + 5)
        assert_equals(got, ref, slice(None), "%r row0 %d" % (key, row0))
        twin = composed(hip, model, pop, row0, N_REF)
        for name, want in twin.items():
            assert np.array_equal(bits(got[name]), bits(want)), "%r row0 %d: %s differs from the composed entry points" % (key, row0, name)
        # both outcomes occur (the g-and-k population sits at the observed parameters, far inside its epsilon: all may be kept)
        assert got["accept"].any() and (key[0] == "gk" or not got["accept"].all())


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_wavefront_and_the_workgroup(hip, n):
    for key in (("gauss", 2), ("uniform", 5), ("gk", 4)):
        for row0 in ROW0S[:2]:
            got = call(hip, model_of(key), population_of(key), row0, None, n, n + 5)
            assert_equals(got, reference(key, row0), slice(0, n), "%r n %d" % (key, n))
    got = call(hip, model_of(("gauss", 2)), population_of(("gauss", 2)), 0, None, n, n)          # no padding column
    assert_equals(got, reference(("gauss", 2), 0), slice(0, n), "stride = n")


@pytest.mark.parametrize("key", [("gauss", 1), ("uniform", 3), ("gauss", 8), ("gk", 4)], ids=lambda k: "%s%d" % k)
def test_listed_ids(hip, key):
    model, pop = model_of(key), population_of(key)
    base = 2 ** 32 - 3
    ids = np.array([base + 700, 5, base + 2, 5, 2 ** 40 + 999, 0, base + 3, 999, base + 2], np.int64)          # unsorted, repeats, >= 2^32
    got = call(hip, model, pop, 0, ids, ids.size, ids.size + 5)
    assert_equals(got, restated(model, pop.host, ids), slice(None), "ids")
    n = 300                                                                # more than a workgroup of listed ids, permuted
    perm = np.random.default_rng(1).permutation(n).astype(np.int64) + base
    got = call(hip, model, pop, 0, perm, n, n + 5)
    assert_equals(got, reference(key, base), perm - base, "permuted ids")


@pytest.mark.parametrize("key", [("gauss", 2), ("uniform", 7), ("gk", 4)], ids=lambda k: "%s%d" % k)
def test_each_output_alone_gives_the_same_bits(hip, key):
    model, pop, n, row0 = model_of(key), population_of(key), 257, ROW0S[1]
    ref = reference(key, row0)
    for want in (("theta",), ("y",), ("distance",), ("log_prior",), ("accept",), ("theta", "accept"), ("y", "log_prior"), ("y", "distance")):
        got = call(hip, model, pop, row0, None, n, n + 5, want=want)       # call() checks that the other buffers keep their canaries
        assert set(got) == set(want)
        assert_equals(got, ref, slice(0, n), "want %r" % (want,))


def test_nothing_is_written_for_n_0_and_by_a_refused_call(hip):
    key = ("gauss", 2)
    model, pop = model_of(key), population_of(key)
    assert call(hip, model, pop, 0, None, 0, 0) == {} and call(hip, model, pop, 7, None, 0, 5) == {} and call(hip, model, pop, 0, [], 0, 0) == {}
    call(hip, model, pop, 0, None, 10, 9, expect=ERR_ARG)
    call(hip, model, pop, -1, None, 10, 10, expect=ERR_ARG)
    call(hip, model, pop, 3, [1, 2, 3], 3, 3, expect=ERR_ARG)
    call(hip, model, pop, 0, None, -1, 10, expect=ERR_ARG)
    call(hip, model, pop, 0, None, 10, 10, want=(), expect=ERR_NULL)
    call(hip, model, None, 0, None, 10, 10, expect=ERR_NULL)
    user = model_of(key)
    user.sim_kind = A.SIM_USER
    call(hip, user, pop, 0, None, 10, 10, expect=ERR_KIND)
    gamma = Mixture_set(0.05, prior=distribution.Gamma(torch.tensor([2.0, 2.0]), torch.tensor([1.0, 1.0]))).descriptor()
    call(hip, gamma, pop, 0, None, 10, 10, expect=ERR_KIND)
    odd = model_of(key)
    odd.y_dim = 3
    call(hip, odd, pop, 0, None, 10, 10, expect=ERR_DIM)
    call(hip, model, population_of(("gauss", 3)), 0, None, 10, 10, expect=ERR_DIM)          # a population of another dimension
    for spoil, want in ((lambda k: setattr(k, "cum_q", None), ERR_NULL), (lambda k: setattr(k, "x", None), ERR_NULL),
                        (lambda k: setattr(k, "n_samples", 0), ERR_ARG), (lambda k: k.bandwidth.__setitem__(1, 0.0), ERR_ARG)):
        bad = DevicePopulation(pop.host)
        spoil(bad.struct)
        call(hip, model, bad, 0, None, 10, 10, expect=want)


# ---------------------------------------------------------------------------------- the ancestor search
def grid_population(n_centres, weights):
    """centre i sits at (i, -i) under a kernel of width 1e-3: rint(theta_0) names a draw's ancestor"""
    i = np.arange(n_centres, dtype=np.float32)
    return DevicePopulation(S.HostPopulation(np.stack([i, -i], axis=1), weights, bw=[1e-3, 1e-3]))


@pytest.mark.parametrize("n_centres", [1, 2, 63, 64, 65, 1000, 4097])
def test_population_sizes_and_weights(hip, n_centres):
    model, n, row0 = model_of(("gauss", 2)), 300, ROW0S[1]
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
        got = call(hip, model, pop, row0, None, n, n + 5)
        assert_equals(got, restated(model, pop.host, ids), slice(None),
                      "%d centres, %s weights" % (n_centres, name))
        ancestor = np.rint(got["theta"][:, 0]).astype(np.int64)
        assert (ancestor >= 0).all() and (ancestor < n_centres).all() and np.array_equal(np.rint(got["theta"][:, 1]).astype(np.int64), -ancestor)
        assert (pop.host.weights[ancestor] > 0).all(), "a centre of weight 0 was chosen"
        if name.startswith("one-hot"):
            hot = int(np.argmax(w))
            # theta minus its noise term is that centre: the draws of the one-centre population, shifted by it, bit for bit
            alone = call(hip, model, grid_population(1, None), row0, None, n, n, want=("theta",))["theta"]
            assert (ancestor == hot).all()
            assert np.array_equal(bits(got["theta"]), bits(np.float32([hot, -hot]) + alone))
        elif n_centres >= 63 and name == "uniform":
            assert np.unique(ancestor).size > min(n_centres, n) // 3        # the whole table is reached
            assert ancestor.min() < n_centres // 8 + 1 and ancestor.max() >= n_centres - n_centres // 8 - 1


# ---------------------------------------------------------------------------------- smc.draws and smc.sample
def test_draws_wrapper(hip):
    m = R.abs_gauss_model(3, distribution.DiagGaussian(3, torch.zeros(3), torch.zeros(3)), epsilon=0.7)
    rng = np.random.default_rng(5)
    X, w = rng.standard_normal((200, 3)).astype(np.float32), rng.random(200).astype(np.float32)
    kde = smc.KernelDensity("scott").fit(torch.from_numpy(X), torch.from_numpy(w))
    pop = S.HostPopulation(X, w, h=200 ** (-1.0 / 7.0))
    assert np.array_equal(bits(host(kde.bandwidth)), bits(pop.bandwidth))
    ref = restated(m.descriptor(), pop, np.arange(100, 365))
    d = smc.draws(m, kde, 265, seed=SEED, row0=100)
    assert d.theta.shape == (265, 3) and d.y.shape == (265, 3) and d.distance.shape == (265,) and d.accept.dtype == torch.uint8
    assert d.theta.is_cuda and d.theta.t().is_contiguous() and d.log_prior.shape == (265,)
    assert_equals({k: host(v) for k, v in d._asdict().items()}, ref, slice(None), "draws()")
    d = smc.draws(m, kde, 3, seed=SEED, ids=[364, 100, 364], want="distance", epsilon=0.1)
    assert d.theta is None and d.y is None and d.accept is None and d.log_prior is None
    assert np.array_equal(bits(host(d.distance)), bits(ref["distance"][[264, 0, 264]]))
    assert smc.draws(m, kde, 0, seed=SEED).theta.shape == (0, 3)
    with pytest.raises(ValueError, match="features"):
        smc.draws(Mixture_set(0.05), kde, 4, seed=SEED)


def test_sample_does_not_depend_on_the_launch_size(hip, monkeypatch):
    model = Mixture_set(0.05)
    a = smc.sample(model, 512, kernel="model", seed=SEED)
    monkeypatch.setattr(smc, "MIN_LAUNCH", 1)
    monkeypatch.setattr(rejection, "MAX_LAUNCH", 777)
    b = smc.sample(model, 512, kernel="model", seed=SEED)
    assert a.generations == b.generations and a.epsilon == b.epsilon == 0.05 and a.ess == b.ess
    for x, y in ((a.theta, b.theta), (a.y, b.y), (a.distance, b.distance), (a.weights, b.weights)):
        assert torch.equal(x, y)
    assert a.theta.is_cuda and a.weights.dtype == torch.float64 and abs(float(a.weights.sum()) - 1.0) < 1e-12
    c = smc.sample(model, 512, kernel="model", seed=SEED + 1)
    assert not torch.equal(a.theta, c.theta)


def test_first_generation_is_the_restated_loop(hip):
    model, N, q, stop = Mixture_set(0.05), 256, 0.5, 1.0
    p = smc.sample(model, N, kernel="hard", epsilon=stop, quantile=q, seed=SEED)
    desc = model.descriptor()
    theta0, dis0, eps0, n0 = S.first_generation(desc, N, q, SEED)
    eps1 = S.next_epsilon(dis0, q, stop)
    assert eps1 < eps0 and len(p.generations) == 2                         # generation 1 reaches the stop
    g0, g1 = p.generations
    assert g0["epsilon"] == eps0 and g0["n_draws"] == n0 and g1["epsilon"] == eps1 == p.epsilon
    pop = S.silverman_population(theta0, np.full(N, 1.0 / N))
    assert np.array_equal(bits(np.float32(g1["bandwidth"])), bits(pop.bandwidth))
    ids, (theta, y, lp, dis, _) = S.hard_generation(desc, pop, N, eps1, SEED, 1, block=1024)
    assert g1["n_draws"] == ids[-1] + 1 and (dis <= np.float32(eps1)).all()
    assert np.array_equal(bits(host(p.theta)), bits(theta)) and np.array_equal(bits(host(p.y)), bits(y))
    assert np.array_equal(bits(host(p.distance)), bits(dis))


def test_fused_model_kernel_samples_the_analytic_posterior(hip):
    N = 4096
    p = smc.sample(Mixture_set(0.05), N, kernel="model", seed=SEED, path="fused")
    assert p.theta.shape == (N, 2) and not torch.isnan(p.weights).any() and p.ess > N / 4 and p.epsilon == 0.05
    rate, m2, _ = R.analytic(0.05)
    mu, se = S.weighted_second_moment(host(p.theta), host(p.weights))
    sims = sum(g["n_draws"] for g in p.generations)
    print("E theta_j^2 %r, analytic %.5f, %r SE; ess %.0f of %d; %d simulations against %.0f of plain rejection"
          % (mu, m2, (mu - m2) / se, p.ess, N, sims, N / rate))
    assert (np.abs(mu - m2) <= 5.0 * se).all() and sims <= 0.5 * N / rate
    # a Uniform prior whose support cuts through the posterior: no particle outside it, every weight finite
    prior = distribution.Uniform(2, torch.tensor([-2.0, -2.0]), torch.tensor([2.5, 2.5]))
    u = smc.sample(R.abs_gauss_model(2, prior, epsilon=0.05, y_obs=[1.5, 1.5]), 1024, kernel="model", seed=SEED)
    assert (u.theta >= -2.0).all() and (u.theta <= 2.5).all() and torch.isfinite(u.weights).all() and torch.isfinite(u.distance).all()
