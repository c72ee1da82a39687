"""ABC-SMC on the CPU: the refusals of glabc_smc_draws as csrc/glabc_check.h answers them under g++, the compiler's resource
report of its kernels, every ValueError and RuntimeError of glabcmcmc_amd.smc, the restatement (tests/smc_ref.py) -- that a draw
depends on (model, population, seed, id) alone and that the prior's support rules the distance --, and the law of the generic
path on CPU tensors.

Law checks.  The particles of the last generation are independent given the previous one, so the standard error of the
self-normalised estimate of E theta_j^2 is sqrt(sum w_i^2 (f_i - mean)^2); the bound is 5 of them against the analytic
posterior of Mixture_set (tests/rejection_ref.py).  The simulations of a whole run must be at most half of what plain
rejection needs for the same number of accepted draws, N / analytic acceptance rate.
"""
import os
import re

import numpy as np
import pytest
import torch

import rejection_ref as R
import smc_ref as S
from glabcmcmc_amd import _capi, distribution, rejection, smc
from glabcmcmc_amd.examples.Mixture import Mixture_set
from test_arg_checks import check_table

OK, NULL, DIM, KIND, ARG = 0, -1, -2, -3, -4
SEED = 20261020


def std_prior(d=2):
    return distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d))


# ---------------------------------------------------------------------------------- the refusals (csrc/glabc_check.h)
def test_check_smc_draws(tmp_path_factory):
    prelude = ("static const int64_t IDS[4] = {3, 1, 3, 1ll << 40}; static uint8_t ACC[4]; static int64_t CUM[4] = {1, 2, 3, 4}; "
               "glabc_kde k; std::memset(&k, 0, sizeof k); k.dim = 3; k.n_samples = 4; k.x = b.f; k.log_w = b.f; k.cum_q = CUM; "
               "for (int j = 0; j < 8; ++j) k.bandwidth[j] = 0.5f; ")
    call = "check_smc_draws(%s, %s, %s, %s, %s, %s, %s, %s, %s, %s, %s)"
    base = dict(m="&b.m", k="&k", row0="0", ids="nullptr", n="65", stride="65", th="b.f", y="b.f", d="b.f", lp="b.f", a="ACC")

    def row(want, spoil="", **kw):
        a = dict(base, **kw)
        return (prelude + spoil, call % (a["m"], a["k"], a["row0"], a["ids"], a["n"], a["stride"], a["th"], a["y"], a["d"], a["lp"], a["a"]), want)
    none = dict(th="nullptr", y="nullptr", d="nullptr", lp="nullptr", a="nullptr")
    gk = "make_gk(b); k.dim = 4; "
    check_table(tmp_path_factory, "smc_draws", [
        row(OK), row(OK, "b.m.prior = dist3(GLABC_DIST_DIAG_GAUSS); "), row(OK, gk), row(OK, n="0", stride="0"), row(OK, stride="70"),
        row(OK, row0="1ll << 40"), row(OK, ids="IDS", n="4", stride="4"), row(OK, "k.n_samples = 1; "),
        row(OK, **dict(none, d="b.f")), row(OK, **dict(none, a="ACC")), row(OK, **dict(none, th="b.f")), row(OK, **dict(none, y="b.f")),
        row(OK, **dict(none, lp="b.f")),
        row(OK, "b.m.theta_dim = b.m.y_dim = b.m.prior.dim = k.dim = 8; "), row(OK, "b.m.theta_dim = b.m.y_dim = b.m.prior.dim = k.dim = 1; "),
        row(OK, "b.m.prior.p2[0] = NaN; b.m.kern_scale = 0.0f; "),           # the Model's values are not examined
        # NULL first: the Model, the population, all five outputs
        row(NULL, m="nullptr"), row(NULL, k="nullptr"), row(NULL, **none), row(NULL, "b.m.theta_dim = 9; ", **none),
        row(NULL, "k.dim = 0; ", k="nullptr", n="-1"), row(NULL, "b.m.sim_kind = GLABC_SIM_USER; ", k="nullptr"),
        # the Model as glabc_abc_draws refuses it, ahead of the population
        row(DIM, "b.m.theta_dim = 0; "), row(DIM, "b.m.theta_dim = b.m.y_dim = 9; "), row(DIM, "b.m.y_dim = 4; "),
        row(DIM, "make_gk(b); b.m.y_dim = 7; k.dim = 4; "), row(DIM, "b.m.y_dim = 4; k.x = nullptr; "),
        row(KIND, "b.m.sim_kind = GLABC_SIM_USER; "), row(KIND, "b.m.prior = dist3(GLABC_DIST_GAMMA); "), row(KIND, "b.m.prior.dim = 2; "),
        row(KIND, "b.m.sim_kind = 7; k.n_samples = 0; "), row(KIND, "b.m.prior.kind = 5; k.cum_q = nullptr; ", n="-1"),
        # the population: kde_check, then cum_q, then its dimension
        row(DIM, "k.dim = 0; "), row(DIM, "k.dim = 9; "), row(ARG, "k.n_samples = 0; "), row(ARG, "k.n_samples = -5; k.x = nullptr; "),
        row(NULL, "k.x = nullptr; "), row(NULL, "k.log_w = nullptr; "), row(NULL, "k.log_w = nullptr; k.bandwidth[0] = 0.0f; "),
        row(ARG, "k.bandwidth[0] = 0.0f; "), row(ARG, "k.bandwidth[2] = -1.0f; "), row(ARG, "k.bandwidth[1] = NaN; "),
        row(ARG, "k.bandwidth[1] = INFINITY; "), row(OK, "k.bandwidth[3] = 0.0f; "),          # past dim: not read
        row(ARG, "k.bandwidth[0] = 0.0f; k.cum_q = nullptr; "), row(NULL, "k.cum_q = nullptr; "), row(NULL, "k.cum_q = nullptr; k.dim = 2; "),
        row(DIM, "k.dim = 2; "), row(DIM, "k.dim = 4; "), row(DIM, gk + "k.dim = 3; "), row(DIM, "k.dim = 2; ", n="-1"),
        # the range of draws last
        row(ARG, n="-1"), row(ARG, stride="64"), row(ARG, row0="-1"), row(ARG, ids="IDS", row0="1", n="4", stride="4"),
        row(ARG, n="-1", stride="-1"),
    ])


def test_check_abc_draws_answers_as_before(tmp_path_factory):
    """check_abc_draws now shares its Model and range checks with check_smc_draws: the order of its refusals is unchanged"""
    call = "check_abc_draws(&b.m, %s, nullptr, %s, %s, b.f, nullptr, nullptr, nullptr)"
    check_table(tmp_path_factory, "abc_draws_order", [
        ("", call % ("0", "65", "65"), OK),
        ("b.m.theta_dim = 9; b.m.sim_kind = GLABC_SIM_USER; ", call % ("0", "-1", "65"), DIM),
        ("b.m.sim_kind = GLABC_SIM_USER; ", call % ("-1", "65", "65"), KIND),
        ("b.m.prior.dim = 2; ", call % ("0", "65", "64"), KIND),
        ("", call % ("0", "65", "64"), ARG),
        ("", "check_abc_draws(nullptr, 0, nullptr, -1, 0, b.f, nullptr, nullptr, nullptr)", NULL),
        ("b.m.theta_dim = 9; ", "check_abc_draws(&b.m, 0, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr)", NULL),
    ])


def test_entry_point_is_bound_and_exported():
    import glabcmcmc_amd
    assert "glabc_smc_draws" in _capi.ENTRY_POINTS and _capi.VERSION == 301 and _capi.STREAM_LAYOUT == 2
    assert len(_capi.ENTRY_POINTS["glabc_smc_draws"][1]) == 13
    assert glabcmcmc_amd.smc is smc and "smc" in glabcmcmc_amd.__all__ and smc.SEED_STEP == S.SEED_STEP
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glabc.h")).read()
    assert "int glabc_smc_draws(const glabc_model* model, const glabc_kde* population, uint64_t seed, int64_t row0" in header
    assert _capi.lib().glabc_smc_draws(None, None, 0, 0, None, 0, 0, None, None, None, None, None, None) == NULL       # resolves, and refuses
    m, k = Mixture_set(0.05).descriptor(), _capi.Kde()
    assert _capi.lib().glabc_smc_draws(m, k, 0, 0, None, 0, 0, 8, None, None, None, None, None) == DIM                 # an empty population


def test_resource_report_shows_no_private_segment():
    """profiles/smc_kernel_resources.txt: nine instantiations of smc_draws_kernel, none with a private segment or a spill"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "profiles", "smc_kernel_resources.txt")).read()
    kernels = re.split(r"^Function Name: ", text, flags=re.M)[1:]
    assert len(kernels) == 9 and all("smc_draws_kernel" in k for k in kernels)
    shapes = sorted(tuple(int(x) for x in re.search(r"smc_draws_kernelILi(\d)ELi(\d)E", k).groups()) for k in kernels)
    assert shapes == sorted([(d, d) for d in range(1, 9)] + [(4, 8)])
    for k in kernels:
        field = lambda name: int(re.search(r"%s: (\d+)" % re.escape(name), k).group(1))          # noqa: E731
        assert field("ScratchSize [bytes/lane]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0
        assert field("Occupancy [waves/SIMD]") >= 8 and field("LDS Size [bytes/block]") == 0


# ---------------------------------------------------------------------------------- the restatement
def small_population(d=2, n=50, seed=1, bw=None):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d)).astype(np.float32)
    w = rng.random(n).astype(np.float32)
    w[::7] = 0.0
    return S.HostPopulation(X, w, h=None if bw is not None else 0.5, bw=bw)


def test_restated_draw_depends_on_seed_and_id_alone():
    model, pop = Mixture_set(0.05).descriptor(), small_population()
    th, y, lp, dis, acc = S.restate(model, pop, SEED, np.arange(40, 140))
    for ids in (np.arange(100, 110), np.array([139, 40, 77, 77, 41]), np.array([77]), np.array([2 ** 32 - 1, 41, 2 ** 40 + 3])):
        inside = ids < 140
        t2, y2, l2, d2, a2 = S.restate(model, pop, SEED, ids)
        for got, want in ((t2, th), (y2, y), (l2, lp), (d2, dis)):
            assert np.array_equal(got[inside].view(np.uint32), want[ids[inside] - 40].view(np.uint32))
        assert np.array_equal(a2[inside], acc[ids[inside] - 40])
    assert not np.array_equal(S.restate(model, pop, SEED + 1, np.arange(40, 140))[0], th)
    # under a narrow kernel the nearest centre is the ancestor: never one of weight 0
    narrow = small_population(bw=[1e-3, 1e-3])
    th = S.restate(model, narrow, SEED, np.arange(300))[0]
    nearest = np.argmin(((th[:, None, :] - narrow.X[None, :, :]) ** 2).sum(axis=2), axis=1)
    assert (narrow.weights == 0).sum() == 8 and (narrow.weights[nearest] > 0).all() and np.unique(nearest).size > 30


def test_restated_distance_is_infinite_outside_the_support():
    prior = distribution.Uniform(2, torch.tensor([-2.0, -2.0]), torch.tensor([2.5, 2.5]))
    model = R.abs_gauss_model(2, prior, epsilon=0.5).descriptor()
    th, y, lp, dis, acc = S.restate(model, small_population(bw=[1.5, 1.5]), SEED, np.arange(500))
    outside = ((th < -2.0) | (th > 2.5)).any(axis=1)
    assert 50 < outside.sum() < 450
    assert np.isinf(lp[outside]).all() and np.isinf(dis[outside]).all() and (dis[outside] > 0).all() and not acc[outside].any()
    assert np.isfinite(lp[~outside]).all() and np.isfinite(dis[~outside]).all() and np.isfinite(y).all() and acc.any()


# ---------------------------------------------------------------------------------- arguments
class Stub:
    """a callback Model no fused path takes"""
    epsilon, theta_dim, y_dim = 0.3, 1, 1

    def generate_samples(self, theta, num_samples=1):
        return theta.clone()

    def discrepancy(self, y):
        return y.view(-1).abs()

    def calculate_log_kernel_dis(self, dis, epsilon=None):
        return -0.5 * (dis / (self.epsilon if epsilon is None else epsilon)) ** 2


def test_value_errors():
    m, p = Mixture_set(0.05), std_prior()
    gen = dict(path="generic", prior=p)
    T = smc.sample
    bad_calls = [
        lambda: T(m, 1, **gen), lambda: T(m, 0, **gen), lambda: T(m, 2.5, **gen), lambda: T(m, True, **gen),
        lambda: T(m, 64, kernel="soft", **gen), lambda: T(m, 64, path="quick", prior=p),
        lambda: T(m, 64, kernel="hard", **gen),                                              # neither epsilon nor a ladder
        lambda: T(m, 64, kernel="hard", epsilon=0.5, epsilons=[1.0, 0.5], **gen),
        lambda: T(m, 64, epsilon=0.0, **gen), lambda: T(m, 64, epsilon=-1.0, **gen), lambda: T(m, 64, epsilon=float("nan"), **gen),
        lambda: T(m, 64, epsilon="wide", **gen),
        lambda: T(m, 64, epsilons=[], **gen), lambda: T(m, 64, epsilons=[1.0, 1.0], **gen), lambda: T(m, 64, epsilons=[0.5, 1.0], **gen),
        lambda: T(m, 64, epsilons=[1.0, 0.0], **gen), lambda: T(m, 64, epsilons=[1.0, float("nan")], **gen), lambda: T(m, 64, epsilons=0.5, **gen),
        lambda: T(m, 64, epsilons=["a"], **gen),
        lambda: T(m, 64, quantile=0.0, **gen), lambda: T(m, 64, quantile=1.5, **gen), lambda: T(m, 64, quantile="half", **gen),
        lambda: T(m, 64, quantile=float("nan"), **gen),
        lambda: T(m, 64, bandwidth="wide", **gen), lambda: T(m, 64, bandwidth=0.0, **gen), lambda: T(m, 64, bandwidth=[0.1, -0.1], **gen),
        lambda: T(m, 64, bandwidth=[0.1, 0.1, 0.1], **gen), lambda: T(m, 64, bandwidth=float("inf"), **gen), lambda: T(m, 64, bandwidth=None, **gen),
        lambda: T(m, 64, max_generations=0, **gen), lambda: T(m, 64, max_draws=0, **gen), lambda: T(m, 64, max_draws=1.5, **gen),
        lambda: T(m, 64, path="generic"), lambda: T(m, 64, path="generic", prior=object()),
        lambda: T(m, 64, path="generic", prior=type("P", (), {"forward": lambda self, n: None})()),       # no log_prob
        lambda: T(Stub(), 64, path="fused"), lambda: T(Stub(), 64, path="auto"),               # auto falls to generic, which needs prior=
        lambda: T(Mixture_set(0.0), 64, **gen),                                               # the Model's own epsilon
        lambda: smc.draws(m, None, -1, seed=1), lambda: smc.draws(m, None, 4, seed=None), lambda: smc.draws(m, None, 4, seed=1.0),
        lambda: smc.draws(m, None, 4, seed=1, row0=-1), lambda: smc.draws(m, None, 4, seed=1, want=()),
        lambda: smc.draws(m, None, 4, seed=1, want=("theta", "weights")), lambda: smc.draws(m, None, 4, seed=1, epsilon=0.0),
        lambda: smc.draws(Stub(), None, 4, seed=1), lambda: smc.draws(m, None, 4, seed=1), lambda: smc.draws(m, "kde", 4, seed=1),
        lambda: smc.draws(m, smc.KernelDensity(), 4, seed=1),                                 # not fitted
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d raised nothing" % i)
    with pytest.raises(ValueError, match="strictly decreasing"):
        T(m, 64, epsilons=[1.0, 0.5, 0.5], **gen)
    with pytest.raises(ValueError, match="soft"):
        T(m, 64, kernel="soft", **gen)
    if not torch.cuda.is_available():                                      # the fused path never computes on the host
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            T(m, 64)


def test_runtime_errors():
    m, gen = Mixture_set(0.05), dict(path="generic", prior=std_prior())
    torch.manual_seed(1)
    with pytest.raises(RuntimeError, match=r"max_generations = 2 reached.*ladder so far: \d"):
        smc.sample(m, 256, max_generations=2, **gen)
    with pytest.raises(RuntimeError, match=r"max_generations = 1 reached"):       # the soft generation counts
        smc.sample(m, 256, epsilon=1.0, max_generations=1, **gen)
    with pytest.raises(RuntimeError, match=r"does not decrease.*ladder so far"):   # quantile 1: the tolerance is the largest distance again
        smc.sample(m, 256, quantile=1.0, **gen)
    with pytest.raises(RuntimeError, match=r"does not decrease"):                  # a ladder that starts above generation 0's tolerance
        smc.sample(m, 256, kernel="hard", epsilons=[50.0, 0.5], **gen)
    with pytest.raises(RuntimeError, match=r"generation 1 kept \d+ of the 256 particles in max_draws = 300 draws \(acceptance rate"):
        smc.sample(m, 256, kernel="hard", epsilon=0.05, max_draws=300, **gen)

    class Flat(Stub):                                                       # every particle of generation 0 has the same theta
        theta_dim = 2

        def generate_samples(self, theta, num_samples=1):
            return torch.rand(theta.shape[0], 1)

    class Point:
        def forward(self, n):
            return torch.cat([torch.randn(n, 1), torch.full((n, 1), 0.25)], dim=1), torch.zeros(n)

        def log_prob(self, z):
            return torch.zeros(z.shape[0])

    with pytest.raises(RuntimeError, match="degenerate: the bandwidth of coordinate 1 is 0.0"):
        smc.sample(Flat(), 128, kernel="hard", epsilon=0.01, path="generic", prior=Point())


# ---------------------------------------------------------------------------------- the law, generic path
def test_generic_model_kernel_samples_the_analytic_posterior():
    torch.manual_seed(SEED)
    N = 2048
    p = smc.sample(Mixture_set(0.05), N, kernel="model", path="generic", prior=std_prior())
    assert p.theta.shape == (N, 2) and p.y.shape == (N, 2) and p.distance.shape == (N,) and p.weights.shape == (N,)
    assert p.weights.dtype == torch.float64 and abs(float(p.weights.sum()) - 1.0) < 1e-12 and not torch.isnan(p.weights).any()
    assert p.epsilon == 0.05 and p.ess == pytest.approx(1.0 / float((p.weights ** 2).sum())) and p.ess > N / 4
    g = p.generations
    assert [x["kernel"] for x in g] == ["hard"] * (len(g) - 1) + ["model"] and g[-1]["epsilon"] == 0.05
    eps = [x["epsilon"] for x in g[:-1]]
    assert all(b < a for a, b in zip(eps, eps[1:])) and eps[-1] == float(np.float32(0.15))       # 3 x the Model's epsilon
    assert g[0]["n_draws"] == 2 * N and g[0]["bandwidth"] is None and all(len(x["bandwidth"]) == 2 for x in g[1:])
    assert all(x["rate"] == N / x["n_draws"] and 0 < x["ess"] <= N + 1e-6 for x in g) and g[-1]["ess"] == p.ess
    rate, m2, _ = R.analytic(0.05)
    mu, se = S.weighted_second_moment(p.theta.numpy(), p.weights.numpy())
    sims = sum(x["n_draws"] for x in g)
    print("E theta_j^2 %r, analytic %.5f, %r SE; ess %.0f of %d; %d simulations against %.0f of plain rejection"
          % (mu, m2, (mu - m2) / se, p.ess, N, sims, N / rate))
    assert (np.abs(mu - m2) <= 5.0 * se).all()
    assert sims <= 0.5 * N / rate


def test_generic_particles_stay_inside_the_support():
    """a Uniform prior whose support cuts through the posterior (the modes at -1.5 stay, those at +1.5 ... +2.5 are cut short)"""
    torch.manual_seed(SEED + 1)
    prior = distribution.Uniform(2, torch.tensor([-2.0, -2.0]), torch.tensor([2.5, 2.5]))
    p = smc.sample(R.abs_gauss_model(2, prior, epsilon=0.05, y_obs=[1.5, 1.5]), 1024, kernel="model", path="generic", prior=prior)
    assert (p.theta >= -2.0).all() and (p.theta <= 2.5).all()
    assert torch.isfinite(p.weights).all() and (p.weights > 0).all() and torch.isfinite(p.distance).all()
    assert ((p.theta > 2.2).any() or (p.theta < -1.8).any()) and p.ess > 1024 / 4          # the support's edge is populated


def test_generic_hard_kernel_agrees_with_rejection():
    torch.manual_seed(SEED + 2)
    model, e, N = Mixture_set(0.05), 0.3, 2048
    p = smc.sample(model, N, kernel="hard", epsilon=e, path="generic", prior=std_prior())
    assert p.epsilon == float(np.float32(e)) and float(p.distance.max()) <= p.epsilon and all(g["kernel"] == "hard" for g in p.generations)
    r = rejection.sample(model, 1 << 17, kernel="hard", epsilon=e, path="generic", prior=std_prior())
    mu, se = S.weighted_second_moment(p.theta.numpy(), p.weights.numpy())
    m = r.ids.numel()
    mu_r, se_r = S.weighted_second_moment(r.theta.numpy(), np.full(m, 1.0 / m))
    print("smc %r +- %r, rejection (%d draws) %r +- %r" % (mu, se, m, mu_r, se_r))
    assert m > 1000 and (np.abs(mu - mu_r) <= 5.0 * np.sqrt(se ** 2 + se_r ** 2)).all()
    # a ladder walks the same way
    torch.manual_seed(SEED + 3)
    q = smc.sample(model, 512, kernel="hard", epsilons=[1.0, 0.6, e], path="generic", prior=std_prior())
    assert [g["epsilon"] for g in q.generations[1:]] == [float(np.float32(v)) for v in (1.0, 0.6, e)] and q.epsilon == float(np.float32(e))


@pytest.mark.parametrize("bandwidth", ["scott", "beaumont", 0.3, torch.tensor([0.2, 0.4])])
def test_generic_bandwidths(bandwidth):
    torch.manual_seed(SEED + 4)
    p = smc.sample(Mixture_set(0.05), 256, kernel="hard", epsilon=0.8, bandwidth=bandwidth, path="generic", prior=std_prior())
    bw = p.generations[-1]["bandwidth"]
    if isinstance(bandwidth, float):
        assert bw == pytest.approx([0.3, 0.3])
    elif torch.is_tensor(bandwidth):
        assert bw == pytest.approx([0.2, 0.4])
    else:
        assert all(0.05 < v < 3.0 for v in bw)
    assert torch.isfinite(p.weights).all() and p.ess > 256 / 8 and p.theta.shape == (256, 2)


def test_rule_factors():
    from helpers import rule
    assert smc.rule_factor("beaumont", 256, 2) == pytest.approx(2 ** 0.5)          # a kernel of twice the weighted variance
    for n, d in ((256, 2), (4096, 4)):
        assert smc.rule_factor("silverman", n, d) == rule("silverman", n, d) and smc.rule_factor("scott", n, d) == rule("scott", n, d)
