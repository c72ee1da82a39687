"""Rejection ABC on the CPU: the restatement of glabc_abc_draws (tests/rejection_ref.py) -- that a draw depends on (model, seed,
id) alone, and its law against the analytic posterior of Mixture_set --, glabcmcmc_amd.rejection's generic path on CPU tensors
(the same law checks, the hard kernel against numpy.partition, ties / NaNs / the exact row count on a stub Model), every
ValueError of the module, the refusals of glabc_abc_draws as csrc/glabc_check.h answers them under g++, and initial_state.

Law checks: the draws are independent, so the accepted count is binomial and the standard error of the mean of theta_j^2 is
sqrt((E theta^4 - (E theta^2)^2) / m) with the moments from quadrature; both bounds are 5 standard errors.
"""
import os
import re

import numpy as np
import pytest
import torch

import rejection_ref as R
from glabcmcmc_amd import _capi, distribution, rejection
from glabcmcmc_amd.examples.Mixture import Mixture_set
from test_arg_checks import check_table

OK, NULL, DIM, KIND, ARG = 0, -1, -2, -3, -4
SEED = 20261019


def std_prior(d=2):
    return distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d))


# ---------------------------------------------------------------------------------- the restatement
def test_restated_draw_depends_on_seed_and_id_alone():
    model = Mixture_set(0.05).descriptor()
    th, y, dis, acc = R.restate(model, SEED, np.arange(40, 140))
    for ids in (np.arange(100, 110), np.array([139, 40, 77, 77, 41]), np.array([77])):
        t2, y2, d2, a2 = R.restate(model, SEED, ids)
        assert np.array_equal(t2.view(np.uint32), th[ids - 40].view(np.uint32))
        assert np.array_equal(y2.view(np.uint32), y[ids - 40].view(np.uint32))
        assert np.array_equal(d2.view(np.uint32), dis[ids - 40].view(np.uint32)) and np.array_equal(a2, acc[ids - 40])
    big = np.array([2 ** 32 - 1, 2 ** 32, 2 ** 40 + 3])
    tb, yb, db, _ = R.restate(model, SEED, big)
    for i, one in enumerate(big):                                      # ids past 2^32 use the counter's high word
        t1, y1, d1, _ = R.restate(model, SEED, np.array([one]))
        assert np.array_equal(t1[0], tb[i]) and np.array_equal(y1[0], yb[i]) and d1[0] == db[i]
    assert not np.array_equal(tb[0], tb[1]) and not np.array_equal(R.restate(model, SEED + 1, big)[0], tb)
    # theta and the noise are independent streams: y - |theta| is not theta's own normal
    assert not np.allclose(y - np.abs(th), th * np.sqrt(0.05))


def test_restatement_samples_the_analytic_posterior():
    model = Mixture_set(0.05).descriptor()
    n = 1 << 20
    th, _, dis, acc = R.restate(model, SEED, np.arange(n))
    assert not np.isnan(dis).any()
    R.law_check(th[acc == 1], n, 0.05)


# ---------------------------------------------------------------------------------- the generic path on CPU tensors
def test_generic_model_kernel_samples_the_analytic_posterior():
    torch.manual_seed(7)
    n = 1 << 20
    r = rejection.sample(Mixture_set(0.05), n, kernel="model", path="generic", prior=std_prior())
    assert r.n_draws == n and r.epsilon == 0.05 and r.theta.shape == (r.ids.numel(), 2) and r.y.shape == r.theta.shape
    assert (r.ids[1:] > r.ids[:-1]).all() and r.ids.dtype == torch.int64
    R.law_check(r.theta.numpy(), n, 0.05)
    # at another epsilon the rate follows
    r2 = rejection.sample(Mixture_set(0.05), 1 << 18, kernel="model", epsilon=0.2, path="generic", prior=std_prior())
    R.law_check(r2.theta.numpy(), 1 << 18, 0.2)


class Recording(Mixture_set):
    """Mixture_set that remembers every distance it was asked for, in order"""

    def __init__(self, epsilon):
        super().__init__(epsilon)
        self.seen = []

    def discrepancy(self, y):
        d = super().discrepancy(y)
        self.seen.append(d.numpy().copy())
        return d


@pytest.mark.parametrize("how", [dict(epsilon=0.3), dict(n_accept=1), dict(n_accept=257), dict(n_accept=10000), dict(quantile=0.0),
                                 dict(quantile=0.013), dict(quantile=0.5), dict(quantile=1.0)])
def test_generic_hard_kernel_against_numpy_partition(how, monkeypatch):
    monkeypatch.setattr(rejection, "GENERIC_CHUNK", 1536)              # seven chunks: the running best is trimmed on the way
    torch.manual_seed(11)
    n = 10000
    model = Recording(0.05)
    r = rejection.sample(model, n, kernel="hard", path="generic", prior=std_prior(), **how)
    dis = np.concatenate(model.seen)
    assert dis.size == n
    if "epsilon" in how:
        want_eps = np.float32(0.3)
    else:
        rank = how["n_accept"] - 1 if "n_accept" in how else int(np.floor(how["quantile"] * (n - 1)))
        want_eps = np.partition(dis, rank)[rank]
    eps, ids = R.hard_select(dis, **how)
    assert eps == want_eps and np.float32(r.epsilon) == want_eps and isinstance(r.epsilon, float)
    assert np.array_equal(r.ids.numpy(), ids) and np.array_equal(r.distance.numpy(), dis[ids])
    assert r.distance.numpy().max() == want_eps or "epsilon" in how
    if "n_accept" in how:
        assert r.ids.numel() == how["n_accept"]
    assert np.array_equal(model.discrepancy(r.y).numpy(), dis[ids])      # the rows belong to their distances
    assert rejection.calibrate_epsilon(Recording(0.05), 100, 0.5, path="generic", prior=std_prior()) > 0.0


def test_calibrate_epsilon_is_samples_epsilon():
    torch.manual_seed(3)
    a = rejection.calibrate_epsilon(Mixture_set(0.05), 5000, 0.01, path="generic", prior=std_prior())
    torch.manual_seed(3)
    b = rejection.sample(Mixture_set(0.05), 5000, kernel="hard", quantile=0.01, path="generic", prior=std_prior())
    assert isinstance(a, float) and a == b.epsilon and b.ids.numel() == 50


# a stub Model: theta is the draw's position, the distance a pattern of repeated values and NaNs
PATTERN = np.array([0.5, 0.25, np.nan, 0.25, 1.0, 0.25, np.nan, 0.5, 0.125, 0.25], np.float32)


class Counter:
    def __init__(self):
        self.next = 0

    def forward(self, n):
        t = torch.arange(self.next, self.next + n, dtype=torch.float32).view(n, 1)
        self.next += n
        return t, torch.zeros(n)


class Stub:
    epsilon, theta_dim, y_dim = 0.3, 1, 1

    def generate_samples(self, theta, num_samples=1):
        return theta.clone()

    def discrepancy(self, y):
        return torch.from_numpy(PATTERN[y.view(-1).long().numpy() % PATTERN.size])

    def calculate_log_kernel_dis(self, dis, epsilon=None):
        return -0.5 * (dis / (self.epsilon if epsilon is None else epsilon)) ** 2


@pytest.mark.parametrize("chunk", [7, 1 << 20])
def test_ties_nans_and_the_exact_row_count(chunk, monkeypatch):
    monkeypatch.setattr(rejection, "GENERIC_CHUNK", chunk)
    n = 50
    dis = PATTERN[np.arange(n) % PATTERN.size]
    n_valid = int((~np.isnan(dis)).sum())                                # 40: 5 x 0.125, 20 x 0.25, 10 x 0.5, 5 x 1.0
    for k in (1, 5, 6, 7, 24, 25, 26, 35, 36, n_valid):
        r = rejection.sample(Stub(), n, kernel="hard", n_accept=k, path="generic", prior=Counter())
        eps, ids = R.hard_select(dis, n_accept=k)
        assert r.ids.numel() == k and np.array_equal(r.ids.numpy(), ids) and np.float32(r.epsilon) == eps
        assert np.array_equal(r.theta.view(-1).numpy(), ids.astype(np.float32)) and not np.isnan(r.distance.numpy()).any()
        ties = r.ids.numpy()[r.distance.numpy() == eps]
        assert np.array_equal(ties, np.nonzero(dis == eps)[0][:ties.size])          # the ties are the first by id
    for q in (0.0, 0.1, 0.5, 0.8):
        r = rejection.sample(Stub(), n, kernel="hard", quantile=q, path="generic", prior=Counter())
        eps, ids = R.hard_select(dis, quantile=q)
        assert np.array_equal(r.ids.numpy(), ids) and np.float32(r.epsilon) == eps          # every tie returns
    r = rejection.sample(Stub(), n, kernel="hard", epsilon=0.25, path="generic", prior=Counter())
    assert np.array_equal(r.ids.numpy(), np.nonzero(dis <= 0.25)[0])
    r = rejection.sample(Stub(), n, kernel="hard", epsilon=0.0, path="generic", prior=Counter())
    assert r.ids.numel() == 0 and r.theta.shape == (0, 1)
    for bad in (dict(n_accept=n_valid + 1), dict(n_accept=n), dict(quantile=1.0), dict(quantile=0.82)):
        with pytest.raises(ValueError, match="NaN"):                      # the wanted rank falls on a NaN
            rejection.sample(Stub(), n, kernel="hard", path="generic", prior=Counter(), **bad)
    with pytest.raises(ValueError, match="NaN"):
        rejection.calibrate_epsilon(Stub(), n, 1.0, path="generic", prior=Counter())
    # the Model's kernel never keeps a NaN either
    torch.manual_seed(0)
    r = rejection.sample(Stub(), 5000, kernel="model", path="generic", prior=Counter())
    assert 0 < r.ids.numel() < 5000 and not np.isnan(r.distance.numpy()).any()


# ---------------------------------------------------------------------------------- arguments
def test_value_errors():
    m, p = Mixture_set(0.05), std_prior()
    gen = dict(path="generic", prior=p)
    S = rejection.sample
    bad_calls = [
        lambda: S(m, 0, **gen), lambda: S(m, -3, **gen), lambda: S(m, 2.5, **gen), lambda: S(m, True, **gen),
        lambda: S(m, 100, kernel="soft", **gen), lambda: S(m, 100, path="quick", prior=p),
        lambda: S(m, 100, kernel="model", n_accept=5, **gen), lambda: S(m, 100, kernel="model", quantile=0.5, **gen),
        lambda: S(m, 100, kernel="model", epsilon=0.0, **gen), lambda: S(m, 100, kernel="model", epsilon=-1.0, **gen),
        lambda: S(m, 100, kernel="model", epsilon=float("nan"), **gen), lambda: S(m, 100, kernel="model", epsilon="wide", **gen),
        lambda: S(m, 100, kernel="hard", **gen), lambda: S(m, 100, kernel="hard", epsilon=0.1, n_accept=5, **gen),
        lambda: S(m, 100, kernel="hard", n_accept=5, quantile=0.1, **gen), lambda: S(m, 100, kernel="hard", epsilon=0.1, quantile=0.1, **gen),
        lambda: S(m, 100, kernel="hard", n_accept=0, **gen), lambda: S(m, 100, kernel="hard", n_accept=101, **gen),
        lambda: S(m, 100, kernel="hard", n_accept=2.0, **gen), lambda: S(m, 100, kernel="hard", quantile=-0.1, **gen),
        lambda: S(m, 100, kernel="hard", quantile=1.5, **gen), lambda: S(m, 100, kernel="hard", quantile=float("nan"), **gen),
        lambda: S(m, 100, kernel="hard", quantile="half", **gen), lambda: S(m, 100, kernel="hard", epsilon=-0.1, **gen),
        lambda: S(m, 100, kernel="hard", epsilon=float("inf"), **gen),
        lambda: S(m, 100, path="generic"), lambda: S(m, 100, path="generic", prior=object()),
        lambda: S(Stub(), 100, path="fused"), lambda: S(Stub(), 100, path="auto"),          # auto falls to generic, which needs prior=
        lambda: rejection.calibrate_epsilon(m, 100, None, **gen), lambda: rejection.calibrate_epsilon(m, 100, 2.0, **gen),
        lambda: rejection.calibrate_epsilon(m, 0, 0.5, **gen), lambda: rejection.calibrate_epsilon(m, 100, 0.5, n_accept=3, **gen),
        lambda: rejection.initial_state(m, 0, **gen), lambda: rejection.initial_state(m, 2.0, **gen),
        lambda: rejection.initial_state(m, 10, n_draws=5, **gen), lambda: rejection.initial_state(m, 10, n_draws=0, **gen),
        lambda: rejection.initial_state(m, 10, kernel="soft", **gen),
        lambda: rejection.draws(m, -1, seed=1), lambda: rejection.draws(m, 1.5, seed=1), lambda: rejection.draws(m, 4, seed=None),
        lambda: rejection.draws(m, 4, seed=1.0), lambda: rejection.draws(m, 4, seed=1, row0=-1),
        lambda: rejection.draws(m, 4, seed=1, want=()), lambda: rejection.draws(m, 4, seed=1, want=("theta", "weights")),
        lambda: rejection.draws(m, 4, seed=1, epsilon=0.0),
        lambda: rejection.draws(m, 4, seed=1, row0=2, ids=[1, 2, 3, 4]), lambda: rejection.draws(m, 4, seed=1, ids=[1, 2, 3]),
        lambda: rejection.draws(m, 4, seed=1, ids=[1.0, 2.0, 3.0, 4.0]), lambda: rejection.draws(m, 4, seed=1, ids=[[1, 2], [3, 4]]),
        lambda: rejection.draws(m, 4, seed=1, ids=[1, -2, 3, 4]),
        lambda: rejection.draws(Stub(), 4, seed=1),
        lambda: rejection.draws(Mixture_set(0.05, prior=distribution.Gamma(torch.tensor([2.0, 2.0]), torch.tensor([1.0, 1.0]))), 4, seed=1),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d raised nothing" % i)
    with pytest.raises(ValueError, match="101"):                          # the offending value is named
        S(m, 100, kernel="hard", n_accept=101, **gen)
    with pytest.raises(ValueError, match="soft"):
        S(m, 100, kernel="soft", **gen)


def test_which_models_take_the_fused_path():
    from glabcmcmc_amd.examples.GK import GK_set
    assert isinstance(rejection.accepted(Mixture_set(0.05)), _capi.Model) and rejection.accepted(GK_set(0.5)) is not None
    assert rejection.accepted(Mixture_set(0.05), 0.2).kern_scale == pytest.approx(0.2)
    gamma = distribution.Gamma(torch.tensor([2.0, 2.0]), torch.tensor([1.0, 1.0]))
    assert rejection.accepted(Mixture_set(0.05, prior=gamma)) is None and rejection.accepted(Stub()) is None
    uniform = distribution.Uniform(2, torch.tensor([-3.0, -3.0]), torch.tensor([3.0, 3.0]))
    assert rejection.accepted(Mixture_set(0.05, prior=uniform)) is not None
    if not torch.cuda.is_available():                                      # the fused path never computes on the host
        for call in (lambda: rejection.sample(Mixture_set(0.05), 100), lambda: rejection.draws(Mixture_set(0.05), 4, seed=1),
                     lambda: rejection.initial_state(Mixture_set(0.05), 4), lambda: rejection.calibrate_epsilon(Mixture_set(0.05), 100, 0.1)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()


def test_entry_point_is_bound_and_exported():
    import glabcmcmc_amd
    assert "glabc_abc_draws" in _capi.ENTRY_POINTS and _capi.VERSION == 301 and _capi.STREAM_LAYOUT == 2
    assert glabcmcmc_amd.rejection is rejection and "rejection" in glabcmcmc_amd.__all__
    assert (_capi.ABC_NOISE_KEY, _capi.ABC_ACCEPT_KEY) == (R.NOISE_KEY, R.ACCEPT_KEY)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glabc.h")).read()
    assert "#define GLABC_ABC_NOISE_KEY  0x%Xull" % R.NOISE_KEY in header and "#define GLABC_ABC_ACCEPT_KEY 0x%Xull" % R.ACCEPT_KEY in header
    assert _capi.lib().glabc_abc_draws(None, 0, 0, None, 0, 0, None, None, None, None, None) == NULL          # resolves, and refuses


# ---------------------------------------------------------------------------------- the refusals (csrc/glabc_check.h)
def test_check_abc_draws(tmp_path_factory):
    prelude = "static const int64_t IDS[4] = {3, 1, 3, 1ll << 40}; static uint8_t ACC[4]; "
    call = "check_abc_draws(%s, %s, %s, %s, %s, %s, %s, %s, %s)"
    base = dict(m="&b.m", row0="0", ids="nullptr", n="65", stride="65", th="b.f", y="b.f", d="b.f", a="ACC")

    def row(want, spoil="", **kw):
        a = dict(base, **kw)
        return (prelude + spoil, call % (a["m"], a["row0"], a["ids"], a["n"], a["stride"], a["th"], a["y"], a["d"], a["a"]), want)
    none = dict(th="nullptr", y="nullptr", d="nullptr", a="nullptr")
    gauss_prior = "b.m.prior = dist3(GLABC_DIST_DIAG_GAUSS); "
    check_table(tmp_path_factory, "abc_draws", [
        row(OK), row(OK, gauss_prior), row(OK, "make_gk(b); "), row(OK, n="0", stride="0"), row(OK, stride="70"), row(OK, row0="1ll << 40"),
        row(OK, ids="IDS", n="4", stride="4"), row(OK, **dict(none, d="b.f")), row(OK, **dict(none, a="ACC")), row(OK, **dict(none, th="b.f")),
        row(OK, **dict(none, y="b.f")),
        row(OK, "b.m.theta_dim = b.m.y_dim = b.m.prior.dim = 8; "), row(OK, "b.m.theta_dim = b.m.y_dim = b.m.prior.dim = 1; "),
        row(OK, "b.m.prior.p2[0] = NaN; b.m.kern_scale = 0.0f; "),          # the parameters' values are not examined
        row(NULL, m="nullptr"), row(NULL, **none), row(NULL, "b.m.theta_dim = 9; ", **none), row(NULL, m="nullptr", n="-1"),
        row(DIM, "b.m.theta_dim = 0; "), row(DIM, "b.m.theta_dim = b.m.y_dim = 9; "), row(DIM, "b.m.y_dim = 4; "), row(DIM, "b.m.y_dim = 0; "),
        row(DIM, "make_gk(b); b.m.y_dim = 7; "), row(DIM, "make_gk(b); b.m.theta_dim = 3; "),
        row(DIM, "b.m.theta_dim = 9; b.m.sim_kind = GLABC_SIM_USER; "), row(DIM, "b.m.y_dim = 4; b.m.prior.kind = GLABC_DIST_GAMMA; ", n="-1"),
        row(KIND, "b.m.sim_kind = GLABC_SIM_USER; "), row(KIND, "b.m.sim_kind = 7; "), row(KIND, "b.m.prior = dist3(GLABC_DIST_GAMMA); "),
        row(KIND, "b.m.prior.kind = 5; "), row(KIND, "b.m.prior.dim = 2; "), row(KIND, "b.m.prior.dim = 4; "),
        row(KIND, "make_gk(b); b.m.prior.dim = 8; "), row(KIND, "b.m.sim_kind = GLABC_SIM_USER; ", n="-1"), row(KIND, "b.m.prior.dim = 2; ", row0="-1"),
        row(ARG, n="-1"), row(ARG, stride="64"), row(ARG, row0="-1"), row(ARG, ids="IDS", row0="1", n="4", stride="4"),
        row(ARG, n="-1", stride="-1"),
    ])


def test_resource_report_shows_no_private_segment():
    """profiles/rejection_kernel_resources.txt: nine instantiations of abc_draws_kernel, none with a private segment or a spill"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "profiles", "rejection_kernel_resources.txt")).read()
    kernels = re.split(r"^Function Name: ", text, flags=re.M)[1:]
    assert len(kernels) == 9 and all("abc_draws_kernel" in k for k in kernels)
    shapes = sorted(tuple(int(x) for x in re.search(r"abc_draws_kernelILi(\d)ELi(\d)E", k).groups()) for k in kernels)
    assert shapes == sorted([(d, d) for d in range(1, 9)] + [(4, 8)])
    for k in kernels:
        field = lambda name: int(re.search(r"%s: (\d+)" % re.escape(name), k).group(1))          # noqa: E731
        assert field("ScratchSize [bytes/lane]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0
        assert field("Occupancy [waves/SIMD]") >= 8


# ---------------------------------------------------------------------------------- initial_state
@pytest.mark.parametrize("kernel", ["hard", "model"])
def test_initial_state_shapes_and_dtypes(kernel):
    torch.manual_seed(5)
    kw = dict(n_draws=1 << 17, epsilon=0.3) if kernel == "model" else {}
    th, y = rejection.initial_state(Mixture_set(0.05), 16, kernel=kernel, path="generic", prior=std_prior(), **kw)
    assert th.shape == (16, 2) and y.shape == (16, 2) and th.dtype == y.dtype == torch.float32
    assert th.device.type == "cpu" and y.device.type == "cpu" and th.is_contiguous() and y.is_contiguous()
    assert torch.isfinite(th).all() and torch.isfinite(y).all()
    if kernel == "hard":                                                  # the 16 nearest of 64 * 16 draws
        assert float(Mixture_set(0.05).discrepancy(y).max()) < 0.6
    else:
        with pytest.raises(RuntimeError, match="only 0 of 64"):           # names the count
            rejection.initial_state(Mixture_set(1e-6), 16, kernel="model", n_draws=64, path="generic", prior=std_prior())
