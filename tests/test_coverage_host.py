"""Coverage checks on the CPU: the restatement of glabc_coverage_counts (tests/coverage_ref.py) against a plain NumPy loop, the
formulas of glabcmcmc_amd.coverage.Coverage against exact fractions, combine over shards, the bisection of ``quantile=`` against
numpy.sort, the generic path on CPU tensors against the restatement fed the same distance, every ValueError of the module, the
refusals of glabc_coverage_counts as csrc/glabc_check.h answers them under g++, the binding and the resource report.

Bounds.  The hard kernel's sums are integers and every comparison below is equality.  Under the Model's kernel the restated
multiplicity is held to rint(65536 exp(-(d / w)^2 / 2)) in float64: the float32 chain (a division, a square, a halving, glabc_expf)
is off by a few units of 2^-24 relative to p <= 1, which is 2^-8 units of m at most, so |m - 65536 p| <= 1/2 + 2^-6.  The generic
path takes torch.exp where the kernel takes glabc_expf; the two may differ in the last bit, so a pair's m may differ by one unit
where 65536 p lies within 2^-6 of a half-integer, and nowhere else.
"""
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import coverage_ref as CR
import rejection_ref as R
from glabcmcmc_amd import _capi, coverage, distribution, rejection
from glabcmcmc_amd.examples.Mixture import Mixture_set
from test_arg_checks import check_table

OK, NULL, DIM, KIND, ARG = 0, -1, -2, -3, -4
SEED = 20261021
N, NT = 700, 24


def fixture(n=N, nt=NT, row0=0):
    """table draws row0 .. of Mixture_set, and nt test pairs from the stream coverage.check would take them from"""
    model = Mixture_set(0.05).descriptor()
    theta, y = CR.table(model, SEED, row0, n)
    ts, ys = CR.table(model, SEED ^ coverage.COVERAGE_TEST_KEY, 0, nt)
    return model, theta, y, ts, ys


def plain_distance(y, y_star):
    d0, d1 = y[:, 0] - y_star[0], y[:, 1] - y_star[1]
    return np.sqrt(d0 * d0 + d1 * d1)                                  # float32 throughout


# ---------------------------------------------------------------------------------- the restatement
def test_restatement_against_a_plain_numpy_loop():
    model, theta, y, ts, ys = fixture()
    widths = np.array([0.3, 0.05, 1.0, np.inf, 0.0, 0.7] * 4, np.float32)
    mass, mass2, below = CR.restate(model, SEED, 0, N, ts, ys, widths, "hard")
    for r in range(NT):
        d = plain_distance(y, ys[r])
        keep = d <= widths[r]
        assert mass[r] == int(keep.sum()) == mass2[r]
        assert [below[r, j] for j in range(2)] == [int((keep & (theta[:, j] < ts[r, j])).sum()) for j in range(2)]
    assert mass[3] == N and mass[4] == 0 and 0 < mass[0] < N           # +inf keeps the table, 0 keeps nothing here
    # the Model's kernel: the quantised weight against float64
    widths = np.array([0.3, 0.05, 1.0, np.inf] * 6, np.float32)
    mass, mass2, below = CR.restate(model, SEED, 0, N, ts, ys, widths, "model")
    for r in range(NT):
        d = plain_distance(y, ys[r]).astype(np.float64)
        exact = 65536.0 * np.exp(-0.5 * (d / np.float64(widths[r])) ** 2)
        m = CR.multiplicity(plain_distance(y, ys[r]), widths[r], "model")
        assert np.abs(m - exact).max() <= 0.5 + 2.0 ** -6 and m.max() <= 65536 and m.min() >= 0
        assert mass[r] == int(m.sum()) and mass2[r] == sum(int(v) ** 2 for v in m)
        assert below[r, 1] == int(m[theta[:, 1] < ts[r, 1]].sum())
    assert mass[3] == 65536 * N and mass2[3] == 65536 ** 2 * N          # an infinite width weighs every pair fully
    # NaNs: a NaN width, a NaN distance and a NaN theta* count nothing
    assert CR.multiplicity(np.array([0.1, np.nan], np.float32), np.nan, "hard").tolist() == [0, 0]
    assert CR.multiplicity(np.array([0.1, np.nan, np.inf], np.float32), 0.5, "model").tolist()[1:] == [0, 0]
    assert CR.multiplicity(np.array([0.0, np.inf], np.float32), np.inf, "model").tolist() == [65536, 0]          # inf / inf is a NaN
    assert CR.multiplicity(np.array([0.0, 0.1], np.float32), 0.0, "model").tolist() == [0, 0]                  # 0 / 0 too
    ts2 = ts.copy()
    ts2[0, 0] = np.nan
    _, _, b = CR.counts(theta, y, ts2, ys, np.full(NT, np.inf, np.float32), "hard", plain_distance)
    assert b[0, 0] == 0 and b[0, 1] > 0


def test_a_tie_in_theta_is_not_below():
    model, theta, y, _, _ = fixture(n=50)
    mass, _, below = CR.counts(theta, y, theta[7:8].copy(), y[7:8].copy(), np.array([np.inf], np.float32), "hard", plain_distance)
    assert mass[0] == 50 and [below[0, j] for j in range(2)] == [int((theta[:, j] < theta[7, j]).sum()) for j in range(2)]
    assert CR.counts(theta, y, theta[7:8].copy(), y[7:8].copy(), np.array([0.0], np.float32), "hard", plain_distance)[0][0] == 1


# ---------------------------------------------------------------------------------- Coverage: the formulas
MASS = [0, 1, 10, 10, 10, 19, 3, 0, 65536 * 4]
BELOW = [[0, 0], [0, 1], [0, 10], [5, 9], [1, 3], [0, 19], [1, 2], [0, 0], [65536 * 2, 65536 * 4]]


def made(kernel="hard", mass=MASS, below=BELOW):
    m = torch.tensor(mass, dtype=torch.int64)
    return coverage.Coverage(m, m.clone() * (1 if kernel == "hard" else 40000), torch.tensor(below, dtype=torch.int64),
                             torch.full((len(mass),), 0.3), 1000, kernel)


@pytest.mark.parametrize("kernel", ["hard", "model"])
def test_coverage_formulas_against_exact_fractions(kernel):
    c = made(kernel)
    unit = Fraction(1 if kernel == "hard" else 65536)
    assert c.unit == unit and c.n_empty == 2 and c.empty.tolist() == [m == 0 for m in MASS] and c.n_draws == 1000
    pit = c.pit
    live = [r for r, m in enumerate(MASS) if m]
    for r, m in enumerate(MASS):
        for j in range(2):
            if m == 0:
                assert torch.isnan(pit[r, j])
            else:
                assert float(pit[r, j]) == float((BELOW[r][j] + unit / 2) / (m + unit))
    ess = c.ess
    assert torch.isnan(ess[0]) and torch.isnan(ess[7])
    for r in live:
        assert float(ess[r]) == pytest.approx(float(Fraction(MASS[r]) ** 2 / (MASS[r] * (1 if kernel == "hard" else 40000))), rel=1e-15)
    for bins in (1, 2, 10, 7):
        want = np.zeros((2, bins), np.int64)
        for r in live:
            for j in range(2):
                want[j, int((BELOW[r][j] + unit / 2) / (MASS[r] + unit) * bins)] += 1
        h = c.rank_histogram(bins)
        assert h.dtype == torch.int64 and np.array_equal(h.numpy(), want) and int(h.sum()) == 2 * len(live)
        e = Fraction(2 * len(live), bins)
        chi = c.chi2(bins)
        assert chi.dof == bins - 1 and chi.value == pytest.approx(float(sum((Fraction(int(v)) - e) ** 2 / e for v in want.sum(axis=0))), abs=1e-12)
        assert chi.per_coordinate.shape == (2,)
    levels = (0.5, 0.9, 0.95, 1.0)
    got = c.coverage(levels)
    assert got.levels == levels and got.n_tests == len(live)
    for i, level in enumerate(levels):
        f = Fraction(level).limit_denominator(10 ** 6)
        inside = [[abs((BELOW[r][j] + unit / 2) / (MASS[r] + unit) - Fraction(1, 2)) <= f / 2 for j in range(2)] for r in live]
        per = [sum(row[j] for row in inside) / len(live) for j in range(2)]
        assert got.per_coordinate[i].tolist() == per and float(got.pooled[i]) == pytest.approx(sum(per) / 2)
    assert got.per_coordinate[3].tolist() == [1.0, 1.0]                 # the whole interval holds every rank


def test_coverage_boundaries_are_decided_exactly():
    # hard, mass 9: pit = (below + 1/2) / 10, so |pit - 1/2| = level / 2 exactly at below = 0 and 9 for level 0.9, and at 2 and 7 for
    # level 0.5 -- ties that float64 arithmetic on 0.9 / 2 and 0.05 cannot be trusted with; all are inside
    c = made(mass=[9] * 10, below=[[b, 9 - b] for b in range(10)])
    got = c.coverage((0.5, 0.9, 0.8))
    assert got.per_coordinate[1].tolist() == [1.0, 1.0]
    assert got.per_coordinate[0].tolist() == [0.6, 0.6]                 # below 2 .. 7
    assert got.per_coordinate[2].tolist() == [0.8, 0.8]                 # |2 b - 9| <= 8: below 1 .. 8 (0.5 and 8.5 are outside)
    # one unit outside the boundary: mass 19, level 0.9 keeps |2 b - 19| <= 18, so below = 0 (pit 1/40) is out
    got = made(mass=[19, 19, 19], below=[[0, 1], [19, 18], [1, 9]]).coverage(0.9)
    assert got.per_coordinate[0].tolist() == [pytest.approx(1 / 3), 1.0]
    # sums past 2^53 stay exact: Python integers take over.  2^61 = 20 k + 12, so with below = k the test 10 |2 below - mass| <=
    # 9 (mass + 1) reads 9 mass + 12 <= 9 mass + 9, outside by 3 in 2 * 10^19, and with below = k + 1 it reads 9 mass - 8, inside
    big = 1 << 61
    c = made(mass=[big, big], below=[[big // 20, big // 20 + 1], [0, big]])
    assert c.coverage(0.9).per_coordinate[0].tolist() == [0.0, 0.5]
    assert c.rank_histogram(10).tolist() == [[2] + [0] * 9, [1] + [0] * 8 + [1]]
    with pytest.raises(ValueError):
        c.coverage(0.0)
    with pytest.raises(ValueError):
        c.coverage((0.5, 1.5))
    with pytest.raises(ValueError):
        c.rank_histogram(0)
    empty = made(mass=[0, 0], below=[[0, 0], [0, 0]])
    assert empty.n_empty == 2 and empty.coverage(0.9).n_tests == 0 and np.isnan(empty.chi2().value) and int(empty.rank_histogram().sum()) == 0


# ---------------------------------------------------------------------------------- the generic path on CPU tensors
def restated_table(model):
    def table(row0, n):
        theta, y = CR.table(model, SEED, row0, n)
        return torch.from_numpy(theta), torch.from_numpy(y)
    return table


def torch_distance(y, y_star):
    return coverage.euclidean(torch.from_numpy(np.ascontiguousarray(y)), torch.from_numpy(np.ascontiguousarray(y_star))).numpy()


def generic(model, ts, ys, n=N, **kw):
    return coverage.check(Mixture_set(0.05), ts.shape[0], n, tests=(torch.from_numpy(ts), torch.from_numpy(ys)), seed=SEED,
                          table=restated_table(model), **kw)


def test_generic_path_equals_the_restatement_fed_the_same_distance(monkeypatch):
    monkeypatch.setattr(rejection, "GENERIC_CHUNK", 256)                # three chunks
    model, theta, y, ts, ys = fixture()
    widths = np.array([0.3, 0.05, 1.0, np.inf, 0.0, 0.7] * 4, np.float32)
    c = generic(model, ts, ys, kernel="hard", epsilon=torch.from_numpy(widths))
    mass, mass2, below = CR.counts(theta, y, ts, ys, widths, "hard", torch_distance)
    assert c.mass.tolist() == list(mass) and c.mass2.tolist() == list(mass2) and c.below.tolist() == below.tolist()
    assert c.kernel == "hard" and c.unit == 1 and c.n_draws == N and np.array_equal(c.widths.numpy(), widths)
    assert c.mass.dtype == c.below.dtype == torch.int64 and not c.mass.is_cuda
    assert torch.equal(c.ess[~c.empty], c.mass[~c.empty].double())       # Kish under the hard kernel: the kept count
    # one width for all tests, and the default: the Model's epsilon
    c1 = generic(model, ts, ys, kernel="hard", epsilon=0.3)
    assert c1.mass.tolist() == list(CR.counts(theta, y, ts, ys, np.full(NT, 0.3, np.float32), "hard", torch_distance)[0])
    assert generic(model, ts, ys, kernel="hard").widths.tolist() == [np.float32(0.05)] * NT
    # a user's distance
    c2 = generic(model, ts, ys, kernel="hard", epsilon=0.4, distance=lambda yy, s: (yy - s).abs().max(dim=1).values)
    cheb = lambda yy, s: np.abs(yy - s).max(axis=1)                      # noqa: E731
    assert c2.mass.tolist() == list(CR.counts(theta, y, ts, ys, np.full(NT, 0.4, np.float32), "hard", cheb)[0])
    # the Model's kernel: the rule pair by pair (module docstring), and the sums of the path's own multiplicities
    w = np.float32(0.3)
    c3 = generic(model, ts, ys, kernel="model", epsilon=float(w))
    for r in range(NT):
        d = torch_distance(y, ys[r])
        m_ref = CR.multiplicity(d, w, "model")
        m_gen = coverage.multiplicity(torch.from_numpy(d), w, "model").numpy()
        frac = 65536.0 * np.exp(-0.5 * (d.astype(np.float64) / np.float64(w)) ** 2) % 1.0
        assert np.abs(m_gen - m_ref).max() <= 1 and np.array_equal(m_gen[np.abs(frac - 0.5) > 2.0 ** -6], m_ref[np.abs(frac - 0.5) > 2.0 ** -6])
        assert int(c3.mass[r]) == int(m_gen.sum()) and int(c3.mass2[r]) == int((m_gen * m_gen).sum())
        assert int(c3.below[r, 0]) == int(m_gen[theta[:, 0] < ts[r, 0]].sum())
    assert (c3.ess[~c3.empty] <= N).all() and c3.unit == 65536


def test_combine_over_draw_shards_and_test_slices_equals_one_shot():
    model, theta, y, ts, ys = fixture()
    widths = torch.tensor([0.3, 0.05, 1.0, 0.7] * 6)
    tt, yy = torch.from_numpy(ts), torch.from_numpy(ys)
    one = generic(model, ts, ys, kernel="hard", epsilon=widths)
    kw = dict(kernel="hard", seed=SEED, table=restated_table(model))
    parts = []
    for t0, t1 in ((0, 10), (10, NT)):                                   # two slices of tests x three shards of draws
        for r0, n in ((0, 300), (300, 1), (301, N - 301)):
            parts.append(coverage.terms(Mixture_set(0.05), t1 - t0, n, tests=(tt[t0:t1], yy[t0:t1]), epsilon=widths[t0:t1], row0=r0, test0=t0, **kw))
    got = coverage.combine(parts[::-1])                                  # in any order
    assert torch.equal(got.mass, one.mass) and torch.equal(got.mass2, one.mass2) and torch.equal(got.below, one.below)
    assert torch.equal(got.widths, one.widths) and got.n_draws == N and got.kernel == "hard"
    assert parts[1].n_draws == 1 and parts[1].row0 == 300 and parts[4].test0 == 10
    with pytest.raises(ValueError):                                      # a slice that met fewer draws
        coverage.combine(parts[:4])
    with pytest.raises(ValueError):
        coverage.combine([])
    with pytest.raises(ValueError):                                      # other widths for the same tests
        coverage.combine([parts[0], parts[1]._replace(widths=parts[1].widths + 1)])
    with pytest.raises(ValueError):
        coverage.combine([parts[0], parts[1]._replace(kernel="model")])


# ---------------------------------------------------------------------------------- the bisection of quantile=
def test_bisection_equals_numpy_sort():
    nan = np.nan
    rows = np.array([
        [0.5, 0.25, 0.25, 1.0, 0.25, 0.125, 3.0, 0.5],                   # ties at the rank
        [0.0, 0.0, 0.0, 2.0, 1.0, 0.0, 5.0, 4.0],                        # a tolerance of exactly 0
        [nan, 0.75, nan, 0.5, np.inf, 1e-45, 3e38, 0.5],                 # NaNs sort last; a subnormal, a huge value, +inf
        [7.0] * 8,
    ], np.float32)
    count = lambda w: torch.from_numpy((rows <= w.numpy()[:, None]).sum(axis=1))          # noqa: E731
    for rank in range(8):
        want = np.array([CR.sort_rank(row, rank) for row in rows])
        if np.isnan(want).any():
            with pytest.raises(ValueError, match="NaN"):
                coverage.bisect_widths(count, 4, rank)
            continue
        got = coverage.bisect_widths(count, 4, rank)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32)), rank
    calls = []
    coverage.bisect_widths(lambda w: calls.append(1) or count(w), 4, 2)
    assert len(calls) == 31
    # driven by the restatement: every test's own rank among its restated distances, and the sums at those tolerances
    model, theta, y, ts, ys = fixture()
    dist = CR.oracle_distance(model)
    dis = np.stack([dist(y, ys[r]) for r in range(NT)])
    for q in (0.0, 0.01, 0.37, 1.0):
        rank = int(np.floor(q * (N - 1)))
        got = coverage.bisect_widths(lambda w: torch.from_numpy((dis <= w.numpy()[:, None]).sum(axis=1)), NT, rank)
        want = np.array([CR.sort_rank(row, rank) for row in dis])
        assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    # the public route on the generic path: quantile -> widths -> sums
    c = generic(model, ts, ys, kernel="hard", quantile=0.01)
    want = np.array([CR.sort_rank(torch_distance(y, ys[r]), 6) for r in range(NT)])           # floor(0.01 * 699) = 6
    assert np.array_equal(c.widths.numpy().view(np.uint32), want.view(np.uint32)) and c.mass.tolist() == [7] * NT


# ---------------------------------------------------------------------------------- arguments
def test_value_errors():
    m = Mixture_set(0.05)
    model, theta, y, ts, ys = fixture(n=40, nt=4)
    tests = (torch.from_numpy(ts), torch.from_numpy(ys))
    gen = dict(tests=tests, table=restated_table(model), seed=SEED)
    K = coverage.check
    bad_calls = [
        lambda: K(m, 0, 40, **gen), lambda: K(m, 4, 0, **gen), lambda: K(m, 4.0, 40, **gen), lambda: K(m, True, 40, **gen),
        lambda: K(m, 4, 40, kernel="soft", **gen), lambda: K(m, 4, 40, path="quick", **gen),
        lambda: K(m, 4, 40, kernel="model", quantile=0.5, **gen), lambda: K(m, 4, 40, kernel="hard", quantile=0.5, epsilon=0.1, **gen),
        lambda: K(m, 4, 40, kernel="hard", quantile=1.5, **gen), lambda: K(m, 4, 40, kernel="hard", quantile="half", **gen),
        lambda: K(m, 4, 40, kernel="model", epsilon=0.0, **gen), lambda: K(m, 4, 40, kernel="hard", epsilon=-0.1, **gen),
        lambda: K(m, 4, 40, epsilon=float("nan"), **gen), lambda: K(m, 4, 40, epsilon="wide", **gen),
        lambda: K(m, 4, 40, epsilon=torch.ones(3), **gen), lambda: K(m, 4, 40, row0=-1, **gen),
        lambda: K(m, 4, 40, **dict(gen, seed=1.5)), lambda: K(m, 4, 40, test_seed="x", **gen),
        lambda: K(m, 4, 40, **dict(gen, tests=(tests[0], tests[1][:3]))), lambda: K(m, 4, 40, **dict(gen, tests=(tests[0][:, :1], tests[1]))),
        lambda: K(m, 4, 40, **dict(gen, tests=tests[0])), lambda: K(m, 4, 40, **dict(gen, tests=None)),          # table= needs tests=
        lambda: K(m, 4, 40, path="fused", **gen), lambda: K(m, 4, 40, **dict(gen, table=3)),
        lambda: K(m, (1 << 20) + 1, 40, **gen),
        lambda: K(Stub(), 4, 40, tests=tests, path="generic"), lambda: K(Stub(), 4, 40, tests=tests, path="fused"),
        lambda: coverage.terms(m, 4, 40, test0=-1, **gen),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d raised nothing" % i)
    with pytest.raises(ValueError, match="soft"):                          # the offending value is named
        K(m, 4, 40, kernel="soft", **gen)
    if not torch.cuda.is_available():                                      # the fused path never computes on the host
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            K(m, 4, 40, seed=SEED)


class Stub:
    """a callback Model: rejection.draws does not take it, the generic path draws it from prior= in torch"""
    epsilon, theta_dim, y_dim = 0.3, 1, 1

    def generate_samples(self, theta, num_samples=1):
        return theta.abs() + 0.1 * torch.randn_like(theta)


def test_callback_model_runs_the_generic_path():
    torch.manual_seed(3)
    prior = distribution.DiagGaussian(1, torch.zeros(1), torch.zeros(1))
    c = coverage.check(Stub(), 16, 2000, kernel="hard", epsilon=0.2, prior=prior)
    assert c.mass.shape == (16,) and c.below.shape == (16, 1) and c.n_draws == 2000 and (c.below[:, 0] <= c.mass).all()
    assert 0 < int(c.mass.sum()) < 16 * 2000 and c.widths.tolist() == [np.float32(0.2)] * 16
    c = coverage.check(Stub(), 16, 2000, prior=prior)                      # the Model's kernel at Stub.epsilon
    assert c.kernel == "model" and (c.ess[~c.empty] <= 2000).all() and (c.mass <= 65536 * 2000).all()


# ---------------------------------------------------------------------------------- the binding and the refusals
def test_entry_point_is_bound_and_exported():
    import glabcmcmc_amd
    assert "glabc_coverage_counts" in _capi.ENTRY_POINTS and len(_capi.ENTRY_POINTS["glabc_coverage_counts"][1]) == 14
    assert _capi.VERSION == 301 and _capi.STREAM_LAYOUT == 2
    assert glabcmcmc_amd.coverage is coverage and "coverage" in glabcmcmc_amd.__all__
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "glabc.h")).read()
    assert "#define GLABC_COVERAGE_TEST_KEY 0x%Xull" % coverage.COVERAGE_TEST_KEY in header
    assert coverage.COVERAGE_TEST_KEY not in (R.NOISE_KEY, R.ACCEPT_KEY, 0) and coverage.MAX_TESTS == 1 << 20
    assert "#define GLABC_MAX_COVERAGE_TESTS (1ll << 20)" in header and "#define GLABC_MAX_COVERAGE_DRAWS (1ll << 30)" in header
    lib = _capi.lib()
    assert lib.glabc_coverage_counts.argtypes == _capi.ENTRY_POINTS["glabc_coverage_counts"][1]
    assert lib.glabc_coverage_counts(None, 0, 0, 0, None, None, None, 0, 0, 0, None, None, None, None) == NULL          # resolves, and refuses


def test_check_coverage_counts(tmp_path_factory):
    prelude = "static unsigned long long M[4]; "
    call = "check_coverage_counts(%s, %s, %s, %s, %s, %s, %s, %s, %s, %s)"
    base = dict(m="&b.m", row0="0", n="65", ts="b.f", ys="b.f", w="b.f", nt="7", stride="7", k="0", mass="M")

    def row(want, spoil="", **kw):
        a = dict(base, **kw)
        return (prelude + spoil, call % tuple(a[k] for k in ("m", "row0", "n", "ts", "ys", "w", "nt", "stride", "k", "mass")), want)
    check_table(tmp_path_factory, "coverage_counts", [
        row(OK), row(OK, "make_gk(b); "), row(OK, "b.m.prior = dist3(GLABC_DIST_DIAG_GAUSS); "), row(OK, k="1"), row(OK, stride="9"),
        row(OK, n="0"), row(OK, nt="0", stride="0"), row(OK, row0="(1ll << 32) + 12345"), row(OK, n="1ll << 30"), row(OK, nt="1ll << 20", stride="1ll << 20"),
        row(OK, "b.m.theta_dim = b.m.y_dim = b.m.prior.dim = 8; "), row(OK, "b.m.theta_dim = b.m.y_dim = b.m.prior.dim = 1; "),
        row(OK, "b.m.kern_scale = 0.0f; b.m.y_obs[0] = NaN; "),              # the parameters' values are not examined
        row(NULL, m="nullptr"), row(NULL, mass="nullptr"), row(NULL, ts="nullptr"), row(NULL, ys="nullptr"), row(NULL, w="nullptr"),
        row(NULL, "b.m.theta_dim = 9; ", mass="nullptr"), row(NULL, m="nullptr", n="-1"), row(NULL, "b.m.sim_kind = GLABC_SIM_USER; ", w="nullptr", k="2"),
        row(DIM, "b.m.theta_dim = 0; "), row(DIM, "b.m.theta_dim = b.m.y_dim = 9; "), row(DIM, "b.m.y_dim = 4; "),
        row(DIM, "make_gk(b); b.m.y_dim = 7; "), row(DIM, "b.m.theta_dim = 9; b.m.sim_kind = GLABC_SIM_USER; "),
        row(DIM, "b.m.y_dim = 4; b.m.prior.kind = GLABC_DIST_GAMMA; ", n="-1"),
        row(KIND, "b.m.sim_kind = GLABC_SIM_USER; "), row(KIND, "b.m.prior = dist3(GLABC_DIST_GAMMA); "), row(KIND, "b.m.prior.dim = 2; "),
        row(KIND, "b.m.sim_kind = GLABC_SIM_USER; ", n="-1"), row(KIND, "b.m.prior.dim = 2; ", k="2"),
        row(ARG, n="-1"), row(ARG, row0="-1"), row(ARG, nt="-1", stride="-1"), row(ARG, stride="6"), row(ARG, k="2"), row(ARG, k="-1"),
        row(ARG, n="(1ll << 30) + 1"), row(ARG, nt="(1ll << 20) + 1", stride="(1ll << 20) + 1"),
    ])


def test_resource_report_shows_no_private_segment():
    """profiles/coverage_kernel_resources.txt: nine instantiations of coverage_kernel, none with a private segment or a vector spill"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "profiles", "coverage_kernel_resources.txt")).read()
    kernels = re.split(r"^Function Name: ", text, flags=re.M)[1:]
    assert len(kernels) == 9 and all("coverage_kernel" in k for k in kernels)
    shapes = sorted(tuple(int(x) for x in re.search(r"coverage_kernelILi(\d)ELi(\d)E", k).groups()) for k in kernels)
    assert shapes == sorted([(d, d) for d in range(1, 9)] + [(4, 8)])
    for k in kernels:
        field = lambda name: int(re.search(r"%s: (\d+)" % re.escape(name), k).group(1))          # noqa: E731
        assert field("ScratchSize [bytes/lane]") == 0 and field("VGPRs Spill") == 0 and 0 < field("VGPRs") <= 256
        assert field("LDS Size [bytes/block]") <= 16384
