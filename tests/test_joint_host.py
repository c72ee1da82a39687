"""The joint posterior on the CPU: the NumPy restatement of glabc_histogram2d and glabc_cross_moments (tests/joint_ref.py) against
numpy.histogram2d, the marginal restatement, glabc_autocov's restatement and numpy.cov; the host formulas of
glabcmcmc_amd.diagnostics (combine_joint, covariance, correlation, hpd_levels, hpd_mask); every ValueError of the new functions;
the refusals of glabc_histogram2d / glabc_cross_moments as csrc/glabc_check.h answers them under g++; and the committed resource
report of the new kernels.

Counts are compared as equal integers and the diagonal of the cross moments as equal float64 bits.  The covariance has a
tolerance, see test_restatement_covariance_matches_numpy.
"""
import os
import re

import numpy as np
import pytest

import diag_ref as R
import joint_ref as J
import quantile_ref as Q
from glabcmcmc_amd import diagnostics as D
from test_arg_checks import check_table

OK, NULL, DIM, ARG = 0, -1, -2, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COV_TOLERANCE = 58.0              # units of eps sqrt(v_ii v_jj): 16 x the largest difference measured (3.64), see below


def all_pairs(d):
    return [(i, j) for i in range(d) for j in range(i + 1, d)]


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def host_terms(hist):
    """JointTerms of a chain-major history from the restatement's per-chain moments: what diagnostics.joint_terms sums on the device"""
    n_rows, d, m_chains = hist.shape
    mean, cov = J.cross_moments(hist)
    full = np.empty((d, d))
    for i in range(d):
        for j in range(i, d):
            full[i, j] = full[j, i] = cov[J.packed_index(i, j, d)].sum()
    return D.JointTerms(m_chains, n_rows, mean.sum(axis=1), mean @ mean.T, full)


def cov_units(got, want):
    """the largest |got - want| in units of eps sqrt(v_ii v_jj)"""
    sd = np.sqrt(np.diag(want))
    return float((np.abs(got - want) / (np.finfo(np.float64).eps * np.outer(sd, sd))).max())


# ---------------------------------------------------------------------------------- the restatement's counts
@pytest.mark.parametrize("lo, hi", [(0, 16), (-7, 9), (3, 4), (-64, 64)])
def test_restatement_grid_matches_numpy(lo, hi):
    """integers in float32, integer lo / hi, bins = hi - lo: the bin arithmetic is exact (test_restatement_histogram_matches_numpy
    of tests/test_quantile_host.py), so the grid must be numpy.histogram2d's"""
    rng = np.random.default_rng([lo + 100, hi + 100, 2])
    x = rng.integers(lo - 2, hi + 3, (40, 3, 23)).astype(np.float32)
    x[0, 0, :5] = hi                                                   # x == hi lands in the last bin
    x[1, 1, :5] = lo
    bins = hi - lo
    pairs = [(0, 1), (1, 0), (0, 2), (2, 1)]
    got = J.histogram2d(x, pairs, bins, [lo] * 3, [hi] * 3)
    for p, (a, b) in enumerate(pairs):
        va, vb = x[:, a].reshape(-1), x[:, b].reshape(-1)
        want, _, _ = np.histogram2d(va, vb, bins=bins, range=((lo, hi), (lo, hi)))
        assert np.array_equal(got[p, :bins * bins].reshape(bins, bins), want.astype(np.uint64)), (a, b)
        off = (va < lo) | (va > hi) | (vb < lo) | (vb > hi)
        assert got[p, bins * bins] == off.sum() and got[p, bins * bins + 1] == 0 and got[p].sum() == va.size
    x[2, 0, 0], x[3, 1, 1] = np.nan, np.nan
    x[4, 0, 2], x[4, 1, 2] = np.nan, lo - 2                            # a NaN beside a value outside counts as a NaN
    assert J.histogram2d(x, pairs, bins, [lo] * 3, [hi] * 3)[0, bins * bins + 1] == 3


@pytest.mark.parametrize("bins", (1, 2, 7, 128))
def test_margins_transposes_and_totals(bins):
    hist = R.diag_history(97, 3, 321)
    lo = hist.min(axis=(0, 2)).astype(np.float64)
    hi = hist.max(axis=(0, 2)).astype(np.float64)
    pairs = [(0, 1), (1, 0), (0, 2), (2, 0), (1, 2), (2, 1), (1, 2)]
    got = J.histogram2d(hist, pairs, bins, lo, hi)
    marg = Q.histogram(hist, bins, lo, hi)
    assert not marg[:, bins:].any()                                    # nothing outside, no NaN
    grids = got[:, :bins * bins].reshape(-1, bins, bins)
    for p, (a, b) in enumerate(pairs):
        assert np.array_equal(grids[p].sum(axis=1), marg[a, :bins]) and np.array_equal(grids[p].sum(axis=0), marg[b, :bins])
        assert np.array_equal(grids[p], grids[pairs.index((b, a))].T)
    assert np.array_equal(grids[4], grids[6])                         # a repeated pair: its own table, the same counts
    assert (got.sum(axis=1) == 97 * 321).all() and not got[:, bins * bins:].any()
    narrow = J.histogram2d(hist, pairs, bins, lo / 2, hi / 2)          # values outside, every slot still sums to T C
    assert (narrow.sum(axis=1) == 97 * 321).all() and narrow[:, bins * bins].all()


def test_special_values_fill_the_special_slots():
    hist = Q.special_history(33, 2, 65)
    got = J.histogram2d(hist, [(0, 1)], 4, [-1.0, 0.0], [1.0, 2.5])
    with np.errstate(invalid="ignore"):
        a, b = hist[:, 0].reshape(-1).astype(np.float64), hist[:, 1].reshape(-1).astype(np.float64)
        nan = np.isnan(a) | np.isnan(b)
        off = ~nan & ((a < -1.0) | (a > 1.0) | (b < 0.0) | (b > 2.5))
    assert got[0, 17] == nan.sum() > 0 and got[0, 16] == off.sum() > 0 and got[0].sum() == a.size
    assert got[0, 3 * 4 + 3] == ((a == 1.0) & (b == 2.5)).sum() + ((a > 0.5) & (a < 1.0) & (b == 2.5)).sum()          # x == hi: the last bin


# ---------------------------------------------------------------------------------- the restatement's moments
def test_restatement_diagonal_is_autocov_lag_zero():
    for shape in ((97, 3, 321), (33, 8, 65), (1, 2, 5), (2, 1, 3)):
        hist = R.diag_history(*shape)
        mean, cov = J.cross_moments(hist)
        want_mean, acov = R.autocov(hist, 0)
        d = shape[1]
        assert cov.shape == (d * (d + 1) // 2, shape[2]) and same_bits(mean, want_mean)
        for j in range(d):
            assert same_bits(cov[J.packed_index(j, j, d)], acov[0, j]), (shape, j)
    assert [J.packed_index(i, j, 3) for i in range(3) for j in range(i, 3)] == list(range(6))


def test_non_finite_values_stay_in_their_chain_and_coordinates():
    hist = np.array(R.diag_history(33, 3, 65))
    hist[5, 1, 7], hist[9, 2, 11] = np.nan, np.inf
    mean, cov = J.cross_moments(hist)
    clean_mean, clean_cov = J.cross_moments(R.diag_history(33, 3, 65))
    bad = ~same_rows(cov, clean_cov)
    want = np.zeros_like(bad)
    for i in range(3):
        for j in range(i, 3):
            want[J.packed_index(i, j, 3), 7] = 1 in (i, j)
            want[J.packed_index(i, j, 3), 11] |= 2 in (i, j)
    assert np.array_equal(bad, want) and np.isnan(cov[bad]).all()
    assert np.isnan(mean[1, 7]) and np.isinf(mean[2, 11]) and (np.isfinite(mean).sum() == mean.size - 2)
    assert clean_mean.shape == mean.shape


def same_rows(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


COV_SHAPES = ((1000, 4, 256, 50.0), (97, 8, 321, 50.0), (33, 3, 65, 50.0), (2, 2, 5, 50.0), (97, 2, 64, 0.0))


def test_restatement_covariance_matches_numpy():
    """The pooled formula from the restatement's per-chain moments against numpy.cov of the pooled float64 draws, in units of
    eps sqrt(v_ii v_jj).  NumPy's summation order is not specified, so the bound is 16 x the largest difference seen between the
    two references: measured 3.64 at (T, D, C) = (1000, 4, 256), 2.86 at (97, 8, 321), 0.67 at (33, 3, 65), 0.85 at (2, 2, 5) and
    0.68 at (97, 2, 64) without offsets; the largest seen is 3.64 and COV_TOLERANCE = 58 is 16 x that.  diagnostics.covariance of
    the same per-chain moments (the sum of outer products of the means where the restatement sums products of deviations; measured
    4.85 against numpy.cov and 2.90 against the restatement at the most) is held to the same bound against both references."""
    for n_rows, d, m_chains, offset in COV_SHAPES:
        hist = R.diag_history(n_rows, d, m_chains, offset)
        pooled = hist.transpose(0, 2, 1).reshape(-1, d).astype(np.float64)
        want = np.cov(pooled, rowvar=False).reshape(d, d)
        ref = J.covariance(hist)
        got = D.covariance(host_terms(hist))
        print("(%d, %d, %d): restatement against numpy.cov %.2f, diagnostics.covariance against numpy.cov %.2f, against the restatement "
              "%.2f eps sqrt(v_ii v_jj)" % (n_rows, d, m_chains, cov_units(ref, want), cov_units(got, want), cov_units(got, ref)))
        assert cov_units(ref, want) <= COV_TOLERANCE and cov_units(got, want) <= COV_TOLERANCE and cov_units(got, ref) <= COV_TOLERANCE
        assert np.array_equal(got, got.T) and np.array_equal(ref, ref.T)
        r = D.correlation(host_terms(hist))
        assert np.allclose(np.diag(r), 1.0, rtol=0, atol=4e-16) and np.allclose(r, np.corrcoef(pooled, rowvar=False).reshape(d, d), rtol=0, atol=1e-13)
        assert np.allclose(r, J.correlation(hist), rtol=0, atol=1e-13)


def test_combine_joint_of_two_shards_is_the_whole():
    hist = R.diag_history(97, 3, 321)
    whole = host_terms(hist)
    both = D.combine_joint([host_terms(hist[:, :, :130]), host_terms(hist[:, :, 130:])])
    assert both.M == 321 and both.n == 97
    assert cov_units(D.covariance(both), D.covariance(whole)) <= COV_TOLERANCE
    assert cov_units(D.covariance(both), J.covariance(hist)) <= COV_TOLERANCE
    lo, hi = np.full(3, -60.0), np.full(3, 60.0)
    pairs = all_pairs(3)
    parts = J.histogram2d(hist[:, :, :130], pairs, 7, lo, hi) + J.histogram2d(hist[:, :, 130:], pairs, 7, lo, hi)
    assert np.array_equal(parts, J.histogram2d(hist, pairs, 7, lo, hi))
    with pytest.raises(ValueError):
        D.combine_joint([whole, host_terms(hist[:50])])               # other n
    with pytest.raises(ValueError):
        D.combine_joint([whole, host_terms(R.diag_history(97, 2, 64))])          # other D
    with pytest.raises(ValueError):
        D.combine_joint([])


def test_correlation_of_a_constant_coordinate_is_nan():
    hist = np.array(R.diag_history(33, 3, 65))
    hist[:, 1, :] = np.float32(2.5)
    r = D.correlation(host_terms(hist))
    assert np.isnan(r[1]).all() and np.isnan(r[:, 1]).all() and r[0, 0] == 1.0 and np.isfinite(r[0, 2])
    assert same_bits(np.isnan(r), np.isnan(J.correlation(hist)))
    with pytest.raises(ValueError):
        D.covariance(D.JointTerms(1, 1, np.zeros(2), np.zeros((2, 2)), np.zeros((2, 2))))


# ---------------------------------------------------------------------------------- highest-density levels
def test_hpd_levels_on_a_grid_with_ties():
    grid = np.array([[5, 5, 1], [0, 3, 3], [2, 0, 1]], np.uint64)           # N = 20
    level, mass, inside = D.hpd_levels(grid, (0.25, 0.5, 0.55, 0.8, 0.85, 1.0))
    assert level.dtype == np.uint64 and mass.dtype == np.uint64 and inside.dtype.kind == "i"
    assert level.tolist() == [5, 5, 3, 3, 2, 1] and mass.tolist() == [10, 10, 16, 16, 18, 20] and inside.tolist() == [2, 2, 4, 4, 5, 7]
    assert np.array_equal(D.hpd_mask(grid, 0.55), grid >= 3) and D.hpd_mask(grid, 0.55).sum() == 4
    assert np.array_equal(D.hpd_mask(grid, 1.0), grid > 0)                   # p = 1: every occupied bin, no empty one
    one = np.zeros((4, 4), np.int64)
    one[2, 1] = 9
    for p in (1e-9, 0.5, 1.0):
        level, mass, inside = D.hpd_levels(one, p)
        assert (level.tolist(), mass.tolist(), inside.tolist()) == ([9], [9], [1])
    assert D.hpd_mask(one, 0.5).sum() == 1 and D.hpd_mask(one, 0.5)[2, 1]


def test_hpd_levels_hold_need_and_no_less_would():
    hist = R.diag_history(97, 3, 321)
    lo, hi = hist.min(axis=(0, 2)).astype(np.float64), hist.max(axis=(0, 2)).astype(np.float64)
    grids = J.histogram2d(hist, all_pairs(3), 7, lo, hi)[:, :49].reshape(3, 7, 7)
    probs = (0.5, 0.9, 0.95, 1.0, 1.0 / 3.0)
    level, mass, inside = D.hpd_levels(grids, probs)
    assert level.shape == mass.shape == inside.shape == (3, 5)
    for g in range(3):
        for i, p in enumerate(probs):
            need, v, m, k = J.hpd_level(grids[g], p)
            assert (int(level[g, i]), int(mass[g, i]), int(inside[g, i])) == (v, m, k), (g, p)
            assert m >= need and m - v * int((grids[g] == v).sum()) < need          # without its lowest level set: below need
            assert np.array_equal(D.hpd_mask(grids, p)[g], grids[g] >= v)
    single = D.hpd_levels(grids[1])                                    # one grid, the default probabilities
    assert [a.shape for a in single] == [(3,)] * 3 and np.array_equal(single[0], level[1, :3])
    assert D.hpd_levels(grids[None])[0].shape == (1, 3, 3)
    big = np.full((2, 2), 2 ** 60, np.uint64)                          # past 2^53: the sums are integers
    big[0, 0] += np.uint64(1)
    level, mass, inside = D.hpd_levels(big, (0.25, 1.0))
    assert level.tolist() == [2 ** 60 + 1, 2 ** 60] and inside.tolist() == [1, 4] and mass.tolist() == [2 ** 60 + 1, 2 ** 62 + 1]


def test_hpd_argument_errors():
    grid = np.ones((3, 3), np.uint64)
    for bad in (np.zeros((3, 3), np.uint64), np.ones(9, np.uint64), np.ones((3, 3)), -np.ones((3, 3), np.int64), np.zeros((0, 0), np.int64),
                np.stack([grid, np.zeros((3, 3), np.uint64)])):
        with pytest.raises(ValueError):
            D.hpd_levels(bad)
        with pytest.raises(ValueError):
            D.hpd_mask(bad, 0.5)
    for probs in (0.0, -0.1, 1.5, np.nan, (0.5, 0.0), [[0.5]], ()):
        with pytest.raises(ValueError):
            D.hpd_levels(grid, probs)
    with pytest.raises(ValueError):
        D.hpd_mask(grid, (0.5, 0.9))


# ---------------------------------------------------------------------------------- argument errors, no GPU needed
def test_argument_errors_come_before_any_device(monkeypatch):
    from glabcmcmc_amd import engine

    def no_device(*a, **k):
        raise AssertionError("an argument error must be raised before the device is asked for")
    monkeypatch.setattr(engine, "require_device", no_device)
    ok = np.zeros((10, 3, 2), np.float32)                                             # (T, C, D): D = 2
    ok3 = np.zeros((10, 2, 3), np.float32)
    for bins in (0, -1, 129, 2.5, True):
        with pytest.raises(ValueError):
            D.histogram2d(ok, None, bins)
    for rng in ((1.0, 1.0), (2.0, 1.0), (0.0, np.inf), (np.nan, 1.0), (0.0, 1.0, 2.0), 3.0, np.zeros((3, 2)), "ab"):
        with pytest.raises(ValueError):
            D.histogram2d(ok, None, 8, rng)
    for pairs in ([(0, 0)], [(0, 2)], [(-1, 0)], [(0, 1, 1)], [0, 1], [], [(0.0, 1.0)], [(0, 1), (1, 1)], 5):
        with pytest.raises(ValueError):
            D.histogram2d(ok, pairs)
    with pytest.raises(ValueError):
        D.histogram2d(ok3, [(0, 3)])
    with pytest.raises(ValueError):
        D.histogram2d(np.zeros((10, 3, 1), np.float32))                               # D == 1: no pair
    with pytest.raises(ValueError):
        D.histogram2d(np.zeros((10, 1), np.float32), [(0, 0)])
    for call in (D.covariance, D.correlation):
        with pytest.raises(ValueError):
            call(np.zeros((1, 1, 2), np.float32))                                     # one draw
    for call in (D.histogram2d, D.cross_moments, D.joint_terms, D.covariance, D.correlation):
        for bad in (np.zeros(5, np.float32), np.zeros((5, 2, 2, 2), np.float32), np.zeros((10, 3, 9), np.float32), np.zeros((0, 3, 2), np.float32)):
            with pytest.raises(ValueError):
                call(bad)
        with pytest.raises(ValueError):
            call(ok, layout="columns")


def test_no_cpu_fallback():
    """Without a GPU the new functions raise; they never compute on the host"""
    import torch
    if not torch.cuda.is_available():
        ok = np.zeros((10, 3, 2), np.float32)
        for call in (lambda: D.histogram2d(ok), lambda: D.histogram2d(ok, [(1, 0)], 8, (0.0, 1.0)), lambda: D.cross_moments(ok),
                     lambda: D.joint_terms(ok), lambda: D.covariance(ok), lambda: D.correlation(ok)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()


def test_entry_points_are_bound():
    from glabcmcmc_amd import _capi
    assert "glabc_histogram2d" in _capi.ENTRY_POINTS and "glabc_cross_moments" in _capi.ENTRY_POINTS
    assert len(_capi.ENTRY_POINTS["glabc_histogram2d"][1]) == 12 and len(_capi.ENTRY_POINTS["glabc_cross_moments"][1]) == 8
    assert _capi.VERSION == 301
    assert D.MAX_PAIRS == 28 == _capi.MAX_DIM * (_capi.MAX_DIM - 1) // 2 and D.MAX_JOINT_BINS == 128
    header = open(os.path.join(ROOT, "include", "glabc.h")).read()
    assert "#define GLABC_MAX_PAIRS 28" in header and "#define GLABC_MAX_JOINT_BINS 128" in header and "#define GLABC_VERSION 301" in header
    doc = D.__doc__.split("Out of scope")[1]
    assert "joint histograms" not in doc and "weighted draws" in doc and "rank-normalised" in doc and "multivariate ESS" in doc


# ---------------------------------------------------------------------------------- the refusals (csrc/glabc_check.h)
PRELUDE_TABLES = ("static const int32_t PR[6] = {0, 1, 1, 0, 0, 1}; static const int32_t P02[4] = {0, 2, 2, 1}; static int32_t ALL[56]; "
                  "static const int32_t SAME[4] = {0, 1, 1, 1}; static const int32_t HIGH[4] = {0, 1, 0, 3}; static const int32_t NEG[4] = {0, 1, -1, 2}; "
                  "static const int32_t LATE[56] = {0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, "
                  "0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 2, 2}; "
                  "static uint64_t CNT[4]; static double OUT[4]; "
                  "static const double LO[3] = {-1.0, 0.0, 5.0}, HI[3] = {1.0, 1e-300, 6.0}; "
                  "static const double BAD_EQ[3] = {-1.0, 1e-300, 5.0}, BAD_NAN[3] = {-1.0, NAN, 5.0}, BAD_INF[3] = {-1.0, 0.0, -INFINITY}, "
                  "HI_INF[3] = {1.0, INFINITY, 6.0}, BAD_REV[3] = {2.0, 0.0, 5.0}, HI_NAN2[3] = {1.0, 1e-300, NAN}; "
                  "for (int i = 0; i < 28; ++i) { ALL[2 * i] = i % 3; ALL[2 * i + 1] = (i + 1 + i / 3 % 2) % 3; } ")


def test_check_histogram2d(tmp_path_factory):
    call = "check_histogram2d(%s, %s, %s, %s, %s, %s, %s, %s, %s, %s, %s)"
    base = dict(h="b.f", rows="97", d="3", n="65", stride="65", np="3", p="PR", bins="64", lo="LO", hi="HI", c="CNT")

    def row(want, **kw):
        a = dict(base, **kw)
        return (PRELUDE_TABLES, call % (a["h"], a["rows"], a["d"], a["n"], a["stride"], a["np"], a["p"], a["bins"], a["lo"], a["hi"], a["c"]), want)
    check_table(tmp_path_factory, "histogram2d", [
        row(OK), row(OK, bins="1"), row(OK, bins="128"), row(OK, rows="1"), row(OK, stride="82"), row(OK, n="0", stride="0"), row(OK, np="1"),
        row(OK, np="2", p="P02"), row(OK, np="28", p="ALL"), row(OK, d="2"),
        row(OK, lo="BAD_INF"), row(OK, hi="HI_NAN2"), row(OK, d="2", lo="BAD_INF"),          # coordinate 2: no pair of PR uses it
        row(NULL, h="nullptr"), row(NULL, p="nullptr"), row(NULL, lo="nullptr"), row(NULL, hi="nullptr"), row(NULL, c="nullptr"),
        row(NULL, h="nullptr", d="0"), row(NULL, c="nullptr", bins="0"), row(NULL, p="nullptr", np="0"),          # a null pointer is reported first
        row(DIM, d="0"), row(DIM, d="9"), row(DIM, d="-1"), row(DIM, d="9", rows="0"), row(DIM, d="0", bins="0"), row(DIM, d="0", np="0"),          # then the dimension
        row(ARG, rows="0"), row(ARG, rows="-5"), row(ARG, n="-1"), row(ARG, stride="64"),
        row(ARG, np="0"), row(ARG, np="-1"), row(ARG, np="29", p="ALL"),
        row(ARG, np="2", p="SAME"), row(ARG, np="2", p="HIGH"), row(ARG, np="2", p="NEG"), row(ARG, np="2", p="P02", d="2"), row(ARG, np="28", p="LATE"),
        row(OK, np="1", p="SAME"), row(OK, np="27", p="LATE"),          # only the first n_pairs pairs are looked at
        row(ARG, bins="0"), row(ARG, bins="-1"), row(ARG, bins="129"),
        row(ARG, lo="BAD_EQ"), row(ARG, lo="BAD_NAN"), row(ARG, hi="BAD_NAN"), row(ARG, hi="HI_INF"), row(ARG, lo="BAD_REV"), row(ARG, lo="HI", hi="LO"),
        row(ARG, np="2", p="P02", lo="BAD_INF"), row(ARG, np="2", p="P02", hi="HI_NAN2"),          # a pair uses coordinate 2 now
    ])


def test_check_cross_moments(tmp_path_factory):
    call = "check_cross_moments(%s, %s, %s, %s, %s, %s, %s)"
    base = dict(h="b.f", rows="97", d="3", n="65", stride="65", m="OUT", v="OUT")

    def row(want, **kw):
        a = dict(base, **kw)
        return (PRELUDE_TABLES, call % (a["h"], a["rows"], a["d"], a["n"], a["stride"], a["m"], a["v"]), want)
    check_table(tmp_path_factory, "cross_moments", [
        row(OK), row(OK, rows="1"), row(OK, stride="82"), row(OK, n="0", stride="0"), row(OK, d="1"), row(OK, d="8"),
        row(NULL, h="nullptr"), row(NULL, m="nullptr"), row(NULL, v="nullptr"), row(NULL, h="nullptr", d="0"), row(NULL, v="nullptr", rows="0"),
        row(DIM, d="0"), row(DIM, d="9"), row(DIM, d="-1"), row(DIM, d="9", rows="0"),
        row(ARG, rows="0"), row(ARG, rows="-5"), row(ARG, n="-1"), row(ARG, stride="64"),
    ])


# ---------------------------------------------------------------------------------- the committed resource report
def test_resource_report_shows_no_private_segment():
    """profiles/joint_kernel_resources.txt: joint_kernel and every cross_kernel<D> without a private segment or a spilled register"""
    text = open(os.path.join(ROOT, "profiles", "joint_kernel_resources.txt")).read()
    kernels = re.split(r"^Function Name: ", text, flags=re.M)[1:]
    assert sum("joint_kernel" in k for k in kernels) >= 1
    assert sorted(int(re.search(r"cross_kernelILi(\d)E", k).group(1)) for k in kernels if "cross_kernel" in k) == list(range(1, 9))
    for k in kernels:
        field = lambda name: int(re.search(r"%s: (\d+)" % re.escape(name), k).group(1))          # noqa: E731
        assert field("ScratchSize [bytes/lane]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0, k.splitlines()[0]
        assert "Dynamic Stack: False" in k
