"""Summaries of weighted draws on the CPU: the NumPy restatement (tests/weighted_ref.py) against
numpy.quantile(weights=, method="inverted_cdf"), numpy.histogram and numpy.histogram2d; the quantisation rule; every ValueError of
``weighted.quantize``; the generic path of every public function of glabcmcmc_amd.weighted on CPU tensors against the restatement;
the exact rank of a multiset of more than 2^53 elements; the refusals of the three entry points as csrc/glabc_check.h answers them
under g++; and the committed resource report of the kernels.

Tolerances: none.  Counts are equal integers, order statistics and quantiles equal values (NaN matching NaN).
"""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import joint_ref as J
import quantile_ref as Q
import weighted_ref as W
from glabcmcmc_amd import _capi, regression, rejection, smc, weighted
from glabcmcmc_amd import diagnostics as D
from test_arg_checks import check_table

OK, NULL, DIM, ARG = 0, -1, -2, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = (0.0, 1e-9, 0.25, 0.5, 0.77, 1.0)


def same_values(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def integer_draws(n, d, lo, hi, seed):
    """integers in float32 (ties throughout), some outside [lo, hi]"""
    rng = np.random.default_rng(seed)
    return rng.integers(lo - 3, hi + 4, size=(d, n)).astype(np.float32)


def small_multiplicities(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 6, size=n).astype(np.uint64) * (rng.random(n) < 0.8)


# ---------------------------------------------------------------------------------- the restatement against NumPy
def test_restatement_quantile_matches_numpy_inverted_cdf():
    rng = np.random.default_rng(1)
    for n, seed in ((1, 2), (7, 3), (200, 4), (1000, 5)):
        x = rng.standard_normal((3, n)).astype(np.float32)
        x[1] = np.round(x[1] * 2) / 2                                # ties, and both zeros
        x[1, ::5] = np.float32(-0.0)
        x[2, n // 2] = np.inf
        x[2, 0] = -np.inf
        m = small_multiplicities(n, seed)
        m[0] = max(int(m[0]), 1)
        got = W.quantile(x, m, QS)
        for j in range(3):
            want = np.quantile(x[j].astype(np.float64), QS, weights=m.astype(np.float64), method="inverted_cdf")
            assert same_values(got[:, j], want), (n, j, got[:, j], want)
    # a NaN that carries weight makes the coordinate's quantiles NaN, as NumPy's; one that carries none is skipped
    x = np.array([[1.0, np.nan, 3.0, 2.0], [1.0, np.nan, 3.0, 2.0]], np.float32)
    assert np.isnan(W.quantile(x, np.array([1, 2, 1, 1], np.uint64), QS)).all()
    assert same_values(W.quantile(x, np.array([1, 0, 1, 1], np.uint64), (0.0, 0.5, 1.0)), [[1.0, 1.0], [2.0, 2.0], [3.0, 3.0]])


@pytest.mark.parametrize("lo, hi", [(0, 16), (-7, 9), (3, 4), (-64, 64)])
def test_restatement_histograms_match_numpy(lo, hi):
    """integers in float32, integer lo / hi, bins = hi - lo: the bin arithmetic is exact, so the weighted counts must be NumPy's"""
    bins, n = hi - lo, 3000
    x = integer_draws(n, 3, lo, hi, 7)
    m = small_multiplicities(n, 8)
    got = W.histogram(x, m.astype(np.float32), 1.0, bins, [lo] * 3, [hi] * 3)
    for j in range(3):
        want, _ = np.histogram(x[j], bins=bins, range=(lo, hi), weights=m.astype(np.float64))
        assert np.array_equal(got[j, :bins], want.astype(np.uint64))
        assert got[j, bins] == m[x[j] < lo].sum() and got[j, bins + 1] == m[x[j] > hi].sum() and got[j, bins + 2] == 0
    pairs = [(0, 1), (2, 0), (1, 0)]
    grid = W.histogram2d(x, m.astype(np.float32), 1.0, pairs, bins, [lo] * 3, [hi] * 3)
    for p, (a, b) in enumerate(pairs):
        want, _, _ = np.histogram2d(x[a], x[b], bins=bins, range=((lo, hi), (lo, hi)), weights=m.astype(np.float64))
        assert np.array_equal(grid[p, :bins * bins].reshape(bins, bins), want.astype(np.uint64)), (a, b)
        off = (x[a] < lo) | (x[a] > hi) | (x[b] < lo) | (x[b] > hi)
        assert grid[p, bins * bins] == m[off].sum() and grid[p, bins * bins + 1] == 0
    assert np.array_equal(grid[1, :bins * bins].reshape(bins, bins), np.histogram2d(x[2], x[0], bins=bins, range=((lo, hi), (lo, hi)),
                                                                                 weights=m.astype(np.float64))[0].astype(np.uint64))


def test_restatement_with_unit_weights_is_the_unweighted_restatement():
    hist = np.array(Q.special_history(1, 3, 321))
    x, ones = hist[0], np.ones(321, np.float32)
    for level, table in ((0, None), (1, [[0x400, 0x3FF], [0x5FC, 0x400], [0x7FF, 0x1]]), (2, [[0x3F9ABC], [0x2FE000], [Q.UNUSED]])):
        assert np.array_equal(W.key_counts(x, ones, 1.0, level, table), Q.key_counts(hist, level, table))
    lo, hi = [-1.0, 0.0, -3.5], [1.0, 2.5, 42.0]
    with np.errstate(invalid="ignore"):                               # a signalling NaN among the special values
        assert np.array_equal(W.histogram(x, ones, 1.0, 5, lo, hi), Q.histogram(hist, 5, lo, hi))
    assert np.array_equal(W.histogram2d(x, ones, 1.0, [(0, 1), (2, 1)], 4, lo, hi), J.histogram2d(hist, [(0, 1), (2, 1)], 4, lo, hi))


def test_zero_weight_keeps_a_nan_out_of_the_nan_slots():
    x = np.array([[np.nan, 1.0, np.nan, 0.5], [0.25, np.nan, 0.75, 0.5]], np.float32)
    w = np.array([0.0, 2.0, -1.0, 3.0], np.float32)
    assert W.key_counts(x, w, 1.0, 0)[:, 0, -1].tolist() == [0, 2]
    assert W.histogram(x, w, 1.0, 2, [0.0, 0.0], [1.0, 1.0]).tolist() == [[0, 5, 0, 0, 0], [0, 3, 0, 0, 2]]
    assert W.histogram2d(x, w, 1.0, [(0, 1)], 2, [0.0, 0.0], [1.0, 1.0])[0].tolist() == [0, 0, 0, 3, 0, 2]


# ---------------------------------------------------------------------------------- the quantisation rule
def test_quantisation_rule():
    rule = lambda w, scale: W.multiplicity(np.array(w, np.float32), scale).tolist()          # noqa: E731
    assert rule([0.5, 1.5, 2.5, 3.5], 1.0) == [0, 2, 2, 4]                                    # ties to even
    assert rule([0.25, 0.75, 1.25], 2.0) == [0, 2, 2]
    assert rule([-0.0, 0.0, -1.0, np.nan, -np.inf], 1e6) == [0, 0, 0, 0, 0]
    below = np.nextafter(np.float32(2.0 ** 32), np.float32(0))                                # 2^32 - 256, the largest float32 below 2^32
    assert rule([below, 2.0 ** 32, np.inf, 3.0e38], 1.0) == [2 ** 32 - 256, 2 ** 32 - 1, 2 ** 32 - 1, 2 ** 32 - 1]
    assert rule([1.0], 4294967294.5) == [4294967294] and rule([1.0], 4294967294.75) == [4294967295]          # rint below the clamp
    assert rule([1.0], 4294967295.0) == [2 ** 32 - 1] and rule([1.0], 1e300) == [2 ** 32 - 1]
    assert rule([1e-45], 1e-300) == [0]                                                       # a product that underflows
    # the module's rule is the restatement's
    w = np.array([0.5, 1.5, 2.5, -0.0, -3.0, np.nan, 7.25, 1e-30], np.float32)
    for scale in (1.0, 2.0, 3.7, 2.0 ** 28):
        assert weighted._multiplicity(torch.from_numpy(w), scale).tolist() == W.multiplicity(w, scale).tolist()
    big = torch.tensor([float(below), 2.0 ** 32, 3.0e38])
    assert weighted._multiplicity(big, 1.0).tolist() == [2 ** 32 - 256, 2 ** 32 - 1, 2 ** 32 - 1]


def test_default_scale_reproduces_weights_exactly():
    rng = np.random.default_rng(11)
    for top in (1.0, 0.37, 3.0e-5, 1.7e12, float(np.float32(2.0 ** -126))):
        w = (rng.random(4000) * top).astype(np.float32)
        w[0] = np.float32(top)
        m, scale = weighted.quantize(torch.from_numpy(w))
        m = m.numpy()
        assert scale == W.default_scale(w) and math.frexp(scale)[0] == 0.5                    # a power of two
        assert 2 ** 31 <= int(m.max()) < 2 ** 32 and np.array_equal(m.astype(np.uint64), W.multiplicity(w, scale))
        exact = w >= np.float32(top) * np.float32(2.0 ** -8)
        assert exact.sum() > 3900 and np.array_equal((m[exact].astype(np.float64) / scale).astype(np.float32), w[exact])
        assert (np.abs(m.astype(np.float64) / scale - w.astype(np.float64)) <= 0.5 / scale).all()


def test_quantize_raises():
    ok = torch.tensor([0.25, 0.0, 0.5])
    m, scale = weighted.quantize(ok)
    assert m.dtype == torch.int64 and m.tolist() == [2 ** 30, 0, 2 ** 31] and scale == 2.0 ** 32
    assert weighted.quantize(ok, 8.0)[0].tolist() == [2, 0, 4] and weighted.quantize(ok.double(), 8)[1] == 8.0
    for bad in ([0.5, float("nan")], [0.5, float("inf")], [0.5, -0.25], [0.5, float("-inf")], [0.0, 0.0], [-0.0], []):
        with pytest.raises(ValueError):
            weighted.quantize(torch.tensor(bad))
    for scale in (0.0, -1.0, float("nan"), float("inf"), 2.0 ** 33, 4294967295.0 * 2, "8", True):
        with pytest.raises(ValueError):
            weighted.quantize(ok, scale)
    assert weighted.quantize(ok, 2.0 ** 32)[0].tolist() == [2 ** 30, 0, 2 ** 31]             # the largest weight stays below the clamp


# ---------------------------------------------------------------------------------- the generic path against the restatement
def draws_and_weights(n=777, d=3, seed=5):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((d, n)).astype(np.float32)
    x[1] = np.round(x[1] * 4) / 4
    x[1, ::7] = np.float32(-0.0)
    x[2, 5], x[0, 9] = np.nan, np.nan                                # both on draws of weight 0, below
    w = rng.random(n).astype(np.float32) ** 3
    w[::11] = 0.0
    w[5] = w[9] = 0.0
    return x, w


def test_generic_path_matches_the_restatement():
    x, w = draws_and_weights()
    theta, wt = torch.from_numpy(np.ascontiguousarray(x.T)), torch.from_numpy(w)
    m, scale = weighted.quantize(wt)
    assert np.array_equal(m.numpy().astype(np.uint64), W.multiplicity(w, scale))
    for s in (None, 1000.0):
        sc = scale if s is None else s
        mm = W.multiplicity(w, sc)
        total = int(mm.sum())
        assert np.array_equal(weighted.key_counts((theta, wt), 0, scale=s), W.key_counts(x, w, sc, 0))
        table = np.array([[0x400, 0x3FF, Q.UNUSED], [0x3FF, 0x7F3, 0x400], [0x5FC, 0x400, 0x3FF]], np.uint32)
        assert np.array_equal(weighted.key_counts((theta, wt), 1, table, scale=s), W.key_counts(x, w, sc, 1, table))
        got = weighted.quantile((theta, wt), QS, scale=s)
        assert got.dtype == np.float64 and same_values(got, W.quantile(x, mm, QS))
        ranks = [0, 1, total // 3, total // 2, total - 1]
        want = np.array([[W.order_statistic(x[j], mm, r) for j in range(3)] for r in ranks], np.float32)
        got = weighted.order_statistics((theta, wt), ranks, scale=s)
        assert got.dtype == np.float32 and same_values(got, want)
        lower, upper = weighted.interval((theta, wt), 0.9, scale=s)
        both = W.quantile(x, mm, ((1.0 - 0.9) / 2.0, (1.0 + 0.9) / 2.0))
        assert same_values(lower, both[0]) and same_values(upper, both[1])
        lo, hi = np.array([-1.0, -0.5, 0.0]), np.array([1.0, 2.0, 0.75])
        for bins in (1, 7, 64):
            h = weighted.histogram((theta, wt), bins, np.stack([lo, hi], axis=1), scale=s)
            want = W.histogram(x, w, sc, bins, lo, hi)
            assert isinstance(h, D.Histogram) and h.counts.dtype == np.uint64
            assert np.array_equal(h.counts, want[:, :bins]) and np.array_equal(h.below, want[:, bins])
            assert np.array_equal(h.above, want[:, bins + 1]) and np.array_equal(h.nan, want[:, bins + 2]) and not h.nan.any()
            assert (h.counts.sum(axis=1) + h.below + h.above == total).all()
            pairs = [(0, 1), (2, 1), (1, 0), (0, 1)]
            g = weighted.histogram2d((theta, wt), pairs, bins, np.stack([lo, hi], axis=1), scale=s)
            want = W.histogram2d(x, w, sc, pairs, bins, lo, hi)
            assert isinstance(g, D.JointHistogram) and np.array_equal(g.counts.reshape(4, -1), want[:, :bins * bins])
            assert np.array_equal(g.outside, want[:, bins * bins]) and not g.nan.any()
            assert np.array_equal(g.counts[0], g.counts[2].T) and np.array_equal(g.counts[0], g.counts[3])
        # range=None: the exact extremes of the draws that carry weight
        keep = mm > 0
        lim = np.stack([[np.nanmin(x[j][keep]), np.nanmax(x[j][keep])] for j in range(3)]).astype(np.float64)
        h = weighted.histogram((theta, wt), 16, scale=s)
        assert np.array_equal(h.edges[:, 0], lim[:, 0]) and np.array_equal(h.edges[:, -1], lim[:, 1])
        assert np.array_equal(h.counts, W.histogram(x, w, sc, 16, lim[:, 0], lim[:, 1])[:, :16]) and not h.below.any() and not h.above.any()
        g = weighted.histogram2d((theta, wt), None, 8, scale=s)
        want = W.histogram2d(x, w, sc, [(0, 1), (0, 2), (1, 2)], 8, lim[:, 0], lim[:, 1])
        assert np.array_equal(g.counts.reshape(3, -1), want[:, :64]) and not g.outside.any()
        # the grids go to hpd_levels as they are
        level, mass, inside = D.hpd_levels(g.counts, (0.5, 0.9))
        for p in range(3):
            for i, prob in enumerate((0.5, 0.9)):
                need, v, ms, cnt = J.hpd_level(want[p, :64], prob)
                assert (int(level[p, i]), int(mass[p, i]), int(inside[p, i])) == (v, ms, cnt)
        assert D.hpd_mask(g.counts[0], 0.9).shape == (8, 8)


def test_summary_terms_and_combine():
    x, w = draws_and_weights()
    theta, wt = torch.from_numpy(np.ascontiguousarray(x.T)), torch.from_numpy(w)
    s = weighted.summary((theta, wt))
    mm = W.multiplicity(w, s["scale"])
    total, sum_sq = sum(int(v) for v in mm.tolist()), sum(int(v) ** 2 for v in mm.tolist())
    assert s["M"] == total and isinstance(s["M"], int) and s["scale"] == W.default_scale(w)
    assert s["ess"] == float(Fraction(total * total, sum_sq)) and 1.0 < s["ess"] < 777
    assert same_values(s["quantiles"], W.quantile(x, mm, (0.025, 0.5, 0.975)))
    keep = mm > 0
    p = mm[keep].astype(np.float64) / total
    mean = (p[None, :] * x[:, keep].astype(np.float64)).sum(axis=1)
    sd = np.sqrt((p[None, :] * (x[:, keep].astype(np.float64) - mean[:, None]) ** 2).sum(axis=1))
    assert np.allclose(s["mean"], mean, rtol=1e-12, atol=1e-14) and np.allclose(s["sd"], sd, rtol=1e-9)
    # shards under one explicit scale add up to the whole
    whole = weighted.terms((theta, wt), s["scale"])
    parts = [weighted.terms((theta[a:b], wt[a:b]), s["scale"]) for a, b in ((0, 100), (100, 101), (101, 777))]
    both = weighted.combine(parts)
    assert (both.M, both.sum_m2, both.n) == (whole.M, whole.sum_m2, 777) == (total, sum_sq, 777)
    assert np.allclose(both.sum_mx, whole.sum_mx, rtol=1e-12) and np.allclose(both.sum_mxx, whole.sum_mxx, rtol=1e-12)
    assert np.allclose(weighted.moments(both)[0], s["mean"], rtol=1e-12, atol=1e-14)
    counts = sum(weighted.key_counts((theta[a:b], wt[a:b]), 0, scale=s["scale"]) for a, b in ((0, 100), (100, 101), (101, 777)))
    assert np.array_equal(counts, weighted.key_counts((theta, wt), 0, scale=s["scale"]))
    with pytest.raises(ValueError):
        weighted.terms((theta, wt), None)
    with pytest.raises(ValueError):
        weighted.combine([whole, weighted.terms((theta, wt), 2.0 * s["scale"] / 4.0)])
    # sum m^2 does not overflow where an int64 sum of squares would: 300 draws of multiplicity 2^32 - 256
    big = weighted.terms((torch.zeros(300, 1), torch.full((300,), float(np.nextafter(np.float32(2.0 ** 32), np.float32(0))))), 1.0)
    assert big.M == 300 * (2 ** 32 - 256) and big.sum_m2 == 300 * (2 ** 32 - 256) ** 2 > 2 ** 63


def test_every_kind_of_draws_is_accepted():
    x, w = draws_and_weights(n=200)
    theta, wt = torch.from_numpy(np.ascontiguousarray(x.T)), torch.from_numpy(w)
    y, dis = torch.zeros(200, 2), torch.zeros(200)
    want = weighted.quantile((theta, wt), QS)
    pop = smc.Population(theta, y, dis, wt.double(), 0.1, 50.0, 3)
    adj = regression.Adjusted(theta, wt.double(), None, None, None, None, 50.0, 1.0, 0.0, None)
    for draws in (pop, adj, [theta, wt], (theta.numpy(), w), (theta.double(), wt)):
        assert same_values(weighted.quantile(draws, QS), want)
    # dimension-major storage, as rejection.sample returns it, is the same draws
    assert same_values(weighted.quantile((torch.from_numpy(x).t(), wt), QS), want)
    # a Rejection has unit weights: with scale 1 the counts are those of the unweighted restatement on the one-row history
    clean = np.where(np.isnan(x), np.float32(0.5), x)
    rej = rejection.Rejection(torch.from_numpy(np.ascontiguousarray(clean.T)), y, dis, torch.arange(200), 0.1, 1000)
    hist = clean[None]
    assert np.array_equal(weighted.key_counts(rej, 0, scale=1.0), Q.key_counts(hist, 0))
    lo, hi = [-1.0, -1.0, -1.0], [1.0, 1.5, 2.0]
    h = weighted.histogram(rej, 9, np.stack([lo, hi], axis=1), scale=1.0)
    assert np.array_equal(np.column_stack([h.counts, h.below, h.above, h.nan]), Q.histogram(hist, 9, lo, hi))
    g = weighted.histogram2d(rej, [(0, 2)], 9, np.stack([lo, hi], axis=1), scale=1.0)
    assert np.array_equal(g.counts.reshape(-1), J.histogram2d(hist, [(0, 2)], 9, lo, hi)[0, :81])
    s = np.sort(clean, axis=1)
    assert same_values(weighted.order_statistics(rej, [0, 99, 199], scale=1.0), s[:, [0, 99, 199]].T)
    assert same_values(weighted.quantile(rej, (0.0, 0.5, 1.0)), s[:, [0, 99, 199]].T.astype(np.float64))          # the default scale too


def test_argument_errors():
    theta, w = torch.zeros(10, 2), torch.ones(10)
    for bad in (theta, (theta,), (theta, w, w), (torch.zeros(10), w), (torch.zeros(10, 9), w), (torch.zeros(10, 0), w), (theta, torch.ones(9)),
                "draws", None):
        with pytest.raises(ValueError):
            weighted.quantile(bad, 0.5)
    for call in (lambda: weighted.quantile((theta, w), 1.5), lambda: weighted.quantile((theta, w), 0.5, path="fast"),
                 lambda: weighted.quantile((theta, w), 0.5, path="fused"), lambda: weighted.interval((theta, w), 1.0),
                 lambda: weighted.histogram((theta, w), 0), lambda: weighted.histogram((theta, w), 4097), lambda: weighted.histogram((theta, w), 8, (1.0, 1.0)),
                 lambda: weighted.histogram2d((theta, w), None, 129), lambda: weighted.histogram2d((theta, w), [(0, 0)]),
                 lambda: weighted.histogram2d((torch.zeros(10, 1), w)), lambda: weighted.order_statistics((theta, w), [-1]),
                 lambda: weighted.order_statistics((theta, w), [10 * 2 ** 31]), lambda: weighted.key_counts((theta, w), 3),
                 lambda: weighted.quantile((theta, torch.zeros(10)), 0.5), lambda: weighted.quantile((theta, -w), 0.5),
                 lambda: weighted.quantile((torch.zeros(0, 2), torch.ones(0)), 0.5), lambda: weighted.summary((theta, w), scale=2.0 ** 33)):
        with pytest.raises(ValueError):
            call()
    assert weighted.histogram((theta, w), 4).counts[:, 2].tolist() == [10 * 2 ** 31] * 2          # a constant coordinate, widened by +-0.5


# ---------------------------------------------------------------------------------- the exact rank
def test_rank_is_exact_beyond_2_to_53():
    """M = 2^54 + 2, which no float64 holds: the float64 product 0.5 M is 2^53 and its rank 2^53 - 1, the exact rank is 2^53.  A
    multiset of 2^53 ones and 2^53 + 2 twos has its boundary between the two: select, fed that multiset's digit counts, must
    return 2.0 at the median where the float64 rank gives 1.0"""
    ones, twos = 2 ** 53, 2 ** 53 + 2
    total = ones + twos
    assert float(total) != total
    exact = weighted._rank(0.5, total)
    assert exact == 2 ** 53 == W.quantile_rank(0.5, total) == math.ceil(Fraction(1, 2) * total) - 1
    assert max(int(math.ceil(0.5 * float(total))), 1) - 1 == 2 ** 53 - 1 != exact             # what a float64 product would pick
    members = [(int(Q.keys(np.array([1.0], np.float32))[0]), ones), (int(Q.keys(np.array([2.0], np.float32))[0]), twos)]
    calls = []

    def count_fn(level, prefixes):
        calls.append(level)
        prefix_bits, digit_bits = D.KEY_LEVELS[level]
        table = [0] if prefixes is None else [int(p) for p in prefixes[0]]
        out = np.zeros((1, len(table), 1 << digit_bits), np.uint64)
        for k, copies in members:
            for s, p in enumerate(table):
                if level == 0 or k >> (32 - prefix_bits) == p:
                    out[0, s, (k >> (32 - prefix_bits - digit_bits)) & ((1 << digit_bits) - 1)] += np.uint64(copies)
        return out
    got = weighted._quantile(count_fn, np.array([0.0, 0.5, 1.0]))
    assert got.tolist() == [[1.0], [2.0], [2.0]] and calls == [0, 1, 2]
    assert weighted.select(count_fn, ranks=[2 ** 53 - 1, 2 ** 53]).tolist() == [[1.0], [2.0]]


# ---------------------------------------------------------------------------------- the binding and the documents
def test_entry_points_are_bound():
    names = ("glabc_weighted_key_counts", "glabc_weighted_histogram", "glabc_weighted_histogram2d")
    assert set(names) <= set(_capi.ENTRY_POINTS) and _capi.VERSION == 301 and _capi.STREAM_LAYOUT == 2
    assert [len(_capi.ENTRY_POINTS[k][1]) for k in names] == [11, 11, 13]
    for name, twin in zip(names, ("glabc_key_counts", "glabc_histogram", "glabc_histogram2d")):
        assert len(_capi.ENTRY_POINTS[name][1]) == len(_capi.ENTRY_POINTS[twin][1]) + 1          # no n_rows; w and scale
    header = open(os.path.join(ROOT, "include", "glabc.h")).read()
    assert "#define GLABC_MAX_WEIGHTED_DRAWS 2147483648ll" in header and weighted.MAX_DRAWS == 2 ** 31
    import glabcmcmc_amd
    assert glabcmcmc_amd.weighted is weighted and "weighted" in glabcmcmc_amd.__all__
    assert weighted.select is D.select


def test_kernel_resource_report():
    """profiles/weighted_kernel_resources.txt: every weighted kernel without a private segment or a spilled register"""
    text = open(os.path.join(ROOT, "profiles", "weighted_kernel_resources.txt")).read()
    kernels = re.split(r"^Function Name: ", text, flags=re.M)[1:]
    assert sum("weighted_joint_kernel" in k for k in kernels) == 1
    assert sorted(int(re.search(r"KeySlotsILi(\d)E", k).group(1)) for k in kernels if "KeySlots" in k) == [0, 1, 2, 4, 8]
    assert sum("HistSlots" in k for k in kernels) == 1 and len(kernels) == 7
    for k in kernels:
        field = lambda name: int(re.search(r"%s: (\d+)" % re.escape(name), k).group(1))          # noqa: E731
        assert field("ScratchSize [bytes/lane]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0, k.splitlines()[0]
        assert "Dynamic Stack: False" in k


# ---------------------------------------------------------------------------------- the refusals (csrc/glabc_check.h)
TABLES = ("static const uint32_t PF[6] = {1, 2, 3, 4, 5, 6}; static const uint32_t DUP[6] = {1, 2, 3, 3, 5, 6}; "
          "static const int32_t PR[6] = {0, 1, 1, 0, 0, 1}; static const int32_t SAME[4] = {0, 1, 1, 1}; static uint64_t CNT[4]; "
          "static const double LO[3] = {-1.0, 0.0, 5.0}, HI[3] = {1.0, 1e-300, 6.0}, BAD_NAN[3] = {-1.0, NAN, 5.0}; ")
SHARED = [dict(), dict(stride="82"), dict(n="0", stride="0"), dict(n="2147483648ll", stride="2147483648ll"), dict(scale="1e-300"),
          dict(scale="1.7e308"), dict(d="1"), dict(d="8")]
SHARED_BAD = [(NULL, dict(x="nullptr")), (NULL, dict(w="nullptr")), (NULL, dict(c="nullptr")), (NULL, dict(w="nullptr", d="0")),
              (NULL, dict(w="nullptr", scale="0.0")), (NULL, dict(x="nullptr", n="-1")),          # a null pointer is reported first
              (DIM, dict(d="0")), (DIM, dict(d="9")), (DIM, dict(d="9", n="-1")), (DIM, dict(d="0", scale="NAN")),          # then the dimension
              (ARG, dict(n="-1")), (ARG, dict(n="2147483649ll", stride="2147483649ll")), (ARG, dict(stride="64")),
              (ARG, dict(scale="0.0")), (ARG, dict(scale="-1.0")), (ARG, dict(scale="NAN")), (ARG, dict(scale="INFINITY")), (ARG, dict(scale="-INFINITY"))]


def test_check_weighted_key_counts(tmp_path_factory):
    call = "check_weighted_key_counts(%s, %s, %s, %s, %s, %s, %s, %s, %s, %s)"
    base = dict(x="b.f", stride="65", d="3", w="b.f", n="65", scale="1024.0", level="1", np="2", p="PF", c="CNT")

    def row(want, **kw):
        a = dict(base, **kw)
        return (TABLES, call % (a["x"], a["stride"], a["d"], a["w"], a["n"], a["scale"], a["level"], a["np"], a["p"], a["c"]), want)
    check_table(tmp_path_factory, "weighted_key_counts", [row(OK, **kw) for kw in SHARED if kw.get("d") != "8"] + [row(want, **kw) for want, kw in SHARED_BAD] + [
        row(OK, d="8", level="0", np="1"), row(OK, level="0", np="1"), row(OK, level="2"), row(OK, level="0", np="1", p="DUP"),
        row(NULL, p="nullptr"), row(NULL, p="nullptr", level="7"),
        row(ARG, level="3"), row(ARG, level="-1"), row(ARG, np="0"), row(ARG, np="9"), row(ARG, level="0", np="2"), row(ARG, p="DUP"),
        row(ARG, p="DUP", scale="NAN"),
    ])


def test_check_weighted_histogram(tmp_path_factory):
    call = "check_weighted_histogram(%s, %s, %s, %s, %s, %s, %s, %s, %s, %s)"
    base = dict(x="b.f", stride="65", d="3", w="b.f", n="65", scale="1024.0", bins="64", lo="LO", hi="HI", c="CNT")

    def row(want, **kw):
        a = dict(base, **kw)
        return (TABLES, call % (a["x"], a["stride"], a["d"], a["w"], a["n"], a["scale"], a["bins"], a["lo"], a["hi"], a["c"]), want)
    check_table(tmp_path_factory, "weighted_histogram", [row(OK, **kw) for kw in SHARED if kw.get("d") != "8"] + [row(want, **kw) for want, kw in SHARED_BAD] + [
        row(OK, bins="1"), row(OK, bins="4096"),
        row(NULL, lo="nullptr"), row(NULL, hi="nullptr", bins="0"),
        row(ARG, bins="0"), row(ARG, bins="4097"), row(ARG, lo="HI", hi="LO"), row(ARG, lo="BAD_NAN"), row(ARG, lo="LO", hi="LO"),
    ])


def test_check_weighted_histogram2d(tmp_path_factory):
    call = "check_weighted_histogram2d(%s, %s, %s, %s, %s, %s, %s, %s, %s, %s, %s, %s)"
    base = dict(x="b.f", stride="65", d="3", w="b.f", n="65", scale="1024.0", np="3", p="PR", bins="64", lo="LO", hi="HI", c="CNT")

    def row(want, **kw):
        a = dict(base, **kw)
        return (TABLES, call % (a["x"], a["stride"], a["d"], a["w"], a["n"], a["scale"], a["np"], a["p"], a["bins"], a["lo"], a["hi"], a["c"]), want)
    check_table(tmp_path_factory, "weighted_histogram2d", [row(OK, **kw) for kw in SHARED if kw.get("d") not in ("1", "8")] + [row(want, **kw) for want, kw in SHARED_BAD] + [
        row(OK, bins="1"), row(OK, bins="128"), row(OK, d="2"), row(OK, np="1", p="SAME"),
        row(NULL, p="nullptr"), row(NULL, lo="nullptr"), row(NULL, hi="nullptr", np="0"),
        row(ARG, np="0"), row(ARG, np="29"), row(ARG, np="2", p="SAME"), row(ARG, d="1"), row(ARG, bins="0"), row(ARG, bins="129"),
        row(ARG, lo="BAD_NAN"), row(ARG, lo="HI", hi="LO"),
    ])
