"""Summaries of weighted draws restated in NumPy: the quantised weight of include/glabc.h, the specifications of
glabc_weighted_key_counts, glabc_weighted_histogram and glabc_weighted_histogram2d, and the quantile rule of
glabcmcmc_amd/weighted.py as a sort and an integer cumulative sum.  The key is tests/quantile_ref.py's and the bins are
tests/joint_ref.py's; nothing is shared with csrc/ or with weighted.py.  tests/test_weighted_host.py checks it against
numpy.quantile(weights=, method="inverted_cdf"), numpy.histogram and numpy.histogram2d, tests/test_weighted_shapes.py holds the
kernels and the module to it.

Draws here are dimension-major float32 [d][stride] with one float32 weight per draw; columns n .. are never read.
"""
import math
from fractions import Fraction

import numpy as np

import joint_ref as J
import quantile_ref as Q

CLAMP = (1 << 32) - 1


# ---------------------------------------------------------------------------------- the quantised weight
def multiplicity(w, scale):
    """float32 weights -> uint64: v = (double) w * scale; 0 if not w > 0; 2^32 - 1 if v >= 4294967295; rint(v), ties to even"""
    w = np.asarray(w, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = w.astype(np.float64) * np.float64(scale)
        m = np.where(v >= 4294967295.0, np.float64(CLAMP), np.rint(v))
        m = np.where(w > 0, m, 0.0)
    return m.astype(np.uint64)


def default_scale(w):
    """2^(31 - floor(log2 max w))"""
    top = float(np.max(np.asarray(w, np.float32)))
    return 2.0 ** (31 - math.floor(math.log2(top)))


def _sum(slot, m, n_slots):
    out = np.zeros(n_slots, np.uint64)
    keep = m > 0
    np.add.at(out, slot[keep], m[keep])
    return out


# ---------------------------------------------------------------------------------- glabc_weighted_key_counts
def key_counts(x, w, scale, level, prefixes=None, n=None):
    """-> uint64 [d][P][2^digit_bits]; prefixes: integers [d][P] (None at level 0: P = 1)"""
    d, stride = x.shape
    n = stride if n is None else n
    prefix_bits, digit_bits = Q.LEVELS[level]
    m = multiplicity(np.asarray(w)[:n], scale)
    table = np.zeros((d, 1), np.uint32) if prefixes is None else np.asarray(prefixes).astype(np.uint32)
    out = np.zeros((d, table.shape[1], 1 << digit_bits), np.uint64)
    for j in range(d):
        k = Q.keys(np.asarray(x)[j, :n]).astype(np.uint64)
        digit = ((k >> np.uint64(32 - prefix_bits - digit_bits)) & np.uint64((1 << digit_bits) - 1)).astype(np.int64)
        for s, p in enumerate(table[j]):
            if level > 0 and int(p) == Q.UNUSED:
                continue
            mine = np.ones(n, bool) if level == 0 else k >> np.uint64(32 - prefix_bits) == np.uint64(p)
            out[j, s] = _sum(digit[mine], m[mine], 1 << digit_bits)
    return out


# ---------------------------------------------------------------------------------- glabc_weighted_histogram
def histogram(x, w, scale, n_bins, lo, hi, n=None):
    """-> uint64 [d][n_bins + 3]: the bins, then below, above, NaN"""
    d, stride = x.shape
    n = stride if n is None else n
    m = multiplicity(np.asarray(w)[:n], scale)
    out = np.zeros((d, n_bins + 3), np.uint64)
    for j in range(d):
        v = np.asarray(x)[j, :n]
        slot = J.axis_bins(v, n_bins, lo[j], hi[j])
        with np.errstate(invalid="ignore"):
            below = v.astype(np.float64) < np.float64(lo[j])
        slot = np.where(slot == J.NAN, n_bins + 2, np.where(slot == J.OUTSIDE, np.where(below, n_bins, n_bins + 1), slot))
        out[j] = _sum(slot, m, n_bins + 3)
    return out


# ---------------------------------------------------------------------------------- glabc_weighted_histogram2d
def histogram2d(x, w, scale, pairs, n_bins, lo, hi, n=None):
    """-> uint64 [P][n_bins^2 + 2]: the cells (bin_a * n_bins + bin_b), then outside, then NaN"""
    d, stride = x.shape
    n = stride if n is None else n
    m = multiplicity(np.asarray(w)[:n], scale)
    cells = n_bins * n_bins
    out = np.zeros((len(pairs), cells + 2), np.uint64)
    for p, (a, b) in enumerate(pairs):
        ba = J.axis_bins(np.asarray(x)[a, :n], n_bins, lo[a], hi[a])
        bb = J.axis_bins(np.asarray(x)[b, :n], n_bins, lo[b], hi[b])
        slot = ba * n_bins + bb
        slot[(ba == J.OUTSIDE) | (bb == J.OUTSIDE)] = cells
        slot[(ba == J.NAN) | (bb == J.NAN)] = cells + 1              # a NaN on either axis comes first
        out[p] = _sum(slot, m, cells + 2)
    return out


# ---------------------------------------------------------------------------------- the multiset's order statistics and quantiles
def sorted_multiset(v, m):
    """-> (values float32 ascending by key with -0 as +0 and NaNs last, cumulative multiplicities as Python integers), draws of
    multiplicity 0 left out"""
    keep = np.asarray(m) > 0
    k = Q.keys(np.asarray(v, np.float32)[keep])
    order = np.argsort(k, kind="stable")
    cum, total = [], 0
    for c in np.asarray(m)[keep][order].tolist():
        total += int(c)
        cum.append(total)
    return Q.unkey(k[order]), cum


def order_statistic(v, m, rank):
    values, cum = sorted_multiset(v, m)
    for value, c in zip(values, cum):                                # the first draw whose cumulative multiplicity exceeds the rank
        if c > rank:
            return value
    raise AssertionError("rank %d outside 0 .. %d" % (rank, cum[-1] - 1))


def quantile_rank(q, total):
    """order statistic max(ceil(q M), 1) - 1, the product in exact integer arithmetic"""
    return max(math.ceil(Fraction(float(q)) * int(total)), 1) - 1


def quantile(x, m, q, n=None):
    """-> float64 [Q][d]: the smallest draw whose cumulative multiplicity reaches max(ceil(q M), 1); NaN where a NaN has positive
    multiplicity"""
    d, stride = x.shape
    n = stride if n is None else n
    m = np.asarray(m)[:n]
    total = sum(int(c) for c in m.tolist())
    out = np.empty((len(q), d))
    for j in range(d):
        v = np.asarray(x)[j, :n]
        has_nan = bool((np.isnan(v) & (m > 0)).any())
        out[:, j] = [np.nan if has_nan else np.float64(order_statistic(v, m, quantile_rank(qq, total))) for qq in q]
    return out
