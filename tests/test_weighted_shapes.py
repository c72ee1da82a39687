"""glabc_weighted_key_counts, glabc_weighted_histogram and glabc_weighted_histogram2d (csrc/glabc_weighted.hip) at every shape at
which the kernels take another path, equal counts against the NumPy restatement of their specification (tests/weighted_ref.py)
and against their unweighted twins, and the functions of glabcmcmc_amd/weighted.py on device tensors against their generic path.

The kernels cut the draws into items of 64 x 4 consecutive draws that the 8 wavefronts of a workgroup take round-robin, and load
every 64-draw segment, the weights' included, through a descriptor of exactly its bytes.  So the grid has draws on both sides of a
segment (64), of an item (256) and of a workgroup's first round (2048), none at all, a stride that is no multiple of 4 (pad 17),
padding columns that hold NaN (a read of one with a weight changes the NaN counter) and base pointers 1, 2 and 3 floats into wider
buffers, the draws' and the weights' independently.  The floats around the weights hold 7.0, not NaN: a NaN weight counts nothing,
so a stray read of one would show nowhere.  cases() is not the full cross product: test_grid_covers_every_pair checks that every
value of an axis meets at least two values of every other axis.

Tolerances: none.  Counts are equal integers, order statistics and quantiles equal values (NaN matching NaN).
"""
import functools

import numpy as np
import pytest
import torch

import joint_ref as J
import quantile_ref as Q
import weighted_ref as W
from helpers import dev
from test_quantile_shapes import ABSENT, after, prefilled, prefix_table

ERR_NULL, ERR_DIM, ERR_ARG = -1, -2, -4          # glabc_status, include/glabc.h

SEGMENTS = 4                                      # WEIGHTED_SEGMENTS of csrc/glabc_weighted.hip
ITEM, ROUND = 64 * SEGMENTS, 8 * 64 * SEGMENTS
DIMS = (1, 2, 3, 8)
DRAWS = (0, 1, 3, 63, 64, 65, ITEM - 1, ITEM + 1, ROUND - 1, ROUND + 1)
PADS = (0, 17)
OFFSETS = (0, 1, 2, 3)                            # floats between a device buffer's base and the draws' / the weights'
N_PREFIXES = (1, 2, 3, 5, 8)                     # 3 and 5: the kernels are compiled for 1, 2, 4 and 8 compared prefixes
SCALE = 1024.0                                    # a power of two: weights of (k + 0.5) / 1024 are ties
CLAMP = (1 << 32) - 1


@functools.lru_cache(maxsize=None)
def cases():
    """(dim, n, pad, draws' offset, weights' offset): every n at every dim"""
    out = []
    for di, d in enumerate(DIMS):
        for ni, n in enumerate(DRAWS):
            out.append((d, n, PADS[(di + ni) % 2], OFFSETS[(di + ni // 2) % 4], OFFSETS[(2 * di + ni + ni // 4) % 4]))
    return tuple(out)


def test_grid_covers_every_pair():
    axes = (DIMS, DRAWS, PADS, OFFSETS, OFFSETS)
    rows = cases()
    for a in range(5):
        assert {c[a] for c in rows} == set(axes[a])
        for b in range(5):
            if a != b:
                for v in axes[a]:
                    met = {c[b] for c in rows if c[a] == v}
                    assert len(met) >= 2, (a, v, b, met)
    assert any(c[3] != c[4] for c in rows) and any(c[3] == c[4] for c in rows)          # the two offsets are independent


@functools.lru_cache(maxsize=None)
def draws(d, n):
    """(x float32 [d][n], w float32 [n]): normal values with ties, the special values of tests/quantile_ref.py and NaNs; weights that
    mix zeros and negatives (some on NaN draws), ties of the rounding, the clamp, tiny and ordinary values.  Some NaN draws keep a
    weight: they must reach the NaN slots, the others must not"""
    rng = np.random.default_rng(1000 * d + n)
    x = (rng.standard_normal((d, n)) * 3.0).astype(np.float32)
    x[:, ::3] = np.round(x[:, ::3])
    special = Q.special_values()
    for j in range(d):
        at = (np.arange(special.size) * 13 + 5 * j) % max(n, 1)
        x[j, at[:n // 2]] = special[:n // 2][:at[:n // 2].size]
    w = (rng.random(n) * 4.0).astype(np.float32)
    w[::5] = ((rng.integers(0, 40, size=w[::5].size) + 0.5) / SCALE).astype(np.float32)          # ties: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2
    w[1::7] = 0.0
    w[3::11] = -1.5
    w[4::13] = np.float32(1.0e7)                                                                   # 1e7 x 1024 clamps at 2^32 - 1
    w[6::17] = np.float32(1.0e-6)                                                                  # rounds to 0
    if n > 20:
        x[0, 1], x[d - 1, 8], x[0, 3] = np.nan, np.nan, np.nan                                   # weights 0, 0 and -1.5
        x[d - 1, 2], x[0, 4] = np.nan, np.nan                                                    # an ordinary weight and the clamp
    x.setflags(write=False)
    w.setflags(write=False)
    return x, w


def placed(x, w, pad, x_off, w_off):
    """-> (buffers, pointer to the draws, stride, pointer to the weights): the draws `x_off` floats into a buffer of NaN with `pad`
    columns of NaN behind every coordinate, the weights `w_off` floats into a buffer of 7.0"""
    d, n = x.shape
    body = np.full((d, n + pad), np.nan, np.float32)
    body[:, :n] = x
    flat = np.full(x_off + body.size + 5, np.nan, np.float32)
    flat[x_off:x_off + body.size] = body.reshape(-1)
    wflat = np.full(w_off + n + 5, 7.0, np.float32)
    wflat[w_off:w_off + n] = w
    tx, tw = dev(flat), dev(wflat)
    return (tx, tw), tx.data_ptr() + 4 * x_off, n + pad, tw.data_ptr() + 4 * w_off


def table_for(x, level, n_prefixes):
    d, n = x.shape
    if level == 0:
        return np.zeros((d, 1), np.uint32)
    if n == 0:
        return np.tile(np.arange(1, n_prefixes + 1, dtype=np.uint32), (d, 1))
    return prefix_table(x[None], level, n_prefixes)


def hip_key_counts(hip, x, w, pad, x_off, w_off, scale, level, table, expect=0):
    d, n = x.shape
    keep, xp, stride, wp = placed(x, w, pad, x_off, w_off)
    p = table.shape[1]
    size = d * p << Q.LEVELS[level][1]
    t, cp, before = prefilled(size)
    table = np.ascontiguousarray(table, np.uint32)
    assert hip.glabc_weighted_key_counts(xp, stride, d, wp, n, scale, level, p, table.ctypes.data, cp, None) == expect
    return (after(t, size) - before).reshape(d, p, -1)


def hip_histogram(hip, x, w, pad, x_off, w_off, scale, bins, lo, hi):
    d, n = x.shape
    keep, xp, stride, wp = placed(x, w, pad, x_off, w_off)
    t, cp, before = prefilled(d * (bins + 3))
    lo, hi = np.ascontiguousarray(lo, np.float64), np.ascontiguousarray(hi, np.float64)
    assert hip.glabc_weighted_histogram(xp, stride, d, wp, n, scale, bins, lo.ctypes.data, hi.ctypes.data, cp, None) == 0
    return (after(t, d * (bins + 3)) - before).reshape(d, bins + 3)


def hip_histogram2d(hip, x, w, pad, x_off, w_off, scale, pairs, bins, lo, hi):
    d, n = x.shape
    keep, xp, stride, wp = placed(x, w, pad, x_off, w_off)
    size = len(pairs) * (bins * bins + 2)
    t, cp, before = prefilled(size)
    lo, hi = np.ascontiguousarray(lo, np.float64), np.ascontiguousarray(hi, np.float64)
    table = np.ascontiguousarray(pairs, np.int32)
    assert hip.glabc_weighted_histogram2d(xp, stride, d, wp, n, scale, len(pairs), table.ctypes.data, bins, lo.ctypes.data, hi.ctypes.data,
                                          cp, None) == 0
    return (after(t, size) - before).reshape(len(pairs), -1)


LO = np.array([-3.0, 0.0, -7.5, -3.0, 1.0, -0.1, -2.0, -50.0])
HI = np.array([3.0, 6.0, 0.7, 3.5, 1.5, 0.2, 5.0, 50.0])


# ---------------------------------------------------------------------------------- GPU: glabc_weighted_key_counts
@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_key_counts_match_the_restatement(hip, d):
    n_cases = 0
    for ci, (_, n, pad, x_off, w_off) in enumerate(c for c in cases() if c[0] == d):
        x, w = draws(d, n)
        for level in (0, 1, 2):
            p = 1 if level == 0 else N_PREFIXES[(ci + level) % len(N_PREFIXES)]
            table = table_for(x, level, p)
            want = W.key_counts(x, w, SCALE, level, None if level == 0 else table)
            added = hip_key_counts(hip, x, w, pad, x_off, w_off, SCALE, level, table)
            where = (d, n, pad, x_off, w_off, level, table.tolist())
            assert np.array_equal(added, want), where
            if level == 0:
                m = W.multiplicity(w, SCALE)
                assert (added.sum(axis=(1, 2)) == m.sum()).all(), where
                for j in range(d):                                    # the NaN draws that carry weight, and no others
                    assert added[j, 0, -1] == m[np.isnan(x[j])].sum(), where
                if n > 20:
                    assert np.isnan(x[0, [1, 3, 4]]).all() and m[[1, 3]].tolist() == [0, 0] and m[4] == CLAMP and added[0, 0, -1] >= CLAMP, where
            else:
                for j in range(d):
                    for s in range(p):
                        if n and table[j, s] in (Q.UNUSED, ABSENT[level]):
                            assert not added[j, s].any(), where
            n_cases += 1
    assert n_cases == len(DRAWS) * 3


@pytest.mark.gpu
def test_every_prefix_count_meets_every_level(hip):
    """1, 2, 3, 5 and 8 prefixes at levels 1 and 2 on one ragged, padded, misaligned shape: the largest table is 8 x 2^11 64-bit
    counters, a CU's LDS to one workgroup"""
    x, w = draws(3, ROUND + 1)
    for level in (1, 2):
        for p in N_PREFIXES:
            table = table_for(x, level, p)
            added = hip_key_counts(hip, x, w, 17, 3, 1, SCALE, level, table)
            assert np.array_equal(added, W.key_counts(x, w, SCALE, level, table)), (level, p)
            assert added.any()


# ---------------------------------------------------------------------------------- GPU: the histograms
HIST_BINS = (1, 2, 64, 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("bins", HIST_BINS)
def test_histogram_matches_the_restatement(hip, bins):
    for d, n, pad, x_off, w_off in cases()[HIST_BINS.index(bins) % 3::3]:
        x, w = draws(d, n)
        x = np.array(x)
        if n > 40:                                                    # values on lo, on hi, next to them and on an interior edge
            plant = [LO[0], HI[0], np.nextafter(np.float32(LO[0]), np.float32(-np.inf)), np.nextafter(np.float32(HI[0]), np.float32(np.inf)),
                     np.nextafter(np.float32(HI[0]), np.float32(0)), np.float32(LO[0] + (HI[0] - LO[0]) / bins * (bins // 2))]
            x[0, 20:20 + len(plant)] = np.array(plant, np.float32)
        added = hip_histogram(hip, x, w, pad, x_off, w_off, SCALE, bins, LO[:d], HI[:d])
        want = W.histogram(x, w, SCALE, bins, LO[:d], HI[:d])
        assert np.array_equal(added, want), (bins, d, n, pad, x_off, w_off, np.argwhere(added != want)[:4])
        assert (added.sum(axis=1) == W.multiplicity(w, SCALE).sum()).all()


PAIR_SETS = {1: [(1, 0)], 3: [(0, 1), (1, 0), (0, 1)],          # a transposed and a repeated pair
             28: [(i, j) for i in range(8) for j in range(i + 1, 8)]}


@pytest.mark.gpu
@pytest.mark.parametrize("bins", (1, 7, 128))
def test_histogram2d_matches_the_restatement(hip, bins):
    n_cases = 0
    for d, n, pad, x_off, w_off in cases():
        for n_pairs, pairs in PAIR_SETS.items():
            if d == 1 or (n_pairs == 28) != (d == 8) or (bins == 128 and n_pairs == 28 and n not in (65, ROUND + 1)):
                continue
            x, w = draws(d, n)
            added = hip_histogram2d(hip, x, w, pad, x_off, w_off, SCALE, pairs, bins, LO[:d], HI[:d])
            want = W.histogram2d(x, w, SCALE, pairs, bins, LO[:d], HI[:d])
            assert np.array_equal(added, want), (bins, d, n, pad, x_off, w_off, n_pairs)
            assert (added.sum(axis=1) == W.multiplicity(w, SCALE).sum()).all()
            if n_pairs == 3:
                cells = added[:, :bins * bins].reshape(3, bins, bins)
                assert np.array_equal(cells[0], cells[1].T) and np.array_equal(cells[0], cells[2])
            n_cases += 1
    assert n_cases >= 40


# ---------------------------------------------------------------------------------- GPU: the unweighted twins
@pytest.mark.gpu
def test_unit_weights_give_the_twins_counts(hip):
    """every weight 1.0 and scale 1: the three entry points against glabc_key_counts / glabc_histogram / glabc_histogram2d on the same
    buffer as a one-row history"""
    for d, n, pad, x_off, w_off in cases()[1::4]:
        x, _ = draws(d, n)
        ones = np.ones(n, np.float32)
        keep, xp, stride, wp = placed(x, ones, pad, x_off, w_off)
        for level in (0, 1, 2):
            table = np.ascontiguousarray(table_for(x, level, 1 if level == 0 else 3), np.uint32)
            p = table.shape[1]
            size = d * p << Q.LEVELS[level][1]
            t1, c1, b1 = prefilled(size)
            t2, c2, b2 = prefilled(size)
            assert hip.glabc_weighted_key_counts(xp, stride, d, wp, n, 1.0, level, p, table.ctypes.data, c1, None) == 0
            assert hip.glabc_key_counts(xp, 1, d, n, stride, level, p, table.ctypes.data, c2, None) == 0
            assert np.array_equal(after(t1, size) - b1, after(t2, size) - b2), (d, n, level)
        lo, hi = np.ascontiguousarray(LO[:d]), np.ascontiguousarray(HI[:d])
        size = d * 67
        t1, c1, b1 = prefilled(size)
        t2, c2, b2 = prefilled(size)
        assert hip.glabc_weighted_histogram(xp, stride, d, wp, n, 1.0, 64, lo.ctypes.data, hi.ctypes.data, c1, None) == 0
        assert hip.glabc_histogram(xp, 1, d, n, stride, 64, lo.ctypes.data, hi.ctypes.data, c2, None) == 0
        got = after(t1, size) - b1
        assert np.array_equal(got, after(t2, size) - b2) and int(got.sum()) == d * n
        if d > 1:
            pairs = np.array([(0, 1), (d - 1, 0)], np.int32)
            size = 2 * (49 + 2)
            t1, c1, b1 = prefilled(size)
            t2, c2, b2 = prefilled(size)
            assert hip.glabc_weighted_histogram2d(xp, stride, d, wp, n, 1.0, 2, pairs.ctypes.data, 7, lo.ctypes.data, hi.ctypes.data, c1, None) == 0
            assert hip.glabc_histogram2d(xp, 1, d, n, stride, 2, pairs.ctypes.data, 7, lo.ctypes.data, hi.ctypes.data, c2, None) == 0
            assert np.array_equal(after(t1, size) - b1, after(t2, size) - b2)


# ---------------------------------------------------------------------------------- GPU: 64-bit counters
@pytest.mark.gpu
def test_counters_are_64_bits_wide(hip):
    """two draws of multiplicity 2^31 and 321 draws of 2^32 - 1 in one slot: exact sums, which a uint32 counter in LDS wraps"""
    for n, weight, scale, m in ((2, 1.0, 2.0 ** 31, 2 ** 31), (321, 1.0e10, 1.0, CLAMP)):
        x = np.full((2, n), np.float32(1.0))
        w = np.full(n, np.float32(weight))
        assert W.multiplicity(w, scale).tolist() == [m] * n
        key = int(Q.keys(np.array([1.0], np.float32))[0])
        for level, (prefix_bits, digit_bits) in enumerate(Q.LEVELS):
            table = np.full((2, 1), key >> (32 - prefix_bits) if level else 0, np.uint32)
            added = hip_key_counts(hip, x, w, 17, 1, 3, scale, level, table)
            digit = (key >> (32 - prefix_bits - digit_bits)) & ((1 << digit_bits) - 1)
            assert (added[:, 0, digit] == n * m).all() and int(added.sum()) == 2 * n * m
        added = hip_histogram(hip, x, w, 0, 2, 1, scale, 4, [0.0, 0.0], [2.0, 2.0])
        assert added.tolist() == [[0, 0, n * m, 0, 0, 0, 0]] * 2
        added = hip_histogram2d(hip, x, w, 17, 3, 0, scale, [(0, 1)], 4, [0.0, 0.0], [2.0, 2.0])
        assert added[0, 2 * 4 + 2] == n * m and int(added.sum()) == n * m


# ---------------------------------------------------------------------------------- GPU: additivity over slices of draws
@pytest.mark.gpu
@pytest.mark.parametrize("k", (63, 65, ITEM + 1))
def test_counts_add_over_slices_of_draws(hip, k):
    """[0, k) and [k, n) accumulated into one table, the second call from base pointers inside the first's arrays"""
    d, n = 3, ROUND + 1
    x, w = draws(d, n)
    keep, xp, stride, wp = placed(x, w, 17, 1, 2)
    zero = np.zeros((d, 1), np.uint32)
    t, cp, before = prefilled(d * 2048)
    for first, count in ((0, k), (k, n - k)):
        assert hip.glabc_weighted_key_counts(xp + 4 * first, stride, d, wp + 4 * first, count, SCALE, 0, 1, zero.ctypes.data, cp, None) == 0
    assert np.array_equal((after(t, d * 2048) - before).reshape(d, 1, 2048), W.key_counts(x, w, SCALE, 0))
    lo, hi = np.ascontiguousarray(LO[:d]), np.ascontiguousarray(HI[:d])
    t, cp, before = prefilled(d * 67)
    for first, count in ((0, k), (k, n - k)):
        assert hip.glabc_weighted_histogram(xp + 4 * first, stride, d, wp + 4 * first, count, SCALE, 64, lo.ctypes.data, hi.ctypes.data, cp, None) == 0
    assert np.array_equal((after(t, d * 67) - before).reshape(d, 67), W.histogram(x, w, SCALE, 64, lo, hi))
    pairs = np.array([(0, 2), (2, 1)], np.int32)
    t, cp, before = prefilled(2 * 51)
    for first, count in ((0, k), (k, n - k)):
        assert hip.glabc_weighted_histogram2d(xp + 4 * first, stride, d, wp + 4 * first, count, SCALE, 2, pairs.ctypes.data, 7, lo.ctypes.data,
                                              hi.ctypes.data, cp, None) == 0
    assert np.array_equal((after(t, 2 * 51) - before).reshape(2, 51), W.histogram2d(x, w, SCALE, pairs.tolist(), 7, lo, hi))


# ---------------------------------------------------------------------------------- GPU: refusals
@pytest.mark.gpu
def test_refused_calls_write_nothing(hip):
    d, n = 3, 70
    x, w = draws(d, n)
    keep, xp, stride, wp = placed(x, w, 0, 0, 0)
    ok = np.array([[1, 2], [3, 4], [5, 6]], np.uint32)
    dup = np.array([[1, 2], [3, 3], [5, 6]], np.uint32)
    size = d * 2 * 2048
    t, cp, before = prefilled(size)
    nan, inf, big = float("nan"), float("inf"), 2 ** 31 + 1
    for rc, a in ((ERR_NULL, (None, n, d, wp, n, 2.0, 1, 2, ok.ctypes.data, cp)), (ERR_NULL, (xp, n, d, None, n, 2.0, 1, 2, ok.ctypes.data, cp)),
                  (ERR_NULL, (xp, n, d, wp, n, 2.0, 1, 2, None, cp)), (ERR_NULL, (xp, n, d, wp, n, 2.0, 1, 2, ok.ctypes.data, None)),
                  (ERR_NULL, (xp, n, 0, None, n, nan, 1, 2, ok.ctypes.data, cp)), (ERR_DIM, (xp, n, 0, wp, n, 2.0, 1, 2, ok.ctypes.data, cp)),
                  (ERR_DIM, (xp, n, 9, wp, -1, 0.0, 1, 2, ok.ctypes.data, cp)), (ERR_ARG, (xp, n, d, wp, -1, 2.0, 1, 2, ok.ctypes.data, cp)),
                  (ERR_ARG, (xp, big, d, wp, big, 2.0, 1, 2, ok.ctypes.data, cp)), (ERR_ARG, (xp, n - 1, d, wp, n, 2.0, 1, 2, ok.ctypes.data, cp)),
                  (ERR_ARG, (xp, n, d, wp, n, 0.0, 1, 2, ok.ctypes.data, cp)), (ERR_ARG, (xp, n, d, wp, n, -2.0, 1, 2, ok.ctypes.data, cp)),
                  (ERR_ARG, (xp, n, d, wp, n, nan, 1, 2, ok.ctypes.data, cp)), (ERR_ARG, (xp, n, d, wp, n, inf, 1, 2, ok.ctypes.data, cp)),
                  (ERR_ARG, (xp, n, d, wp, n, 2.0, 3, 2, ok.ctypes.data, cp)), (ERR_ARG, (xp, n, d, wp, n, 2.0, 1, 9, ok.ctypes.data, cp)),
                  (ERR_ARG, (xp, n, d, wp, n, 2.0, 0, 2, ok.ctypes.data, cp)), (ERR_ARG, (xp, n, d, wp, n, 2.0, 1, 2, dup.ctypes.data, cp)),
                  (0, (xp, n, d, wp, 0, 2.0, 1, 2, ok.ctypes.data, cp)), (0, (xp, 0, d, wp, 0, 2.0, 0, 1, ok.ctypes.data, cp))):
        assert hip.glabc_weighted_key_counts(*a, None) == rc, a
        assert np.array_equal(after(t, size), before), a
    lo, hi, bad = np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 1.0]), np.array([0.0, np.nan, 0.0])
    for rc, a in ((ERR_NULL, (xp, n, d, None, n, 2.0, 8, lo.ctypes.data, hi.ctypes.data, cp)), (ERR_NULL, (xp, n, d, wp, n, 2.0, 8, None, hi.ctypes.data, cp)),
                  (ERR_DIM, (xp, n, 9, wp, n, 2.0, 0, lo.ctypes.data, hi.ctypes.data, cp)), (ERR_ARG, (xp, n - 1, d, wp, n, 2.0, 8, lo.ctypes.data, hi.ctypes.data, cp)),
                  (ERR_ARG, (xp, big, d, wp, big, 2.0, 8, lo.ctypes.data, hi.ctypes.data, cp)), (ERR_ARG, (xp, n, d, wp, n, nan, 8, lo.ctypes.data, hi.ctypes.data, cp)),
                  (ERR_ARG, (xp, n, d, wp, n, 0.0, 8, lo.ctypes.data, hi.ctypes.data, cp)), (ERR_ARG, (xp, n, d, wp, n, 2.0, 4097, lo.ctypes.data, hi.ctypes.data, cp)),
                  (ERR_ARG, (xp, n, d, wp, n, 2.0, 8, hi.ctypes.data, lo.ctypes.data, cp)), (ERR_ARG, (xp, n, d, wp, n, 2.0, 8, bad.ctypes.data, hi.ctypes.data, cp)),
                  (0, (xp, n, d, wp, 0, 2.0, 8, lo.ctypes.data, hi.ctypes.data, cp))):
        assert hip.glabc_weighted_histogram(*a, None) == rc, a
        assert np.array_equal(after(t, size), before), a
    pairs, same = np.array([(0, 1), (2, 0)], np.int32), np.array([(0, 1), (1, 1)], np.int32)
    for rc, a in ((ERR_NULL, (xp, n, d, None, n, 2.0, 2, pairs.ctypes.data, 8, lo.ctypes.data, hi.ctypes.data, cp)),
                  (ERR_NULL, (xp, n, d, wp, n, 2.0, 2, None, 8, lo.ctypes.data, hi.ctypes.data, cp)),
                  (ERR_DIM, (xp, n, 0, wp, n, 2.0, 2, pairs.ctypes.data, 8, lo.ctypes.data, hi.ctypes.data, cp)),
                  (ERR_ARG, (xp, n, d, wp, -1, 2.0, 2, pairs.ctypes.data, 8, lo.ctypes.data, hi.ctypes.data, cp)),
                  (ERR_ARG, (xp, big, d, wp, big, 2.0, 2, pairs.ctypes.data, 8, lo.ctypes.data, hi.ctypes.data, cp)),
                  (ERR_ARG, (xp, n, d, wp, n, inf, 2, pairs.ctypes.data, 8, lo.ctypes.data, hi.ctypes.data, cp)),
                  (ERR_ARG, (xp, n, d, wp, n, -1.0, 2, pairs.ctypes.data, 8, lo.ctypes.data, hi.ctypes.data, cp)),
                  (ERR_ARG, (xp, n, d, wp, n, 2.0, 29, pairs.ctypes.data, 8, lo.ctypes.data, hi.ctypes.data, cp)),
                  (ERR_ARG, (xp, n, d, wp, n, 2.0, 2, same.ctypes.data, 8, lo.ctypes.data, hi.ctypes.data, cp)),
                  (ERR_ARG, (xp, n, d, wp, n, 2.0, 2, pairs.ctypes.data, 129, lo.ctypes.data, hi.ctypes.data, cp)),
                  (ERR_ARG, (xp, n, d, wp, n, 2.0, 2, pairs.ctypes.data, 8, bad.ctypes.data, hi.ctypes.data, cp)),
                  (0, (xp, n, d, wp, 0, 2.0, 2, pairs.ctypes.data, 8, lo.ctypes.data, hi.ctypes.data, cp))):
        assert hip.glabc_weighted_histogram2d(*a, None) == rc, a
        assert np.array_equal(after(t, size), before), a


# ---------------------------------------------------------------------------------- GPU: weighted.py end to end
def same_values(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.gpu
def test_public_functions_equal_the_generic_path(hip):
    from glabcmcmc_amd import diagnostics as D
    from glabcmcmc_amd import weighted
    d, n = 3, ROUND + 1
    x, w = draws(d, n)
    x = np.where(np.isinf(x), np.float32(9.0), x)                                    # a finite range for range=None
    w = np.where((w > 0) & (w < 1.0e6), w, np.float32(0.0))                          # what quantize accepts: no negative, no clamp
    x[1:] = np.where(np.isnan(x[1:]), np.float32(1.25), x[1:])                       # coordinate 0 keeps NaNs that carry weight;
    x[0, 2], x[1, 1], x[2, 8] = np.nan, np.nan, np.nan                               # in the others only draws of weight 0 are NaN
    assert w[2] > 0 and w[1] == 0 and w[8] == 0
    qs = (0.0, 0.025, 0.25, 0.5, 0.77, 0.975, 1.0)
    host_rows, host_w = torch.from_numpy(np.ascontiguousarray(x.T)), torch.from_numpy(w)
    storage = dev(x)                                                                 # dimension-major, as rejection.sample returns it
    for theta in (storage.t(), dev(np.ascontiguousarray(x.T)), dev(np.ascontiguousarray(x.T)).double()):
        on_gpu, on_cpu = (theta, dev(w)), (host_rows, host_w)
        if theta.dtype == torch.float32 and theta.stride(0) == 1:
            assert weighted._Prepared(on_gpu, None, "auto").x.data_ptr() == storage.data_ptr()          # read in place
        for scale in (None, 4096.0):
            sc = W.default_scale(w) if scale is None else scale
            m = W.multiplicity(w, sc)
            total = int(m.sum())
            got = weighted.quantile(on_gpu, qs, scale=scale)
            assert same_values(got, weighted.quantile(on_cpu, qs, scale=scale)) and same_values(got, weighted.quantile(on_gpu, qs, scale=scale, path="generic"))
            assert same_values(got, W.quantile(x, m, qs)) and not np.isnan(got[:, 1:]).any() and np.isnan(got[:, 0]).all()
            lower, upper = weighted.interval(on_gpu, 0.9, scale=scale)
            want = weighted.interval(on_cpu, 0.9, scale=scale)
            assert same_values(lower, want[0]) and same_values(upper, want[1])
            ranks = [0, 1, total // 3, total // 2, total - 1] + [(i * (total - 1)) // 8 for i in range(9)]          # more than 8 prefixes
            got = weighted.order_statistics(on_gpu, ranks, scale=scale)
            assert got.dtype == np.float32 and same_values(got, weighted.order_statistics(on_cpu, ranks, scale=scale))
            assert same_values(got[:3, 1], [W.order_statistic(x[1], m, r) for r in ranks[:3]])
            for level in (0, 1):
                table = None if level == 0 else table_for(x, 1, 9)                   # two launches
                assert np.array_equal(weighted.key_counts(on_gpu, level, table, scale=scale), W.key_counts(x, w, sc, level, table))
            for rng in (None, np.stack([LO[:d], HI[:d]], axis=1)):
                h, g = weighted.histogram(on_gpu, 65, rng, scale=scale), weighted.histogram(on_cpu, 65, rng, scale=scale)
                for a, b in zip(h, g):
                    assert np.array_equal(a, b)
                assert (h.counts.sum(axis=1) + h.below + h.above + h.nan == total).all() and h.nan[0] > 0 and not h.nan[1:].any()
                j2, g2 = weighted.histogram2d(on_gpu, None, 33, rng, scale=scale), weighted.histogram2d(on_cpu, None, 33, rng, scale=scale)
                for a, b in zip(j2, g2):
                    assert np.array_equal(a, b)
                want = W.histogram2d(x, w, sc, [(0, 1), (0, 2), (1, 2)], 33, j2.edges[:, 0], j2.edges[:, -1])
                assert np.array_equal(j2.counts.reshape(3, -1), want[:, :33 * 33]) and np.array_equal(j2.nan, want[:, -1]) and j2.nan[0] > 0 and j2.nan[2] == 0
                level, mass, inside = D.hpd_levels(j2.counts, (0.5, 0.9, 0.95))
                again = D.hpd_levels(want[:, :33 * 33].reshape(3, 33, 33), (0.5, 0.9, 0.95))
                assert all(np.array_equal(a, b) for a, b in zip((level, mass, inside), again))
                need, v, ms, cnt = J.hpd_level(want[2, :33 * 33], 0.9)
                assert (int(level[2, 1]), int(mass[2, 1]), int(inside[2, 1])) == (v, ms, cnt)
            s, c = weighted.summary(on_gpu, scale=scale), weighted.summary(on_cpu, scale=scale)
            assert s["M"] == c["M"] == total and s["ess"] == c["ess"] and s["scale"] == sc and same_values(s["quantiles"], c["quantiles"])
            assert np.isnan(s["mean"][0]) and np.allclose(s["mean"][1:], c["mean"][1:], rtol=1e-12, atol=1e-14)
    with pytest.raises(ValueError):
        weighted.quantile(on_cpu, 0.5, path="fused")
