"""glabc_key_counts and glabc_histogram (csrc/glabc_quant.hip) at every shape at which the counting kernel takes another path,
equal counts against the NumPy restatement of their specification (tests/quantile_ref.py), and the quantile functions of
glabcmcmc_amd/diagnostics.py against numpy.sort and the restatement.

The kernel cuts a coordinate into items of 64 chains x 16 rows that the 8 wavefronts of its workgroups take round-robin, and
loads every row segment through a descriptor of exactly its bytes.  So the grid has chains on both sides of 64 and of the
4-float alignment of a wide load, one row, rows on both sides of 16 and of 8 x 16, a stride that is no multiple of 4 (pad 17),
padding columns that hold NaN (a read of one changes the NaN counter) and a base pointer 1, 2 and 3 floats into a wider buffer,
as the slab addressing of a caller would give it.  cases() is not the full cross product: test_grid_covers_every_pair checks
that every value of an axis meets at least two values of every other axis.

Tolerances: none for counts and order statistics (equal integers; equal float32 values, NaN matching NaN).  quantile against
the restatement's formula: equal float64.  quantile against numpy.quantile: 4 ulps of max(|x_lo|, |x_hi|) -- NumPy's lerp rounds
one product and one sum, possibly from the other end, so 2 ulps is the bound and 4 leaves a factor of two.
"""
import functools

import numpy as np
import pytest
import torch

import diag_ref as R
import quantile_ref as Q
from helpers import dev, host

ERR_NULL, ERR_DIM, ERR_ARG = -1, -2, -4          # glabc_status, include/glabc.h

DIMS = (1, 2, 3, 8)
CHAINS = (1, 3, 4, 5, 63, 64, 65, 321)
PADS = (0, 17)
OFFSETS = (0, 1, 2, 3)                            # floats between the device buffer's base and the history's
ROWS = (1, 2, 33, 97)
N_PREFIXES = (1, 2, 3, 5, 8)                     # 3 and 5: the kernels are compiled for 1, 2, 4 and 8 compared prefixes
GUARD = 7                                         # canary elements on either side of the counts
CANARY = np.uint64(0xDEADC0DEDEADBEEF)
ABSENT = {1: 0x7F3, 2: 0x3F9ABC}                  # prefixes no test value has: keys 0xFE6..., a float of about 1.6e38


@functools.lru_cache(maxsize=None)
def cases():
    """(theta_dim, n_chains, pad, offset, n_rows): two chain counts per (theta_dim, n_rows)"""
    out = []
    for di, d in enumerate(DIMS):
        for ri, n_rows in enumerate(ROWS):
            for s in (0, 1):
                ci = (2 * di + ri + 4 * s) % len(CHAINS)
                out.append((d, CHAINS[ci], PADS[(di + ci // 2 + s) % 2], OFFSETS[(di + ri + ci // 2 + s) % 4], n_rows))
    return tuple(out)


def test_grid_covers_every_pair():
    axes = (DIMS, CHAINS, PADS, OFFSETS, ROWS)
    rows = cases()
    for a in range(5):
        assert {c[a] for c in rows} == set(axes[a])
        for b in range(5):
            if a != b:
                for v in axes[a]:
                    met = {c[b] for c in rows if c[a] == v}
                    assert len(met) >= 2, (a, v, b, met)


INPUTS = ("diag", "special", "constant")


@functools.lru_cache(maxsize=None)
def history(kind, n_rows, d, n):
    if kind == "diag":
        return R.diag_history(n_rows, d, n)
    h = Q.special_history(n_rows, d, n) if kind == "special" else np.full((n_rows, d, n), np.float32(-1.75))
    h.setflags(write=False)
    return h


def placed(hist, pad, offset):
    """-> (device buffer, pointer to the history, stride): the history `offset` floats into a buffer of NaN, `pad` columns of NaN
    behind every row segment"""
    n_rows, d, n = hist.shape
    body = R.padded(hist, pad) if pad else np.asarray(hist)
    flat = np.full(offset + body.size + 5, np.nan, np.float32)
    flat[offset:offset + body.size] = body.reshape(-1)
    t = dev(flat)
    return t, t.data_ptr() + 4 * offset, n + pad


def prefilled(size):
    """counts that already hold something, between guard bands -> (device tensor, pointer to the counts, what they hold)"""
    before = (np.arange(size, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1000)) + np.uint64(1)
    buf = np.concatenate([np.full(GUARD, CANARY), before, np.full(GUARD, CANARY)])
    t = dev(buf.view(np.int64))
    return t, t.data_ptr() + 8 * GUARD, before


def after(t, size):
    a = host(t).view(np.uint64)
    assert (a[:GUARD] == CANARY).all() and (a[GUARD + size:] == CANARY).all(), "the counts' guard bands were written"
    return a[GUARD:GUARD + size]


def prefix_table(hist, level, n_prefixes):
    """uint32 [d][n_prefixes]: prefixes the restatement's own selection walks on this input, one slot with a prefix that no value
    has and one unused slot where there is room, at places that differ per coordinate"""
    n_rows, d, n = hist.shape
    total = n_rows * n
    walked = Q.selection_prefixes(hist, level, sorted({0, total // 5, total // 2, (4 * total) // 5, total - 1}))
    table = np.full((d, n_prefixes), Q.UNUSED, np.uint32)
    for j in range(d):
        slots = list(walked[j][:max(1, n_prefixes - 2)])
        if n_prefixes > 2 or (n_prefixes == 2 and j % 2 == 0):          # two slots: the absent prefix or the unused slot, by turns
            slots.insert((j + 1) % (len(slots) + 1), ABSENT[level])
        while len(slots) < n_prefixes:
            slots.insert(j % (len(slots) + 1), Q.UNUSED)
        table[j] = slots[:n_prefixes]
    return table


def hip_key_counts(hip, hist, pad, offset, level, table, n=None, expect=0):
    n_rows, d, chains = hist.shape
    buf, ptr, stride = placed(hist, pad, offset)
    p = table.shape[1]
    size = d * p << Q.LEVELS[level][1]
    t, cp, before = prefilled(size)
    table = np.ascontiguousarray(table, np.uint32)
    assert hip.glabc_key_counts(ptr, n_rows, d, chains if n is None else n, stride, level, p, table.ctypes.data, cp, None) == expect
    got = after(t, size)
    return (got - before).reshape(d, p, -1), got, before


# ---------------------------------------------------------------------------------- GPU: glabc_key_counts
@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_key_counts_match_the_restatement(hip, d):
    n_cases = 0
    for ci, (_, n, pad, offset, n_rows) in enumerate(c for c in cases() if c[0] == d):
        for ki, kind in enumerate(INPUTS):
            hist = history(kind, n_rows, d, n)
            for level in (0, 1, 2):
                p = 1 if level == 0 else N_PREFIXES[(ci + ki + level) % len(N_PREFIXES)]
                table = np.zeros((d, 1), np.uint32) if level == 0 else prefix_table(hist, level, p)
                want = Q.key_counts(hist, level, None if level == 0 else table)
                added, got, before = hip_key_counts(hip, hist, pad, offset, level, table)
                where = (kind, d, n, pad, offset, n_rows, level, table.tolist())
                assert np.array_equal(added, want), where
                if level == 0:
                    assert int(added.sum()) == d * n_rows * n, where
                else:
                    for j in range(d):
                        for s in range(p):
                            if table[j, s] in (Q.UNUSED, ABSENT[level]):          # gained nothing: still what they held
                                assert not added[j, s].any(), where
                    assert any(added[j].any() for j in range(d)), where
                n_cases += 1
    assert n_cases == 8 * 3 * 3


@pytest.mark.gpu
def test_every_prefix_count_meets_every_level(hip):
    """1, 2, 3, 5 and 8 prefixes at levels 1 and 2 on one ragged, padded, misaligned shape, and a constant history: every value in
    one counter"""
    for kind in INPUTS:
        hist = history(kind, 97, 3, 321)
        for level in (1, 2):
            for p in N_PREFIXES:
                table = prefix_table(hist, level, p)
                added, _, _ = hip_key_counts(hip, hist, 17, 3, level, table)
                assert np.array_equal(added, Q.key_counts(hist, level, table)), (kind, level, p)
    const = history("constant", 97, 3, 321)
    k = int(Q.keys(np.float32(-1.75).reshape(1))[0])
    for level, (prefix_bits, digit_bits) in enumerate(Q.LEVELS):
        table = np.full((3, 1), k >> (32 - prefix_bits) if level else 0, np.uint32)
        added, _, _ = hip_key_counts(hip, const, 17, 1, level, table)
        digit = (k >> (32 - prefix_bits - digit_bits)) & ((1 << digit_bits) - 1)
        assert (added[:, 0, digit] == 97 * 321).all() and int(added.sum()) == 3 * 97 * 321


@pytest.mark.gpu
def test_counts_add_over_slabs_of_chains_and_slices_of_rows(hip):
    """two launches into one table, the second from a base pointer inside the first's rows: the sum is the whole's counts"""
    hist = history("diag", 97, 2, 321)
    buf, ptr, stride = placed(hist, 0, 0)
    want = Q.key_counts(hist, 0)
    t, cp, before = prefilled(2 * 2048)
    zero = np.zeros((2, 1), np.uint32)
    for chain0, k in ((0, 130), (130, 191)):
        assert hip.glabc_key_counts(ptr + 4 * chain0, 97, 2, k, stride, 0, 1, zero.ctypes.data, cp, None) == 0
    assert np.array_equal((after(t, 2 * 2048) - before).reshape(2, 1, 2048), want)
    t, cp, before = prefilled(2 * 2048)
    for row0, k in ((0, 40), (40, 57)):
        assert hip.glabc_key_counts(ptr + 4 * row0 * 2 * stride, k, 2, 321, stride, 0, 1, zero.ctypes.data, cp, None) == 0
    assert np.array_equal((after(t, 2 * 2048) - before).reshape(2, 1, 2048), want)


@pytest.mark.gpu
def test_refused_calls_write_nothing(hip):
    n_rows, d, n = 33, 3, 70
    hist = history("diag", n_rows, d, n)
    buf, h, stride = placed(hist, 0, 0)
    ok1 = np.array([[1, 2], [3, 4], [5, 6]], np.uint32)
    dup = np.array([[1, 2], [3, 3], [5, 6]], np.uint32)
    wide = np.array([[1, 2], [3, 1 << 11], [5, 6]], np.uint32)
    t, cp, before = prefilled(d * 2 * 2048)
    for rc, args in ((ERR_NULL, (None, n_rows, d, n, n, 1, 2, ok1.ctypes.data, cp)), (ERR_NULL, (h, n_rows, d, n, n, 1, 2, None, cp)),
                     (ERR_NULL, (h, n_rows, d, n, n, 1, 2, ok1.ctypes.data, None)), (ERR_NULL, (None, n_rows, 0, n, n, 1, 2, ok1.ctypes.data, cp)),
                     (ERR_DIM, (h, n_rows, 0, n, n, 1, 2, ok1.ctypes.data, cp)), (ERR_DIM, (h, n_rows, 9, n, n, 5, 2, ok1.ctypes.data, cp)),
                     (ERR_ARG, (h, 0, d, n, n, 1, 2, ok1.ctypes.data, cp)), (ERR_ARG, (h, n_rows, d, -1, n, 1, 2, ok1.ctypes.data, cp)),
                     (ERR_ARG, (h, n_rows, d, n, n - 1, 1, 2, ok1.ctypes.data, cp)), (ERR_ARG, (h, n_rows, d, n, n, 3, 2, ok1.ctypes.data, cp)),
                     (ERR_ARG, (h, n_rows, d, n, n, -1, 2, ok1.ctypes.data, cp)), (ERR_ARG, (h, n_rows, d, n, n, 1, 0, ok1.ctypes.data, cp)),
                     (ERR_ARG, (h, n_rows, d, n, n, 1, 9, ok1.ctypes.data, cp)), (ERR_ARG, (h, n_rows, d, n, n, 0, 2, ok1.ctypes.data, cp)),
                     (ERR_ARG, (h, n_rows, d, n, n, 1, 2, dup.ctypes.data, cp)), (ERR_ARG, (h, n_rows, d, n, n, 1, 2, wide.ctypes.data, cp)),
                     (0, (h, n_rows, d, 0, n, 1, 2, ok1.ctypes.data, cp)), (0, (h, n_rows, d, 0, 0, 0, 1, ok1.ctypes.data, cp))):
        assert hip.glabc_key_counts(*args, None) == rc, args
        assert np.array_equal(after(t, d * 2 * 2048), before), args
    lo, hi, nan = np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 1.0]), np.array([0.0, np.nan, 0.0])
    for rc, args in ((ERR_NULL, (None, n_rows, d, n, n, 8, lo.ctypes.data, hi.ctypes.data, cp)), (ERR_NULL, (h, n_rows, d, n, n, 8, None, hi.ctypes.data, cp)),
                     (ERR_NULL, (h, n_rows, d, n, n, 8, lo.ctypes.data, None, cp)), (ERR_NULL, (h, n_rows, d, n, n, 8, lo.ctypes.data, hi.ctypes.data, None)),
                     (ERR_DIM, (h, n_rows, 9, n, n, 0, lo.ctypes.data, hi.ctypes.data, cp)), (ERR_ARG, (h, 0, d, n, n, 8, lo.ctypes.data, hi.ctypes.data, cp)),
                     (ERR_ARG, (h, n_rows, d, n, n - 1, 8, lo.ctypes.data, hi.ctypes.data, cp)), (ERR_ARG, (h, n_rows, d, n, n, 0, lo.ctypes.data, hi.ctypes.data, cp)),
                     (ERR_ARG, (h, n_rows, d, n, n, 4097, lo.ctypes.data, hi.ctypes.data, cp)), (ERR_ARG, (h, n_rows, d, n, n, 8, hi.ctypes.data, lo.ctypes.data, cp)),
                     (ERR_ARG, (h, n_rows, d, n, n, 8, lo.ctypes.data, lo.ctypes.data, cp)), (ERR_ARG, (h, n_rows, d, n, n, 8, nan.ctypes.data, hi.ctypes.data, cp)),
                     (0, (h, n_rows, d, 0, n, 8, lo.ctypes.data, hi.ctypes.data, cp))):
        assert hip.glabc_histogram(*args, None) == rc, args
        assert np.array_equal(after(t, d * 2 * 2048), before), args


# ---------------------------------------------------------------------------------- GPU: glabc_histogram
BINS = (1, 2, 63, 64, 65, 4096)
HIST_SHAPES = ((1, 1, 0, 0, 1), (2, 3, 17, 1, 2), (3, 65, 17, 3, 33), (8, 63, 0, 2, 97), (2, 321, 17, 1, 97), (3, 64, 0, 0, 33),
               (1, 5, 17, 2, 2), (2, 4, 0, 3, 97))          # (theta_dim, n_chains, pad, offset, n_rows): ragged, padded, misaligned


def histogram_input(n_rows, d, n, n_bins, lo, hi):
    """diag_history (offsets up to +-50: values on both sides of [-32, 32]) with values planted exactly on lo, on hi, on interior
    edges, next to them, outside both ends, infinite and NaN"""
    hist = np.array(R.diag_history(n_rows, d, n))
    flat = hist.reshape(-1)
    width = (hi - lo) / n_bins
    edge = [np.float32(lo + k * width) for k in sorted({1, n_bins // 2, n_bins - 1}) if 0 < k < n_bins]
    plant = [lo, hi, np.nextafter(np.float32(lo), np.float32(-np.inf)), np.nextafter(np.float32(hi), np.float32(np.inf)),
             np.nextafter(np.float32(hi), np.float32(0)), np.inf, -np.inf, np.nan, -0.0, 100.0, -100.0]
    plant += edge + [np.nextafter(e, np.float32(-np.inf)) for e in edge]
    at = (np.arange(len(plant)) * 7919) % flat.size
    flat[at] = np.array(plant, np.float32)[:len(at)]
    return hist


@pytest.mark.gpu
@pytest.mark.parametrize("n_bins", BINS)
def test_histogram_matches_the_restatement(hip, n_bins):
    for si, (d, n, pad, offset, n_rows) in enumerate(HIST_SHAPES):
        lo = np.array([-32.0, 0.0, -7.5, -32.0, 1.0, -0.1, 20.0, -50.0][:d]) if si % 2 == 0 else np.full(d, -32.0)
        hi = np.array([32.0, 64.0, 0.7, 33.0, 1.5, 0.2, 50.0, 50.0][:d]) if si % 2 == 0 else np.full(d, 32.0)
        hist = histogram_input(n_rows, d, n, n_bins, float(lo[0]), float(hi[0]))
        buf, ptr, stride = placed(hist, pad, offset)
        size = d * (n_bins + 3)
        t, cp, before = prefilled(size)
        assert hip.glabc_histogram(ptr, n_rows, d, n, stride, n_bins, lo.ctypes.data, hi.ctypes.data, cp, None) == 0
        added = (after(t, size) - before).reshape(d, n_bins + 3)
        want = Q.histogram(hist, n_bins, lo, hi)
        assert np.array_equal(added, want), (n_bins, d, n, pad, offset, n_rows, np.argwhere(added != want)[:4])
        assert (added.sum(axis=1) == n_rows * n).all()
        if hist.size > 2000:                                      # the planted values are all there
            x = hist.reshape(-1)
            assert (x == np.float32(lo[0])).any() and (x == np.float32(hi[0])).any() and np.isnan(x).any() and np.isinf(x).any()
            assert added[:, n_bins].any() and added[:, n_bins + 1].any() and added[:, n_bins + 2].any()


# ---------------------------------------------------------------------------------- GPU: diagnostics.py end to end
def same_values(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


@functools.lru_cache(maxsize=None)
def sorted_columns(n_rows, d, n):
    hist = R.diag_history(n_rows, d, n)
    s = np.stack([np.sort(hist[:, j].reshape(-1)) for j in range(d)], axis=1)          # [N][d]
    s.setflags(write=False)
    return s


def layouts(hist):
    """the same chain-major history as every kind of argument -> [(history, layout)]"""
    rows = np.array(hist.transpose(0, 2, 1), order="C")                              # (T, C, D), its own memory
    buf = dev(np.array(hist))
    return [(buf.permute(0, 2, 1), "rows"), (rows, "rows"), (torch.from_numpy(rows), "rows"), (np.array(hist), "chain_major"),
            (buf, "chain_major")], buf


@pytest.mark.gpu
def test_order_statistics_quantile_interval_histogram_in_every_layout(hip):
    from glabcmcmc_amd import diagnostics as D
    hist = R.diag_history(97, 3, 321)
    s = sorted_columns(97, 3, 321)
    n = s.shape[0]
    ranks = [0, 1, n // 4, n // 2, n - 2, n - 1] + sorted({(i * (n - 1)) // 8 for i in range(9)})          # more than 8 prefixes
    qs = (0.0, 0.025, 1.0 / 3.0, 0.5, 0.975, 1.0)
    want_q = Q.quantile(hist, qs)
    want_i = Q.quantile(hist, ((1.0 - 0.95) / 2.0, (1.0 + 0.95) / 2.0))          # not 0.025 and 0.975 to the last bit
    lo, hi = s[0].astype(np.float64), s[-1].astype(np.float64)
    want_h, want_h2 = Q.histogram(hist, 65, lo, hi), Q.histogram(hist, 64, np.full(3, -32.0), np.full(3, 32.0))
    args, buf = layouts(hist)
    assert D._chain_major(args[0][0], "rows").data_ptr() == buf.data_ptr()          # the (T, C, D) view is used in place
    for history_arg, layout in args:
        got = D.order_statistics(history_arg, ranks, layout=layout)
        assert got.dtype == np.float32 and same_values(got, s[ranks])
        got_q = D.quantile(history_arg, qs, layout=layout)
        assert got_q.dtype == np.float64 and np.array_equal(got_q, want_q)
        lower, upper = D.interval(history_arg, 0.95, layout=layout)
        assert np.array_equal(lower, want_i[0]) and np.array_equal(upper, want_i[1])
        h = D.histogram(history_arg, 65, layout=layout)
        assert np.array_equal(h.edges[:, 0], lo) and np.array_equal(h.edges[:, -1], hi) and h.edges.shape == (3, 66)
        assert np.array_equal(h.counts, want_h[:, :65]) and not h.below.any() and not h.above.any() and not h.nan.any()
        assert h.counts.dtype == np.uint64 and (h.counts.sum(axis=1) == n).all()
        h = D.histogram(history_arg, 64, (-32.0, 32.0), layout=layout)
        assert np.array_equal(h.counts, want_h2[:, :64]) and np.array_equal(h.below, want_h2[:, 64])
        assert np.array_equal(h.above, want_h2[:, 65]) and h.below.any() and h.above.any()
        assert np.array_equal(h.edges, np.tile(np.linspace(-32.0, 32.0, 65), (3, 1)))
    counts = D.key_counts(args[0][0], 0)
    assert counts.dtype == np.uint64 and np.array_equal(counts, Q.key_counts(hist, 0))
    one = D.order_statistics(np.array(hist[:, :, 5]), [0, 96])                       # (T, D): a single chain
    assert same_values(one, np.stack([hist[:, :, 5].min(axis=0), hist[:, :, 5].max(axis=0)]))


@pytest.mark.gpu
def test_special_values_nan_and_a_constant_coordinate(hip):
    from glabcmcmc_amd import diagnostics as D
    hist = np.array(Q.special_history(33, 3, 65))
    hist[:, 2, :] = np.float32(7.25)                                                  # a constant coordinate
    s = np.stack([np.sort(hist[:, j].reshape(-1)) for j in range(3)], axis=1)
    n = s.shape[0]
    ranks = list(range(0, n, 97)) + [n - 1]
    assert same_values(D.order_statistics(hist, ranks, layout="chain_major"), s[ranks])
    got = D.quantile(hist, (0.0, 0.5, 1.0), layout="chain_major")
    assert same_values(got, Q.quantile(hist, (0.0, 0.5, 1.0))) and np.isnan(got[:, :2]).all() and (got[:, 2] == 7.25).all()
    with pytest.raises(ValueError):                                                   # the minimum is -inf: no finite range
        D.histogram(hist, 16, layout="chain_major")
    finite = np.where(np.isfinite(hist), hist, np.float32(np.nan))
    h = D.histogram(finite, 16, layout="chain_major")
    lo, hi = np.nanmin(finite, axis=(0, 2)).astype(np.float64), np.nanmax(finite, axis=(0, 2)).astype(np.float64)
    lo[2], hi[2] = 6.75, 7.75                                                         # widened by +-0.5, like NumPy
    assert np.array_equal(h.edges[:, 0], lo) and np.array_equal(h.edges[:, -1], hi)
    want = Q.histogram(finite, 16, lo, hi)
    assert np.array_equal(h.counts, want[:, :16]) and np.array_equal(h.nan, want[:, 18]) and h.nan[0] > 0 and h.nan[2] == 0
    assert h.counts[2, 8] == 33 * 65 and np.array_equal(h.counts[2], np.histogram(finite[:, 2].reshape(-1), 16)[0])


@pytest.mark.gpu
def test_select_of_sharded_counts_is_the_whole(hip):
    from glabcmcmc_amd import diagnostics as D
    hist = R.diag_history(97, 3, 321)
    s = sorted_columns(97, 3, 321)
    n = s.shape[0]
    rows = dev(np.array(hist)).permute(0, 2, 1)                                      # (T, C, D)
    shards = (rows[:, :130], rows[:, 130:])
    calls = []

    def all_reduced(level, prefixes):
        calls.append(level)
        return sum(D.key_counts(shard, level, prefixes) for shard in shards)
    ranks = [0, n // 3, n // 2, n - 1]
    assert same_values(D.select(all_reduced, ranks=ranks), s[ranks]) and calls == [0, 1, 2]
    qs = (0.025, 0.5, 0.975)
    assert np.array_equal(D.select(all_reduced, q=qs), D.quantile(rows, qs))
    assert np.array_equal(D.select(all_reduced, q=qs), Q.quantile(hist, qs))


@pytest.mark.gpu
def test_quantiles_of_a_sampler_run_in_place(hip):
    import glabcmcmc_amd as g
    from glabcmcmc_amd import diagnostics as D
    from glabcmcmc_amd.examples.Mixture import Mixture_set
    m = Mixture_set(0.3)
    lp = g.DiagGaussian(2, loc=torch.zeros(1, 2), log_scale=torch.log(torch.tensor([0.35, 0.35])))
    ip = g.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.tensor([0.0, 0.0]))
    chains, iters = 256, 200
    out = g.GLMCMC(m, iters, torch.zeros(chains, 2), torch.zeros(chains, 2) + 0.1, lp, None, 0.7, ip, 5, seed=11, return_device=True,
                   verbose=False)
    assert out.is_cuda and out.shape == (iters, chains, 2)
    x = out.cpu().numpy().reshape(-1, 2).astype(np.float64)
    s = np.sort(x, axis=0)
    n = s.shape[0]
    qs = (0.025, 0.25, 0.5, 0.75, 0.975)
    got = D.quantile(out, qs)
    for i, q in enumerate(qs):
        a = int(np.floor(q * (n - 1)))
        bound = 4 * np.spacing(np.maximum(np.abs(s[a]), np.abs(s[min(a + 1, n - 1)])))
        err = np.abs(got[i] - np.quantile(x, q, axis=0))
        print("q = %.3f: %r, |error| / bound %.3g" % (q, got[i].tolist(), (err / bound).max()))
        assert (err <= bound).all()
    assert same_values(D.order_statistics(out, [0, n // 2, n - 1]), s[[0, n // 2, n - 1]].astype(np.float32))
    lower, upper = D.interval(out, 0.5)                                             # (1 - 0.5) / 2 and (1 + 0.5) / 2 are exact
    assert np.array_equal(lower, got[1]) and np.array_equal(upper, got[3])
    for h in (D.histogram(out), D.histogram(out, 100, (-1.0, 1.0))):
        assert (h.counts.sum(axis=1) + h.below + h.above + h.nan == iters * chains).all()
    h = D.histogram(out)
    chain_major = np.ascontiguousarray(out.cpu().numpy().transpose(0, 2, 1))
    assert np.array_equal(h.edges[:, 0], s[0]) and np.array_equal(h.edges[:, -1], s[-1])
    assert np.array_equal(h.counts, Q.histogram(chain_major, 64, s[0], s[-1])[:, :64])
