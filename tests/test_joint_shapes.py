"""glabc_histogram2d and glabc_cross_moments (csrc/glabc_joint.hip) at every shape at which their kernels take another path, held
to the NumPy restatement of their specifications (tests/joint_ref.py), and the joint functions of glabcmcmc_amd/diagnostics.py.

joint_kernel cuts a pair's work into items of 64 chains x 8 rows that the 8 wavefronts of its workgroups take round-robin and
loads every row segment of both coordinates through a descriptor of exactly its bytes; cross_kernel<D> gives a chain to a lane
and walks its rows in batches of 32 / D with a one-row tail.  So the grids have chains on both sides of 64 and of the 4-float
alignment of a wide load, one row, rows on both sides of 8, of 8 x 8 and of every batch length (129 = 4 x 32 + 1), a stride that
is no multiple of 4 (pad 17), padding columns that hold NaN (a read of one changes the NaN counter, or a chain's sums) and a base
pointer 1, 2 and 3 floats into a wider buffer.  Bins 1, 2, 7 and 128 (the table past 64 KB of LDS); one pair, a pair with its
transpose, a repeated pair, all D (D - 1) / 2 pairs (28 at D = 8, the most a launch takes).  The cases are covering grids, not
full products: test_grids_cover_every_pair checks that every value of an axis meets at least two values of every other axis.

Tolerances: none for counts (equal integers) and for the per-chain moments (equal float64 bits, NaN matching NaN).  The pooled
covariance against the restatement: COV_TOLERANCE of tests/test_joint_host.py, in units of eps sqrt(v_ii v_jj).  The sums of
joint_terms over C chains against float64 sums of the restatement's per-chain numbers: (C - 1) eps sum |x|, the bound of a sum of C
numbers in any order.
"""
import functools

import numpy as np
import pytest
import torch

import diag_ref as R
import joint_ref as J
import quantile_ref as Q
from helpers import dev, host
from test_joint_host import COV_TOLERANCE, all_pairs, cov_units, same_bits

ERR_NULL, ERR_DIM, ERR_ARG = -1, -2, -4          # glabc_status, include/glabc.h

DIMS = (2, 3, 8)
CROSS_DIMS = (1, 2, 3, 8)
CHAINS = (1, 3, 4, 5, 63, 64, 65, 321)
PADS = (0, 17)
OFFSETS = (0, 1, 2, 3)                            # floats between the device buffer's base and the history's
ROWS = (1, 2, 33, 97, 129)
BINS = (1, 2, 7, 128)
PAIR_SETS = ("one", "both", "repeated", "all")
INPUTS = ("diag", "special", "constant")
GUARD = 7                                         # canary elements on either side of an output
CANARY = np.uint64(0xDEADC0DEDEADBEEF)
EPS = np.finfo(np.float64).eps


def grid(dims):
    """(theta_dim, n_chains, pad, offset, n_rows): two chain counts per (theta_dim, n_rows)"""
    out = []
    for di, d in enumerate(dims):
        for ri, n_rows in enumerate(ROWS):
            for s in (0, 1):
                ci = (2 * di + ri + 4 * s) % len(CHAINS)
                out.append((d, CHAINS[ci], PADS[(di + ci // 2 + s) % 2], OFFSETS[(di + ri + ci // 2 + s) % 4], n_rows))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def count_cases():
    """the shapes of grid(DIMS), each with (bins, pair set, input): rotations of different periods, so that the axes do not move in step"""
    out = []
    for i, shape in enumerate(grid(DIMS)):
        out.append(shape + (BINS[(i + i // 2) % 4], PAIR_SETS[(i + i // 7) % 4], INPUTS[(i + i // 3) % 3]))
    return tuple(out)


def covered(rows, axes):
    for a in range(len(axes)):
        assert {c[a] for c in rows} == set(axes[a]), (a, {c[a] for c in rows})
        for b in range(len(axes)):
            if a != b:
                for v in axes[a]:
                    met = {c[b] for c in rows if c[a] == v}
                    assert len(met) >= 2, (a, v, b, met)


def test_grids_cover_every_pair():
    covered(grid(CROSS_DIMS), (CROSS_DIMS, CHAINS, PADS, OFFSETS, ROWS))
    covered(count_cases(), (DIMS, CHAINS, PADS, OFFSETS, ROWS, BINS, PAIR_SETS, INPUTS))


@functools.lru_cache(maxsize=None)
def history(kind, n_rows, d, n):
    if kind == "diag":
        return R.diag_history(n_rows, d, n)
    h = Q.special_history(n_rows, d, n) if kind == "special" else np.full((n_rows, d, n), np.float32(-1.75))
    h.setflags(write=False)
    return h


def limits(kind, d, turn):
    """lo, hi [d] that leave values outside, and put values on lo and on hi: diag has offsets up to +-50; special holds -1, 2.5,
    +-0, +-inf and NaN; the constant is -1.75, on lo or on hi by turns"""
    if kind == "diag":
        return np.linspace(-32.0, -20.0, d), np.linspace(32.0, 45.0, d)
    if kind == "special":
        return np.full(d, -1.0), np.full(d, 2.5)
    return (np.full(d, -1.75), np.full(d, 0.0)) if turn % 2 else (np.full(d, -3.0), np.full(d, -1.75))


def pair_set(name, d, turn):
    a, b = turn % d, (turn + 1 + turn // d % (d - 1)) % d
    if a == b:
        b = (a + 1) % d
    other = ((a + 1) % d, (b + 1) % d) if (a + 1) % d != (b + 1) % d else (b, a)
    return {"one": [(a, b)], "both": [(a, b), (b, a)], "repeated": [(a, b), other, (a, b)], "all": all_pairs(d)}[name]


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
    assert (a[:GUARD] == CANARY).all() and (a[GUARD + size:] == CANARY).all(), "the output's guard bands were written"
    return a[GUARD:GUARD + size]


def hip_histogram2d(hip, hist, pad, offset, pairs, n_bins, lo, hi):
    n_rows, d, n = hist.shape
    buf, ptr, stride = placed(hist, pad, offset)
    table = np.ascontiguousarray(pairs, np.int32)
    size = len(pairs) * (n_bins * n_bins + 2)
    t, cp, before = prefilled(size)
    lo, hi = np.ascontiguousarray(lo, np.float64), np.ascontiguousarray(hi, np.float64)
    assert hip.glabc_histogram2d(ptr, n_rows, d, n, stride, len(pairs), table.ctypes.data, n_bins, lo.ctypes.data, hi.ctypes.data, cp, None) == 0
    return (after(t, size) - before).reshape(len(pairs), -1)


# ---------------------------------------------------------------------------------- GPU: glabc_histogram2d
@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_histogram2d_matches_the_restatement(hip, d):
    n_cases = 0
    for i, (_, n, pad, offset, n_rows, n_bins, pairs_name, kind) in enumerate(c for c in count_cases() if c[0] == d):
        hist = history(kind, n_rows, d, n)
        lo, hi = limits(kind, d, i)
        pairs = pair_set(pairs_name, d, i)
        if pairs_name == "one" and d > 2:                              # a coordinate no pair uses: its lo and hi are not looked at
            lo, hi = lo.copy(), hi.copy()
            unused = [j for j in range(d) if j not in pairs[0]]
            lo[unused[0]], hi[unused[-1]] = np.nan, -np.inf
        added = hip_histogram2d(hip, hist, pad, offset, pairs, n_bins, lo, hi)
        want = J.histogram2d(hist, pairs, n_bins, lo, hi)
        where = (kind, d, n, pad, offset, n_rows, n_bins, pairs)
        assert np.array_equal(added, want), (where, np.argwhere(added != want)[:4])
        assert (added.sum(axis=1) == n_rows * n).all(), where
        if kind == "special" and n_rows * n > 200:
            assert added[:, -1].all() and added[:, -2].all() and added[:, :-2].any(), where
        n_cases += 1
    assert n_cases == 10


@pytest.mark.gpu
def test_every_bin_count_and_pair_set_on_one_ragged_shape(hip):
    """bins x pair sets x inputs on one padded, misaligned shape of more than one workgroup's items, D = 3 and the 28 pairs of D = 8"""
    for kind in INPUTS:
        for d, n_rows, n in ((3, 97, 321), (8, 33, 65)):
            hist = history(kind, n_rows, d, n)
            lo, hi = limits(kind, d, 1)
            for bi, n_bins in enumerate(BINS):
                for pi, name in enumerate(PAIR_SETS):
                    if d == 8 and (bi + pi) % 2:
                        continue
                    pairs = pair_set(name, d, bi + pi)
                    added = hip_histogram2d(hip, hist, 17, 3, pairs, n_bins, lo, hi)
                    assert np.array_equal(added, J.histogram2d(hist, pairs, n_bins, lo, hi)), (kind, d, n_bins, pairs)
    assert len(pair_set("all", 8, 0)) == 28


@pytest.mark.gpu
def test_counts_add_over_slabs_of_chains_and_slices_of_rows(hip):
    """two launches into one table, the second from a base pointer inside the first's rows: the sum is the whole's counts"""
    hist = history("diag", 97, 3, 321)
    buf, ptr, stride = placed(hist, 0, 0)
    pairs = np.array(all_pairs(3), np.int32)
    lo, hi = np.full(3, -32.0), np.full(3, 32.0)
    want = J.histogram2d(hist, all_pairs(3), 7, lo, hi).reshape(-1)
    for parts in (((0, 97, 0, 130), (0, 97, 130, 191)), ((0, 40, 0, 321), (40, 57, 0, 321))):
        t, cp, before = prefilled(3 * 51)
        for row0, rows, chain0, k in parts:
            assert hip.glabc_histogram2d(ptr + 4 * (row0 * 3 * stride + chain0), rows, 3, k, stride, 3, pairs.ctypes.data, 7, lo.ctypes.data,
                                         hi.ctypes.data, cp, None) == 0
        assert np.array_equal(after(t, 3 * 51) - before, want), parts


def hip_cross(hip, hist, pad, offset, n=None, expect=0):
    n_rows, d, chains = hist.shape
    n = chains if n is None else n
    buf, ptr, stride = placed(hist, pad, offset)
    tri = d * (d + 1) // 2
    outs = []
    for size in (d * n, tri * n):
        guard = np.full(GUARD, CANARY).view(np.float64)
        t = dev(np.concatenate([guard, np.full(size, 12345.5), guard]))
        outs.append((t, t.data_ptr() + 8 * GUARD, size))
    assert hip.glabc_cross_moments(ptr, n_rows, d, n, stride, outs[0][1], outs[1][1], None) == expect
    got = []
    for t, _, size in outs:
        a = host(t)
        assert (a[:GUARD].view(np.uint64) == CANARY).all() and (a[GUARD + size:].view(np.uint64) == CANARY).all(), "guard bands written"
        got.append(a[GUARD:GUARD + size])
    return got[0].reshape(d, n), got[1].reshape(tri, n)


# ---------------------------------------------------------------------------------- GPU: glabc_cross_moments
@pytest.mark.gpu
@pytest.mark.parametrize("d", CROSS_DIMS)
def test_cross_moments_match_the_restatement(hip, d):
    n_cases = 0
    for _, n, pad, offset, n_rows in (c for c in grid(CROSS_DIMS) if c[0] == d):
        for kind in INPUTS:
            hist = history(kind, n_rows, d, n)
            mean, cov = hip_cross(hip, hist, pad, offset)
            want_mean, want_cov = J.cross_moments(hist)
            where = (kind, d, n, pad, offset, n_rows)
            assert same_bits(mean, want_mean), where
            assert same_bits(cov, want_cov), (where, np.argwhere(~((cov == want_cov) | (np.isnan(cov) & np.isnan(want_cov))))[:4])
            if kind == "constant":
                assert (mean == -1.75).all() and (cov == 0.0).all()
            if kind == "special" and n_rows * n > 200:
                assert np.isnan(cov).any()
            n_cases += 1
    assert n_cases == 30


@pytest.mark.gpu
def test_cross_moments_diagonal_is_autocov_and_non_finite_values_stay_put(hip):
    hist = np.array(R.diag_history(97, 3, 321))
    mean, cov = hip_cross(hip, hist, 17, 1)
    buf, ptr, stride = placed(hist, 17, 1)
    m = torch.empty(3, 321, dtype=torch.float64, device="cuda")
    a = torch.empty(1, 3, 321, dtype=torch.float64, device="cuda")
    assert hip.glabc_autocov(ptr, 97, 3, 321, stride, 0, m.data_ptr(), a.data_ptr(), None) == 0
    assert same_bits(mean, host(m))
    for j in range(3):
        assert same_bits(cov[J.packed_index(j, j, 3)], host(a)[0, j]), j
    hist[5, 1, 7], hist[9, 2, 11] = np.nan, np.inf
    mean2, cov2 = hip_cross(hip, hist, 0, 0)
    changed = ~((cov2 == cov) | (np.isnan(cov2) & np.isnan(cov)))
    assert sorted(map(tuple, np.argwhere(changed).tolist())) == sorted(
        [(J.packed_index(i, j, 3), 7) for i in range(3) for j in range(i, 3) if 1 in (i, j)] +
        [(J.packed_index(i, j, 3), 11) for i in range(3) for j in range(i, 3) if 2 in (i, j)])
    assert same_bits(cov2, J.cross_moments(hist)[1]) and same_bits(mean2, J.cross_moments(hist)[0])


# ---------------------------------------------------------------------------------- GPU: refusals
@pytest.mark.gpu
def test_refused_calls_write_nothing(hip):
    n_rows, d, n = 33, 3, 70
    hist = history("diag", n_rows, d, n)
    buf, h, stride = placed(hist, 0, 0)
    ok = np.array([[0, 1], [2, 1]], np.int32)
    same = np.array([[0, 1], [2, 2]], np.int32)
    high = np.array([[0, 1], [3, 1]], np.int32)
    neg = np.array([[0, 1], [-1, 1]], np.int32)
    first = np.array([[0, 1], [1, 0]], np.int32)
    lo, hi, nan = np.array([0.0, 0.0, 0.0]), np.array([1.0, 1.0, 1.0]), np.array([0.0, 0.0, np.nan])
    size = 2 * (8 * 8 + 2)
    t, cp, before = prefilled(size)
    P, L, H = ok.ctypes.data, lo.ctypes.data, hi.ctypes.data
    for rc, args in ((ERR_NULL, (None, n_rows, d, n, n, 2, P, 8, L, H, cp)), (ERR_NULL, (h, n_rows, d, n, n, 2, None, 8, L, H, cp)),
                     (ERR_NULL, (h, n_rows, d, n, n, 2, P, 8, None, H, cp)), (ERR_NULL, (h, n_rows, d, n, n, 2, P, 8, L, None, cp)),
                     (ERR_NULL, (h, n_rows, d, n, n, 2, P, 8, L, H, None)), (ERR_NULL, (None, n_rows, 0, n, n, 2, P, 8, L, H, cp)),
                     (ERR_DIM, (h, n_rows, 0, n, n, 2, P, 8, L, H, cp)), (ERR_DIM, (h, n_rows, 9, n, n, 0, P, 0, L, H, cp)),
                     (ERR_ARG, (h, 0, d, n, n, 2, P, 8, L, H, cp)), (ERR_ARG, (h, n_rows, d, -1, n, 2, P, 8, L, H, cp)),
                     (ERR_ARG, (h, n_rows, d, n, n - 1, 2, P, 8, L, H, cp)), (ERR_ARG, (h, n_rows, d, n, n, 0, P, 8, L, H, cp)),
                     (ERR_ARG, (h, n_rows, d, n, n, 29, P, 8, L, H, cp)), (ERR_ARG, (h, n_rows, d, n, n, 2, same.ctypes.data, 8, L, H, cp)),
                     (ERR_ARG, (h, n_rows, d, n, n, 2, high.ctypes.data, 8, L, H, cp)), (ERR_ARG, (h, n_rows, d, n, n, 2, neg.ctypes.data, 8, L, H, cp)),
                     (ERR_ARG, (h, n_rows, 2, n, n, 2, P, 8, L, H, cp)),
                     (ERR_ARG, (h, n_rows, d, n, n, 2, P, 0, L, H, cp)), (ERR_ARG, (h, n_rows, d, n, n, 2, P, 129, L, H, cp)),
                     (ERR_ARG, (h, n_rows, d, n, n, 2, P, 8, H, L, cp)), (ERR_ARG, (h, n_rows, d, n, n, 2, P, 8, L, L, cp)),
                     (ERR_ARG, (h, n_rows, d, n, n, 2, P, 8, nan.ctypes.data, H, cp)), (ERR_ARG, (h, n_rows, d, n, n, 2, P, 8, L, nan.ctypes.data, cp)),
                     (0, (h, n_rows, d, 0, n, 2, P, 8, L, H, cp)), (0, (h, n_rows, d, 0, 0, 2, P, 8, L, H, cp))):
        assert hip.glabc_histogram2d(*args, None) == rc, args
        assert np.array_equal(after(t, size), before), args
    # the NaN sits on coordinate 2: fine as long as no pair uses it
    assert hip.glabc_histogram2d(h, n_rows, d, n, n, 2, first.ctypes.data, 8, nan.ctypes.data, H, cp, None) == 0
    assert not np.array_equal(after(t, size), before)

    guard = np.full(GUARD, CANARY).view(np.float64)
    out = dev(np.concatenate([guard, np.full(6 * n, 12345.5), guard]))
    held = host(out).copy()
    m, v = out.data_ptr() + 8 * GUARD, out.data_ptr() + 8 * (GUARD + 3 * n)          # too small for the covariance: nothing may be written
    for rc, args in ((ERR_NULL, (None, n_rows, d, n, n, m, v)), (ERR_NULL, (h, n_rows, d, n, n, None, v)), (ERR_NULL, (h, n_rows, d, n, n, m, None)),
                     (ERR_NULL, (None, n_rows, 9, n, n, m, v)), (ERR_DIM, (h, n_rows, 0, n, n, m, v)), (ERR_DIM, (h, 0, 9, n, n, m, v)),
                     (ERR_ARG, (h, 0, d, n, n, m, v)), (ERR_ARG, (h, n_rows, d, -1, n, m, v)), (ERR_ARG, (h, n_rows, d, n, n - 1, m, v)),
                     (0, (h, n_rows, d, 0, n, m, v)), (0, (h, n_rows, d, 0, 0, m, v))):
        assert hip.glabc_cross_moments(*args, None) == rc, args
        assert np.array_equal(host(out).view(np.uint64), held.view(np.uint64)), args


# ---------------------------------------------------------------------------------- GPU: diagnostics.py end to end
def layouts(hist):
    """the same chain-major history as every kind of argument -> [(history, layout)]"""
    rows = np.array(hist.transpose(0, 2, 1), order="C")                              # (T, C, D), its own memory
    buf = dev(np.array(hist))
    return [(buf.permute(0, 2, 1), "rows"), (rows, "rows"), (torch.from_numpy(rows), "rows"), (np.array(hist), "chain_major"),
            (buf, "chain_major")], buf


def sum_close(got, parts, axis):
    """a float64 sum over `axis` of C numbers, in any order: within (C - 1) eps sum |x|"""
    parts = np.asarray(parts, np.float64)
    bound = (parts.shape[axis] - 1) * EPS * np.abs(parts).sum(axis=axis)
    return bool((np.abs(np.asarray(got) - parts.sum(axis=axis)) <= bound).all())


@functools.lru_cache(maxsize=None)
def module_reference():
    hist = R.diag_history(97, 3, 321)
    mean, cov = J.cross_moments(hist)
    full = np.stack([[cov[J.packed_index(min(i, j), max(i, j), 3)] for j in range(3)] for i in range(3)])          # [3][3][C]
    return hist, mean, cov, full, J.covariance(hist), J.correlation(hist)


@pytest.mark.gpu
def test_module_functions_in_every_layout(hip):
    from glabcmcmc_amd import diagnostics as D
    hist, mean, cov, full, want_cov, want_corr = module_reference()
    lo, hi = hist.min(axis=(0, 2)).astype(np.float64), hist.max(axis=(0, 2)).astype(np.float64)
    want_auto = J.histogram2d(hist, all_pairs(3), 7, lo, hi)
    pairs = [(2, 0), (0, 2), (1, 2)]
    want_fixed = J.histogram2d(hist, pairs, 64, np.full(3, -32.0), np.full(3, 32.0))
    args, buf = layouts(hist)
    assert D._chain_major(args[0][0], "rows").data_ptr() == buf.data_ptr()          # the (T, C, D) view is used in place
    for history_arg, layout in args:
        h = D.histogram2d(history_arg, bins=7, layout=layout)
        assert h.counts.dtype == np.uint64 and h.counts.shape == (3, 7, 7) and h.pairs.tolist() == [[0, 1], [0, 2], [1, 2]]
        assert np.array_equal(h.counts.reshape(3, -1), want_auto[:, :49]) and not h.outside.any() and not h.nan.any()
        assert np.array_equal(h.edges[:, 0], lo) and np.array_equal(h.edges[:, -1], hi) and h.edges.shape == (3, 8)
        marg = D.histogram(history_arg, 7, layout=layout)              # range=None: the margins are the marginal histograms
        for p, (a, b) in enumerate(h.pairs):
            assert np.array_equal(h.counts[p].sum(axis=1), marg.counts[a]) and np.array_equal(h.counts[p].sum(axis=0), marg.counts[b])
        h = D.histogram2d(history_arg, pairs, 64, (-32.0, 32.0), layout=layout)
        assert np.array_equal(h.counts.reshape(3, -1), want_fixed[:, :4096]) and np.array_equal(h.outside, want_fixed[:, 4096])
        assert h.outside.all() and not h.nan.any() and np.array_equal(h.counts[0], h.counts[1].T)
        assert np.array_equal(h.edges, np.tile(np.linspace(-32.0, 32.0, 65), (3, 1)))
        m, v = D.cross_moments(history_arg, layout=layout)
        assert m.is_cuda and v.is_cuda and m.dtype == v.dtype == torch.float64 and same_bits(host(m), mean) and same_bits(host(v), cov)
        t = D.joint_terms(history_arg, layout=layout)
        assert (t.M, t.n) == (321, 97) and sum_close(t.sum_mean, mean, 1) and sum_close(t.sum_cov, full, 2)
        assert sum_close(t.sum_mean_outer, mean[:, None, :] * mean[None, :, :], 2) and np.array_equal(t.sum_cov, t.sum_cov.T)
        got = D.covariance(history_arg, layout=layout)
        assert got.shape == (3, 3) and np.array_equal(got, got.T) and cov_units(got, want_cov) <= COV_TOLERANCE
        assert np.array_equal(D.covariance(t), got)
        r = D.correlation(history_arg, layout=layout)
        assert np.allclose(r, want_corr, rtol=0, atol=(2 * COV_TOLERANCE + 4) * EPS) and np.array_equal(r, D.correlation(t))
    one = np.array(hist[:, :, 5])                                      # (T, D): a single chain
    h = D.histogram2d(one, [(0, 1)], 2)
    assert h.counts.sum() == 97 and np.array_equal(h.counts[0], J.histogram2d(hist[:, :, 5:6], [(0, 1)], 2, h.edges[:, 0], h.edges[:, -1])[0, :4].reshape(2, 2))
    assert cov_units(D.covariance(one), np.cov(one.astype(np.float64), rowvar=False)) <= COV_TOLERANCE


@pytest.mark.gpu
def test_shards_of_chains_combine_to_the_whole(hip):
    from glabcmcmc_amd import diagnostics as D
    hist, mean, cov, full, want_cov, _ = module_reference()
    rows = dev(np.array(hist)).permute(0, 2, 1)                                      # (T, C, D)
    shards = (rows[:, :130], rows[:, 130:])
    both = D.combine_joint([D.joint_terms(s) for s in shards])
    whole = D.joint_terms(rows)
    assert (both.M, both.n) == (whole.M, whole.n) == (321, 97)
    assert cov_units(D.covariance(both), D.covariance(whole)) <= COV_TOLERANCE and cov_units(D.covariance(both), want_cov) <= COV_TOLERANCE
    parts = [D.histogram2d(s, None, 7, (-32.0, 32.0)) for s in shards]
    h = D.histogram2d(rows, None, 7, (-32.0, 32.0))
    assert np.array_equal(parts[0].counts + parts[1].counts, h.counts) and np.array_equal(parts[0].outside + parts[1].outside, h.outside)
    assert np.array_equal(h.counts.reshape(3, -1), J.histogram2d(hist, all_pairs(3), 7, np.full(3, -32.0), np.full(3, 32.0))[:, :49])


@pytest.mark.gpu
def test_more_pairs_than_a_launch_takes_and_special_values(hip):
    from glabcmcmc_amd import diagnostics as D
    hist = np.array(Q.special_history(33, 3, 65))
    hist[:, 2, :] = np.float32(7.25)                                                  # a constant coordinate
    pairs = (all_pairs(3) + [(b, a) for a, b in all_pairs(3)]) * 5 + [(2, 0)]         # 31 pairs: two launches
    h = D.histogram2d(hist, pairs, 4, [(-1.0, 2.5), (-1.0, 2.5), (7.0, 7.5)], layout="chain_major")
    want = J.histogram2d(hist, pairs, 4, [-1.0, -1.0, 7.0], [2.5, 2.5, 7.5])
    assert h.counts.shape == (31, 4, 4) and h.pairs.tolist() == [list(p) for p in pairs]
    assert np.array_equal(h.counts.reshape(31, -1), want[:, :16]) and np.array_equal(h.outside, want[:, 16]) and np.array_equal(h.nan, want[:, 17])
    assert h.nan.all() and h.outside.all() and np.array_equal(h.counts[30], h.counts[1].T)
    with pytest.raises(ValueError):                                                   # the minimum is -inf: no finite range
        D.histogram2d(hist, layout="chain_major")
    finite = np.where(np.isfinite(hist), hist, np.float32(np.nan))
    h = D.histogram2d(finite, [(0, 2)], 16, layout="chain_major")
    assert h.edges[2, 0] == 6.75 and h.edges[2, -1] == 7.75                          # widened by +-0.5, as histogram
    assert np.array_equal(h.counts[0].sum(axis=1), D.histogram(finite, 16, layout="chain_major").counts[0]) and not h.counts[0][:, :8].any()
    r = D.correlation(np.where(np.isfinite(hist), hist, np.float32(1.0)), layout="chain_major")
    assert np.isnan(r[2]).all() and np.isnan(r[:, 2]).all() and r[0, 0] == 1.0 and np.isfinite(r[0, 1])
    level, mass, inside = D.hpd_levels(h.counts)
    assert level.shape == (1, 3) and (mass >= np.ceil(np.array([0.5, 0.9, 0.95]) * int(h.counts.sum()))).all()


@pytest.mark.gpu
def test_joint_summaries_of_a_sampler_run_in_place(hip):
    import glabcmcmc_amd as g
    from glabcmcmc_amd import diagnostics as D
    from glabcmcmc_amd.examples.Mixture import Mixture_set
    m = Mixture_set(0.3)
    lp = g.DiagGaussian(2, loc=torch.zeros(1, 2), log_scale=torch.log(torch.tensor([0.35, 0.35])))
    ip = g.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.tensor([0.0, 0.0]))
    chains, iters = 256, 200
    out = g.GLMCMC(m, iters, torch.zeros(chains, 2), torch.zeros(chains, 2) + 0.1, lp, None, 0.7, ip, 5, seed=11, return_device=True,
                   verbose=False)
    x = out.cpu().numpy().reshape(-1, 2).astype(np.float64)
    chain_major = np.ascontiguousarray(out.cpu().numpy().transpose(0, 2, 1))
    got = D.covariance(out)
    print("covariance %r, against numpy.cov %.2f eps sqrt(v_ii v_jj)" % (got.tolist(), cov_units(got, np.cov(x, rowvar=False))))
    assert cov_units(got, np.cov(x, rowvar=False)) <= COV_TOLERANCE and cov_units(got, J.covariance(chain_major)) <= COV_TOLERANCE
    h = D.histogram2d(out, bins=2, range=(-1024.0, 1024.0))                        # the mass of each quadrant
    quadrants = np.array([[((x[:, 0] < 0) & (x[:, 1] < 0)).sum(), ((x[:, 0] < 0) & (x[:, 1] >= 0)).sum()],
                          [((x[:, 0] >= 0) & (x[:, 1] < 0)).sum(), ((x[:, 0] >= 0) & (x[:, 1] >= 0)).sum()]])
    assert np.array_equal(h.counts[0], quadrants) and h.counts.sum() == iters * chains and not h.outside.any() and not h.nan.any()
    h = D.histogram2d(out)
    lo, hi = x.min(axis=0), x.max(axis=0)
    assert np.array_equal(h.counts.reshape(1, -1), J.histogram2d(chain_major, [(0, 1)], 64, lo, hi)[:, :4096]) and h.counts.sum() == iters * chains
    level, mass, inside = D.hpd_levels(h.counts[0])
    for i, p in enumerate((0.5, 0.9, 0.95)):
        assert (int(level[i]), int(mass[i]), int(inside[i])) == J.hpd_level(h.counts[0], p)[1:]
    assert (np.diff(level.astype(np.int64)) <= 0).all() and (np.diff(inside) >= 0).all()
