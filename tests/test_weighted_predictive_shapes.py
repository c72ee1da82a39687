"""glabc_weighted_predictive_counts (csrc/glabc_weighted_predictive.hip) at every shape at which the kernel takes another path, and
predictive.check_weighted / terms_weighted / combine_weighted end to end on the GPU.

weighted_predictive_kernel<D, YD, S> cuts the draws into items of S = 16 / D consecutive 64-draw segments (16, 8, 5, 4, 3, 2, 2, 2 at
D = 1 .. 8; 4 for g-and-k), loads every theta segment and the weight segment through a descriptor of exactly its bytes, and skips a
segment in which no lane carries weight.  So the grid has every theta_dim and g-and-k; n = 1, 63, 64, 65, 64 S - 1, 64 S, 64 S + 1 and
8 x 64 S + 1 (both sides of a segment, of an item and of one workgroup's first round); a stride that is no multiple of 4 (pad 17) with
NaN in the padding columns and NaN behind the last weight (a read of either changes a table); base pointers 0 .. 3 floats into wider
buffers; ids from 0, crossing 2^32 inside a call and past 2^40; sampler-like and special-valued draws; 1, 2, 64 and 512 bins.  The
weights of a case (weights_of) hold, wherever n has room: ordinary positive weights, an exact 0 on a draw whose theta is NaN,
a negative and a NaN weight, a weight that rounds to 0, the ties w scale = 0.5, 1.5, 2.5, a weight clamped at 2^32 - 1, two draws of
multiplicity 2^31 (one bin over the whole range and thresholds of +inf put them in one bin and one tail: 32-bit counters would
wrap) and, from n = 129, a whole 64-draw segment of zero weights.  A covering grid, not a full product: test_grid_covers_every_pair.

Equal integers throughout, against (a) integer sums of m over the draws glabc_predictive_draws makes on the one-row history with the
same id0 -- the on-device composition of the parent commit's entry point --, (b) the restatement (tests/weighted_predictive_ref.py;
g-and-k draws with non-finite theta are held to (a) only: the device sorts with fmin / fmax, the checker by comparisons, and the two
order NaNs differently), and (c) with unit weights and scale 1.0 glabc_predictive_counts' three tables on the same history.  Every
table lies between guard bands of canaries and already holds something: the call adds.

Law (derived, not tuned): constant theta = 1 on |theta| + noise at d = 2, 65 536 draws, weights 1 and 3 interleaved.  Every draw's
y_j is 1 + sigma z, so P(y_j >= 1) = 1/2 whatever the weight; the weighted fraction sum m_i 1[y_ij >= 1] / M has variance
(1/4) sum m_i^2 / M^2 = 1 / (4 n_eff) with Kish's n_eff = (4 x 32 768)^2 / (10 x 32 768) = 52 428.8: standard error 0.5 / sqrt(52 428.8)
= 0.002184.  Held within 5 standard errors, the bound of the unweighted twin's law test.
"""
import collections
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import predictive_ref as P
import quantile_ref as Q
import rejection_ref as R
import weighted_predictive_ref as WP
import weighted_ref as W
from glabcmcmc_amd import distribution, predictive, weighted
from helpers import dev, host
from test_predictive_shapes import IDS, MODELS, SEED, after, history, model_of, prefilled

pytestmark = pytest.mark.gpu

ERR_NULL, ERR_DIM, ERR_KIND, ERR_ARG = -1, -2, -3, -4
PADS = (0, 17)
OFFSETS = (0, 1, 2, 3)
KINDS = ("sampler", "special")
BINS = (1, 2, 64, 512)
SCALES = (1.0, 0.5, 4.0)
WANTS = (("counts", "tails", "extremes"), ("counts",), ("tails",), ("extremes",), ("tails", "extremes"))


def segments(d):
    return 16 // d


def draw_counts(d):
    s = segments(d)
    return tuple(sorted({1, 63, 64, 65, 64 * s - 1, 64 * s, 64 * s + 1, 8 * 64 * s + 1}))


@functools.lru_cache(maxsize=None)
def cases():
    """(model key, n, pad, offset, id case, kind, bins, scale, wanted tables): one per (model, draw count); the other axes rotate
    with different periods"""
    out = []
    for mi, key in enumerate(MODELS):
        for ni, n in enumerate(draw_counts(key[1])):
            i = len(out)
            out.append((key, n, PADS[(i + i // 2) % 2], OFFSETS[(i + i // 4) % 4], (i + i // 3) % 3, KINDS[(i + i // 5) % 2],
                        BINS[(mi + ni) % 4], SCALES[(i + i // 7) % 3], WANTS[(i + i // 6) % 5]))
    return tuple(out)


def test_grid_covers_every_pair():
    rows = [c[2:] for c in cases()]
    axes = (PADS, OFFSETS, (0, 1, 2), KINDS, BINS, SCALES, WANTS)
    for a in range(len(axes)):
        assert {c[a] for c in rows} == set(axes[a]), (a, {c[a] for c in rows})
        for b in range(len(axes)):
            for v in axes[a]:
                assert a == b or len({c[b] for c in rows if c[a] == v}) >= 2, (a, v, b)
    for key in MODELS:                                             # every model meets every draw count, bin count, id case and kind
        mine = [c for c in cases() if c[0] == key]
        assert [c[1] for c in mine] == list(draw_counts(key[1])) and len(mine) in (7, 8)
        assert {c[6] for c in mine} == set(BINS) and {c[4] for c in mine} == {0, 1, 2} and {c[5] for c in mine} == set(KINDS)
        assert len({c[8] for c in mine}) >= 4 and {c[2] for c in mine} == set(PADS)
    assert any(c[0][0] == "gk" and c[6] == 512 for c in cases()) and any(c[0] == ("abs", 8) and c[6] == 512 for c in cases())      # K = 9


# ---------------------------------------------------------------------------------- the inputs of a case
@functools.lru_cache(maxsize=None)
def draws_of(key, kind, n):
    """dimension-major float32 [D][n]: the one-row history of tests/test_predictive_shapes.py, NaN where a draw will carry no weight"""
    x = np.array(history(key, kind, 1, n)[0])
    if n > 40:
        x[:, 3] = np.nan
    if n >= 129:
        x[:, 70] = np.nan
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def weights_of(n, scale):
    """float32 [n] (module docstring); what the special weights must quantise to is asserted here, once"""
    w = np.random.default_rng(7 * n + 1).uniform(0.5, 9.0, n).astype(np.float32) / np.float32(scale)
    if n > 40:
        s = np.float32(1.0 / scale)
        w[3], w[5], w[6], w[7] = 0.0, -2.0, np.nan, 0.25 * s
        w[8], w[9], w[10] = 0.5 * s, 1.5 * s, 2.5 * s
        w[11] = 2.0 ** 33 * s
        w[12] = w[37] = 2.0 ** 31 * s
        m = WP.multiplicity(w, scale)
        assert [m[i] for i in (3, 5, 6, 7, 8, 9, 10, 11, 12, 37)] == [0, 0, 0, 0, 0, 2, 2, 2 ** 32 - 1, 2 ** 31, 2 ** 31]
    if n >= 129:
        w[64:128] = 0.0                                            # a whole segment: the skip
    w.setflags(write=False)
    return w


def placed_draws(x, w, pad, offset):
    """-> (keep-alive, pointer to x, stride, pointer to w): x `offset` floats into a buffer of NaN with `pad` columns of NaN behind
    every coordinate, w (offset + 1) % 4 floats into a buffer of NaN with NaN behind its last element"""
    d, n = x.shape
    body = np.full((d, n + pad), np.nan, np.float32)
    body[:, :n] = x
    flat = np.full(offset + body.size + 5, np.nan, np.float32)
    flat[offset:offset + body.size] = body.reshape(-1)
    w_off = (offset + 1) % 4
    wflat = np.full(w_off + n + 70, np.nan, np.float32)
    wflat[w_off:w_off + n] = w
    tx, tw = dev(flat), dev(wflat)
    return (tx, tw), tx.data_ptr() + 4 * offset, n + pad, tw.data_ptr() + 4 * w_off


def device_statistics(hip, model, ptr, stride, n, id0):
    """(a): float32 [n][K] of the draws glabc_predictive_draws makes on the one-row history [1][D][stride] with n_chains = n"""
    yd = model.y_dim
    y, dis = torch.empty(yd, n, device="cuda"), torch.empty(n, device="cuda")
    assert hip.glabc_predictive_draws(C.byref(model), ptr, 1, model.theta_dim, n, stride, SEED, id0, n, y.data_ptr(), n, dis.data_ptr(), n, None) == 0
    return np.ascontiguousarray(np.concatenate([host(y), host(dis)[None]]).T)


def axes_of(stats, m):
    """a range and thresholds made of counted values: the closed last bin and the "equal" tail are met"""
    k = stats.shape[1]
    keep = np.array([c > 0 for c in m], bool)
    lo, hi, thr = np.zeros(k), np.ones(k), np.zeros(k, np.float32)
    for j in range(k):
        v = np.sort(stats[keep, j][np.isfinite(stats[keep, j])])
        if v.size:
            lo[j], hi[j], thr[j] = float(v[v.size // 10]), float(v[9 * v.size // 10]), v[v.size // 2]
        if not lo[j] < hi[j]:                                      # one value: a bin around it, wide enough to be one in float64
            half = max(0.5, 0.25 * abs(lo[j]))
            lo[j], hi[j] = lo[j] - half, lo[j] + half
    return lo, hi, thr


def call(hip, model, ptr, stride, wptr, n, scale, id0, n_bins, lo, hi, thr, want=WANTS[0], tables=None, expect=0, fn=None):
    """one glabc_weighted_predictive_counts call -> ({name: what the call added (counts, tails) or left (extremes)}, the tables);
    `tables`: accumulate into these instead of fresh ones.  fn: another entry point with the same arguments behind its head"""
    k = model.y_dim + 1
    sizes = {"counts": k * (n_bins + 3), "tails": 4 * k, "extremes": 2 * k}
    if tables is None:
        tables = {"counts": prefilled(sizes["counts"]), "tails": prefilled(sizes["tails"]),
                  "extremes": prefilled(sizes["extremes"], np.uint32, np.tile(np.array(P.KEY_NONE, np.uint32), k))}
    lo = None if lo is None else np.ascontiguousarray(lo, np.float64)
    hi = None if hi is None else np.ascontiguousarray(hi, np.float64)
    thr = None if thr is None else np.ascontiguousarray(thr, np.float32)
    p = lambda a: None if a is None else a.ctypes.data          # noqa: E731
    q = lambda name: tables[name][1] if name in want else None   # noqa: E731
    fn = (lambda *a: hip.glabc_weighted_predictive_counts(C.byref(model), *a)) if fn is None else fn
    rc = fn(ptr, stride, model.theta_dim, wptr, n, scale, SEED, id0, n_bins, p(lo) if "counts" in want else None,
            p(hi) if "counts" in want else None, p(thr) if "tails" in want else None, q("counts"), q("tails"), q("extremes"), None)
    torch.cuda.synchronize()
    assert rc == expect, rc
    out = {}
    for name in ("counts", "tails", "extremes"):
        t, _, before = tables[name]
        now = after(t, sizes[name], np.uint32 if name == "extremes" else np.uint64)
        if name in want and rc == 0:
            out[name] = (now.copy() if name == "extremes" else now - before).reshape(k, -1)
        else:
            assert np.array_equal(now, before), "%s was written by a call that must not" % name
    return out, tables


def reference(stats, m, n_bins, lo, hi, thr):
    return {"counts": WP.as_u64(WP.counts(stats, m, n_bins, lo, hi)), "tails": WP.as_u64(WP.tails(stats, m, thr)),
            "extremes": WP.extremes(stats, m)}


def same_bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------------------------- the covering grid
@pytest.mark.parametrize("key", MODELS, ids=lambda k: "%s%d" % k)
def test_tables_equal_the_composition_the_restatement_and_the_unweighted_twin(hip, key):
    model = model_of(key)
    k = model.y_dim + 1
    seen = collections.Counter()
    for _, n, pad, offset, idc, kind, n_bins, scale, want in (c for c in cases() if c[0] == key):
        where = (key, n, pad, offset, idc, kind, n_bins, scale, want)
        id0 = IDS[idc][0]
        x, w = draws_of(key, kind, n), weights_of(n, scale)
        keep, ptr, stride, wptr = placed_draws(x, w, pad, offset)
        m = WP.multiplicity(w, scale)
        # (a) the draws of the parent commit's entry point, weighted on the host
        stats = device_statistics(hip, model, ptr, stride, n, id0)
        lo, hi, thr = axes_of(stats, m)
        ref = reference(stats, m, n_bins, lo, hi, thr)
        got, _ = call(hip, model, ptr, stride, wptr, n, scale, id0, n_bins, lo, hi, thr, want=want)
        assert set(got) == set(want)
        for name in want:
            assert np.array_equal(got[name], ref[name]), ("composition", name, where, np.argwhere(got[name] != ref[name])[:4])
        if "counts" in want:
            assert (got["counts"].sum(axis=1) == sum(m)).all(), where
        if "tails" in want:
            assert (got["tails"].sum(axis=1) == sum(m)).all(), where
            if n > 40 and kind == "sampler":
                assert got["tails"][:, 1].all(), where              # a threshold that is a counted value
        # (b) the restatement from the CPU checker's functions
        if key[0] != "gk" or kind == "sampler":
            restated = WP.statistics(model, x, n, SEED, id0)
            counted = np.array([c > 0 for c in m], bool)
            assert same_bits(restated[counted], stats[counted]), ("restated draws", where)
            again = reference(restated, m, n_bins, lo, hi, thr)
            for name in want:
                assert np.array_equal(got[name], again[name]), ("restatement", name, where)
        if n > 40:
            # the uint32-wrap detector: one bin over the whole range, every threshold +inf -- the two draws of multiplicity 2^31 meet
            # in one bin or one outside slot and, where finite, in one tail
            whole_lo, whole_hi = np.full(k, -3.0e38), np.full(k, 3.0e38)
            inf = np.full(k, np.inf, np.float32)
            one, _ = call(hip, model, ptr, stride, wptr, n, scale, id0, 1, whole_lo, whole_hi, inf, want=("counts", "tails"))
            ref1 = reference(stats, m, 1, whole_lo, whole_hi, inf)
            assert np.array_equal(one["counts"], ref1["counts"]) and np.array_equal(one["tails"], ref1["tails"]), ("one bin", where)
            if kind == "sampler":                                  # both are finite
                assert (one["counts"][:, 0] >= 2 ** 32).all() and (one["tails"][:, 0] >= 2 ** 32).all(), where
            # a draw of no weight whose theta is NaN is in no slot and no tail: the NaN counts are the counted draws' alone
            nan_m = [sum(c for c, v in zip(m, stats[:, j]) if np.isnan(v)) for j in range(k)]
            assert one["counts"][:, 3].tolist() == nan_m == one["tails"][:, 3].tolist(), where
            if kind == "sampler":
                assert not any(nan_m) and np.isnan(stats[3]).all(), where
        # (c) unit weights and scale 1.0: the unweighted twin's tables on the same history
        ones = dev(np.concatenate([np.ones(n, np.float32), np.full(3, np.nan, np.float32)]))
        unit, _ = call(hip, model, ptr, stride, ones.data_ptr(), n, 1.0, id0, n_bins, lo, hi, thr)
        twin, _ = call(hip, model, ptr, stride, None, None, None, id0, n_bins, lo, hi, thr,
                       fn=lambda x_, stride_, d_, w_, n_, scale_, seed_, id0_, *rest: hip.glabc_predictive_counts(
                           C.byref(model), x_, 1, d_, n, stride_, seed_, id0_, n, *rest))
        for name in WANTS[0]:
            assert np.array_equal(unit[name], twin[name]), ("unit weights", name, where)
        assert (unit["tails"].sum(axis=1) == n).all()
        seen[n] += 1
    assert sorted(seen) == list(draw_counts(key[1]))


@pytest.mark.parametrize("key", [("abs", 1), ("abs", 3), ("abs", 8), ("gk", 4)], ids=lambda k: "%s%d" % k)
def test_slices_of_draws_add_up_to_the_one_shot_tables(hip, key):
    model = model_of(key)
    s = segments(key[1])
    n, scale, id0 = 2 * 64 * s + 10, 0.5, 2 ** 32 - 40
    x, w = draws_of(key, "sampler", n), weights_of(n, scale)
    keep, ptr, stride, wptr = placed_draws(x, w, 17, 1)
    m = WP.multiplicity(w, scale)
    stats = device_statistics(hip, model, ptr, stride, n, id0)
    lo, hi, thr = axes_of(stats, m)
    whole, _ = call(hip, model, ptr, stride, wptr, n, scale, id0, 7, lo, hi, thr)
    for a in (37, 64 * s):                                         # inside a segment, on an item's edge
        tables, total = None, None
        for first, count in ((0, a), (a, n - a)):
            total, tables = call(hip, model, ptr + 4 * first, stride, wptr + 4 * first, count, scale, id0 + first, 7, lo, hi, thr, tables=tables)
        for name in WANTS[0]:
            assert np.array_equal(total[name], whole[name]), (key, a, name)
    # other ids give other draws: the tables are a function of id0
    other, _ = call(hip, model, ptr, stride, wptr, n, scale, id0 + 1, 7, lo, hi, thr)
    assert not np.array_equal(other["counts"], whole["counts"])


def test_refused_calls_write_nothing_and_no_draws_is_ok(hip):
    key = ("abs", 3)
    model = model_of(key)
    x, w = draws_of(key, "sampler", 70), weights_of(70, 1.0)
    keep, ptr, stride, wptr = placed_draws(x, w, 0, 0)
    lo, hi, thr = np.zeros(4), np.ones(4), np.zeros(4, np.float32)
    base = dict(ptr=ptr, stride=70, wptr=wptr, n=70, scale=1.0, id0=0, n_bins=7, lo=lo, hi=hi, thr=thr)
    for rc, kw in ((ERR_NULL, dict(ptr=None)), (ERR_NULL, dict(wptr=None)), (ERR_NULL, dict(want=())), (ERR_ARG, dict(n=-1)), (ERR_ARG, dict(stride=69)),
                   (ERR_ARG, dict(scale=0.0)), (ERR_ARG, dict(scale=float("nan"))), (ERR_ARG, dict(id0=-1)), (ERR_ARG, dict(id0=2 ** 63 - 60)),
                   (ERR_ARG, dict(n_bins=0)), (ERR_ARG, dict(n_bins=513)), (ERR_ARG, dict(hi=lo)),
                   (ERR_ARG, dict(thr=np.array([0, 0, np.nan, 0], np.float32))), (0, dict(n=0)), (0, dict(n=0, stride=0))):
        a = dict(base)
        a.update(kw)
        want = a.pop("want", WANTS[0])
        got, _ = call(hip, model, a["ptr"], a["stride"], a["wptr"], a["n"], a["scale"], a["id0"], a["n_bins"], a["lo"], a["hi"], a["thr"], want=want,
                      expect=rc)
        if rc == 0:                                                # no draws: nothing added, the extremes as they were
            assert not got["counts"].any() and not got["tails"].any()
            assert np.array_equal(got["extremes"], np.tile(np.array(P.KEY_NONE, np.uint32), (4, 1)))
    # nothing but weightless draws: a launch that adds nothing
    zero = dev(np.zeros(70, np.float32))
    got, _ = call(hip, model, ptr, 70, zero.data_ptr(), 70, 1.0, 0, 7, lo, hi, thr)
    assert not got["counts"].any() and not got["tails"].any() and np.array_equal(got["extremes"], np.tile(np.array(P.KEY_NONE, np.uint32), (4, 1)))


# ---------------------------------------------------------------------------------- predictive.py end to end
Population = collections.namedtuple("Population", "theta weights epsilon")
Rejection = collections.namedtuple("Rejection", "theta y distance")


def test_check_weighted_end_to_end(hip):
    key = ("abs", 3)
    Model = R.abs_gauss_model(3, distribution.DiagGaussian(3, torch.zeros(3), torch.zeros(3)), epsilon=1.3)
    desc = Model.descriptor()
    n = 150
    rng = np.random.default_rng(21)
    x = np.array(history(key, "sampler", 1, n)[0])
    w = rng.uniform(0.5, 9.0, n).astype(np.float32)
    x[:, 4], w[4] = np.nan, 0.0
    w[64:128] = 0.0
    theta = dev(np.ascontiguousarray(x.T))                                               # (n, D)
    thr = np.array([1.5, 1.4, 1.3, 1.3], np.float32)                                     # the defaults: y_obs and epsilon
    scale = weighted.quantize(torch.from_numpy(w))[1]
    assert scale == W.default_scale(w)
    m = WP.multiplicity(w, scale)
    total = sum(m)
    for draw0 in (0, 2 ** 40 + 5):
        stats = WP.statistics(desc, x, n, 77, draw0)
        e = WP.extremes(stats, m)
        lim = np.stack([Q.unkey(e[:, 0]), Q.unkey(e[:, 1])], axis=1).astype(np.float64)
        c = predictive.check_weighted(Model, Population(theta, dev(w), 1.3), bins=7, seed=77, draw0=draw0)          # range=None: two passes
        assert c.n == total and isinstance(c.n, int)
        assert np.array_equal(c.y_edges[:, 0], lim[:3, 0]) and np.array_equal(c.y_edges[:, -1], lim[:3, 1])
        assert c.distance_edges[0] == lim[3, 0] and c.distance_edges[-1] == lim[3, 1]
        want = WP.as_u64(WP.counts(stats, m, 7, lim[:, 0], lim[:, 1]))
        tails = WP.tails(stats, m, thr)
        assert np.array_equal(c.y_counts, want[:3, :7]) and np.array_equal(c.distance_counts, want[3, :7])
        assert not c.y_outside.any() and not c.distance_outside.any() and np.array_equal(c.tails, WP.as_u64(tails))
        for j in range(3):
            assert c.p_upper[j] == (tails[j][1] + tails[j][2]) / total
        assert c.within_epsilon == (tails[3][0] + tails[3][1]) / total
        again = predictive.check_weighted(Model, (theta, dev(w)), bins=7, range=lim, seed=77, draw0=draw0, scale=scale, path="fused")
        for got, ref in zip(again, c):
            assert np.array_equal(got, ref)
        # predictive.simulate with row0 = draw0 materialises the very draws
        y_rep, distance = predictive.simulate(Model, theta, seed=77, row0=draw0)
        assert same_bits(host(y_rep), stats[:, :3]) and same_bits(host(distance), stats[:, 3])
    # three ragged shards with draw0 are the one-shot tables exactly
    lim = np.array([[0.0, 4.0], [0.0, 4.0], [-1.0, 3.0], [0.0, 6.0]])
    whole = predictive.terms_weighted(Model, (theta, dev(w)), bins=7, range=lim, seed=77, scale=scale, draw0=11)
    parts = [predictive.terms_weighted(Model, (theta[a:b], dev(w[a:b])), bins=7, range=lim, seed=77, scale=scale, draw0=11 + a)
             for a, b in ((0, 37), (37, 128), (128, 150))]
    assert parts[1].n_draws == 91 and parts[1].n > 0
    both = predictive.combine_weighted(parts)
    assert both.n == whole.n == total and both.n_draws == 150 and np.array_equal(both.counts, whole.counts) and np.array_equal(both.tails, whole.tails)
    stats = WP.statistics(desc, x, n, 77, 11)
    assert np.array_equal(whole.counts, WP.as_u64(WP.counts(stats, m, 7, lim[:, 0], lim[:, 1])))
    # unit weights: a pair with None and a Rejection equal check on the (T, D) history, draw for draw
    ok = np.ones(n, bool)
    ok[4] = False
    kept = dev(np.ascontiguousarray(x.T[ok]))
    plain = predictive.check(Model, kept, bins=7, range=lim, seed=77)
    for draws in ((kept, None), Rejection(kept, None, None)):
        unit = predictive.check_weighted(Model, draws, bins=7, range=lim, seed=77, scale=1.0)
        assert unit.n == 149
        for got, ref in zip(unit, plain):
            assert np.array_equal(got, ref)
    # a constant statistic is widened by +-0.5; one draw
    single = predictive.check_weighted(Model, (kept[:1], None), bins=4, seed=77)
    assert np.allclose(single.y_edges[:, -1] - single.y_edges[:, 0], 1.0) and (single.y_counts.sum(axis=1) == single.n).all() and single.n == 2 ** 31
    # the generic route on CPU tensors: other noise, the same integers' totals; the fused route refuses what it cannot run
    g = predictive.check_weighted(Model, (theta.cpu(), torch.from_numpy(w)), bins=7, range=lim, seed=77, path="generic")
    assert g.n == total and (g.tails.sum(axis=1) == total).all()

    class Callback:
        theta_dim, y_dim, epsilon, y_obs = 3, 3, 1.0, torch.zeros(1, 3)

        def generate_samples(self, t, num_samples=1):
            return t.view(-1, 3) + torch.randn(t.view(-1, 3).shape)

    with pytest.raises(ValueError):
        predictive.check_weighted(Callback(), (theta.cpu(), None), seed=1, path="fused")
    with pytest.raises(ValueError):                                                      # nothing but NaN carries weight: no range
        predictive.check_weighted(Model, (torch.full((4, 3), float("nan"), device="cuda"), None), seed=1)


def test_gk_check_weighted_runs_on_the_kernel(hip):
    from glabcmcmc_amd.examples.GK import GK_set
    Model = GK_set(200.0)
    x = np.array(history(("gk", 4), "sampler", 1, 300)[0])
    w = np.random.default_rng(5).uniform(0.0, 1.0, 300).astype(np.float32)
    scale = W.default_scale(w)
    m = WP.multiplicity(w, scale)
    stats = WP.statistics(Model.descriptor(), x, 300, 9, 0)
    e = WP.extremes(stats, m)
    lim = np.stack([Q.unkey(e[:, 0]), Q.unkey(e[:, 1])], axis=1).astype(np.float64)
    c = predictive.check_weighted(Model, (dev(np.ascontiguousarray(x.T)), dev(w)), bins=512, seed=9)
    want = WP.as_u64(WP.counts(stats, m, 512, lim[:, 0], lim[:, 1]))
    assert c.y_counts.shape == (8, 512) and np.array_equal(c.y_counts, want[:8, :512]) and np.array_equal(c.distance_counts, want[8, :512])
    assert c.n == sum(m) > 2 ** 32


# ---------------------------------------------------------------------------------- the law of the weighted check
def test_law_of_the_weighted_p_values(hip):
    Model = R.abs_gauss_model(2, distribution.DiagGaussian(2, torch.zeros(2), torch.zeros(2)), epsilon=0.3, y_obs=[1.5, 1.5])
    n = 65536
    theta = torch.ones(n, 2, device="cuda")
    w = torch.ones(n, device="cuda")
    w[1::2] = 3.0
    n_eff = (4 * 32768) ** 2 / (10 * 32768)
    assert n_eff == 52428.8
    se = 0.5 / math.sqrt(n_eff)
    c = predictive.check_weighted(Model, (theta, w), bins=1, range=[(0.0, 2.0), (0.0, 2.0), (0.0, 10.0)], thresholds=[1.0, 1.0, 0.3], seed=2026,
                                  scale=1.0)
    assert c.n == 4 * 32768 and (c.tails.sum(axis=1) == c.n).all() and not c.tails[:, 3].any()
    print("weighted p_upper %r (0.5 +- %.6f)" % (c.p_upper.tolist(), se))
    assert (np.abs(c.p_upper - 0.5) <= 5 * se).all()
