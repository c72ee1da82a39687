"""glabc_predictive_draws and glabc_predictive_counts (csrc/glabc_predictive.hip) at every shape at which the kernel takes another
path, and glabcmcmc_amd/predictive.py end to end.

predictive_kernel<D, YD> cuts the history into items of 64 chains x R rows, R = 16 / D (16, 8, 5, 4, 3, 2, 2, 2 at D = 1 .. 8; 4 for
g-and-k), loads every row segment through a descriptor of exactly its bytes and makes one draw per lane and row.  So the grid has
every theta_dim and g-and-k, chains on both sides of 64 and more than one segment, rows 1, 2 and both sides of R and of 2 R, a
stride that is no multiple of 4 (pad 17) with NaN in the padding columns (a read of one changes a draw), a base pointer 0 .. 3
floats into a wider buffer, ids that cross 2^32 inside a call and lie past 2^40, and id_step > n_chains.  The cases are a covering
grid, not a full product: test_grid_covers_every_pair checks that every value of an axis meets two values of every other axis.

Bit for bit: the draws against (a) the on-device composition of the parent commit's entry points, row by row -- transpose ->
glabc_model_simulate(eps = NULL, seed ^ GLABC_PREDICTIVE_KEY, row0 = id0 + t id_step) -> glabc_model_discrepancy -- and (b) the
restatement from the CPU checker's functions (tests/predictive_ref.py); "equal bits" lets a NaN match a NaN of another payload.
g-and-k histories with non-finite rows are held to (a) only: the device sorts with fmin / fmax, the checker by comparisons, and the
two order NaNs differently.  Counts, tails and extremes: equal integers.  Every output lies between guard bands of canaries and the
padding columns of y_out / dis_out keep theirs.

Law (derived, not tuned): a constant history theta = 1 on |theta| + noise at d = 2, 1024 chains x 64 rows, N = 65 536 independent
draws y_j = 1 + sigma z.  P(y_j >= 1) = 1/2, binomial standard error 0.5 / 256; the mass of [1 - sigma, 1 + sigma] is
erf(1 / sqrt 2) = 0.6827, standard error sqrt(0.6827 x 0.3173 / 65 536); both within 5 standard errors.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import predictive_ref as P
import quantile_ref as Q
import rejection_ref as R
from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import diagnostics, distribution, predictive
from helpers import assert_untouched, bits, canary_f32, canary_left, dev, host

pytestmark = pytest.mark.gpu

ERR_NULL, ERR_DIM, ERR_KIND, ERR_ARG = -1, -2, -3, -4
SEED = 0x123456789ABCDEF1                  # both key words in use
KEY = SEED ^ P.PREDICTIVE_KEY
GUARD = 64
MODELS = [("abs", d) for d in range(1, 9)] + [("gk", 4)]
CHAINS = (1, 3, 63, 64, 65, 321)
PADS = (0, 17)
OFFSETS = (0, 1, 2, 3)
IDS = ((0, 0), (2 ** 32 - 40, 0), (2 ** 40 + 5, 7))          # (id0, id_step - n_chains): the second crosses the counter's low word inside a call
KINDS = ("sampler", "special")
U64_CANARY = np.uint64(0xDEADC0DEDEADBEEF)


def rows_per_item(d):
    return 16 // d


def row_counts(d):
    r = rows_per_item(d)
    return tuple(sorted({1, 2, max(r - 1, 1), r, r + 1, 2 * r + 1}))


@functools.lru_cache(maxsize=None)
def model_of(key):
    kind, d = key
    if kind == "gk":
        from glabcmcmc_amd.examples.GK import GK_set
        return GK_set(200.0).descriptor()
    prior = distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d))
    return R.abs_gauss_model(d, prior, epsilon=0.4 + 0.3 * d).descriptor()


@functools.lru_cache(maxsize=None)
def cases():
    """(model key, n_rows, n_chains, pad, offset, id case, kind): two per (model, row count), rotations of different periods"""
    out = []
    for mi, key in enumerate(MODELS):
        for ri, n_rows in enumerate(row_counts(key[1])):
            for s in (0, 1):
                i = len(out)
                out.append((key, n_rows, CHAINS[(mi + ri + 3 * s + i // 12) % 6], PADS[(i + i // 2) % 2], OFFSETS[(i + i // 4) % 4],
                            (i + i // 3) % 3, KINDS[(i + i // 5) % 2]))
    return tuple(out)


def test_grid_covers_every_pair():
    rows = [(c[2], c[3], c[4], c[5], c[6]) for c in cases()]
    axes = (CHAINS, PADS, OFFSETS, (0, 1, 2), KINDS)
    for a in range(len(axes)):
        assert {c[a] for c in rows} == set(axes[a]), (a, {c[a] for c in rows})
        for b in range(len(axes)):
            for v in axes[a]:
                assert a == b or len({c[b] for c in rows if c[a] == v}) >= 2, (a, v, b)
    for key in MODELS:                                             # every model meets every row count, both kinds and all id cases
        mine = [c for c in cases() if c[0] == key]
        assert {c[1] for c in mine} == set(row_counts(key[1])) and {c[6] for c in mine} == set(KINDS) and {c[5] for c in mine} == {0, 1, 2}
        r = rows_per_item(key[1])
        assert {r, r + 1} <= {c[1] for c in mine} and len({c[2] for c in mine}) >= 4


@functools.lru_cache(maxsize=None)
def history(key, kind, n_rows, n):
    """chain-major float32 [n_rows][D][n]: sampler-like values, or the special values of quantile_ref (NaN, +-inf, +-0, denormals)"""
    d = key[1]
    rng = np.random.default_rng(1000 * n_rows + n + d)
    if kind == "special":
        h = np.array(Q.special_history(n_rows, d, n))
    elif key[0] == "gk":
        h = (np.array([3.0, 1.0, 2.0, 0.5], np.float32)[None, :, None] +
             np.array([0.5, 0.2, 0.3, 0.1], np.float32)[None, :, None] * rng.standard_normal((n_rows, 4, n)).astype(np.float32))
        h[:, 1] = np.abs(h[:, 1])
    else:
        h = (1.5 * rng.standard_normal((n_rows, d, n))).astype(np.float32)
    h.setflags(write=False)
    return h


def placed(hist, pad, offset):
    """-> (device buffer, pointer to the history, stride): the history `offset` floats into a buffer of NaN, `pad` columns of NaN
    behind every row segment"""
    n_rows, d, n = hist.shape
    body = np.full((n_rows, d, n + pad), np.nan, np.float32)
    body[:, :, :n] = hist
    flat = np.full(offset + body.size + 5, np.nan, np.float32)
    flat[offset:offset + body.size] = body.reshape(-1)
    t = dev(flat)
    return t, t.data_ptr() + 4 * offset, n + pad


class Guarded:
    """a device buffer of `rows` x `stride` float32 between two guard bands, all canaries"""

    def __init__(self, rows, stride):
        self.rows, self.stride = rows, stride
        self.t = dev(canary_f32(2 * GUARD + rows * stride))
        self.ptr = self.t.data_ptr() + 4 * GUARD

    def read(self, n):
        """-> [rows][n] written by the call; the guard bands and columns n .. stride - 1 must hold their canaries"""
        h = host(self.t)
        body = h[GUARD:len(h) - GUARD].reshape(self.rows, self.stride)
        assert_untouched(h[:GUARD], h[len(h) - GUARD:], body[:, n:])
        assert canary_left(body[:, :n]) == 0, "an element the call owns was never written"
        return body[:, :n]

    def untouched(self):
        assert_untouched(host(self.t))


def same(a, b):
    """equal bits, a NaN matching a NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def hip_draws(hip, model, hist, pad, offset, id0, id_step, want=("y", "dis"), expect=0):
    n_rows, d, n = hist.shape
    buf, ptr, stride = placed(hist, pad, offset)
    yd = model.y_dim
    y, dis = Guarded(n_rows * yd, n + 3), Guarded(n_rows, n + 2)
    rc = hip.glabc_predictive_draws(C.byref(model), ptr, n_rows, d, n, stride, SEED, id0, id_step, y.ptr if "y" in want else None, n + 3,
                                    dis.ptr if "dis" in want else None, n + 2, None)
    torch.cuda.synchronize()
    assert rc == expect, rc
    out = {}
    for name, b in (("y", y), ("dis", dis)):
        if name in want and rc == 0:
            out[name] = b.read(n).reshape((n_rows, yd, n) if name == "y" else (n_rows, n)).copy()
        else:
            b.untouched()
    return out


def composed(hip, model, hist, id0, id_step):
    """the twin: the parent commit's entry points row by row, theta and y through device memory"""
    n_rows, d, n = hist.shape
    ys, ds = [], []
    for t in range(n_rows):
        theta = dev(np.ascontiguousarray(hist[t].T))
        y, dis = torch.empty(n, model.y_dim, device="cuda"), torch.empty(n, device="cuda")
        assert hip.glabc_model_simulate(C.byref(model), theta.data_ptr(), None, n, KEY, id0 + t * id_step, y.data_ptr(), None) == 0
        assert hip.glabc_model_discrepancy(C.byref(model), y.data_ptr(), n, dis.data_ptr(), None) == 0
        ys.append(host(y).T)
        ds.append(host(dis))
    return np.stack(ys), np.stack(ds)


# ---------------------------------------------------------------------------------- glabc_predictive_draws
@pytest.mark.parametrize("key", MODELS, ids=lambda k: "%s%d" % k)
def test_draws_equal_the_composition_and_the_restatement(hip, key):
    model = model_of(key)
    n_cases = 0
    for _, n_rows, n, pad, offset, idc, kind in (c for c in cases() if c[0] == key):
        hist = history(key, kind, n_rows, n)
        id0, id_step = IDS[idc][0], n + IDS[idc][1]
        where = (key, n_rows, n, pad, offset, id0, id_step, kind)
        got = hip_draws(hip, model, hist, pad, offset, id0, id_step)
        y, dis = composed(hip, model, hist, id0, id_step)
        assert same(got["y"], y) and same(got["dis"], dis), ("composition", where)
        if key[0] != "gk" or kind == "sampler":
            y, dis = P.restate(model, hist, n, SEED, id0, id_step)
            assert same(got["y"], y) and same(got["dis"], dis), ("restatement", where)
        if kind == "special" and key[0] == "abs" and n_rows * n > 60:
            assert np.isnan(got["dis"]).any() and np.isfinite(got["dis"]).any(), where
        n_cases += 1
    assert n_cases == 2 * len(row_counts(key[1]))


@pytest.mark.parametrize("key", [("abs", 2), ("abs", 5), ("gk", 4)], ids=lambda k: "%s%d" % k)
def test_each_draws_output_alone_and_slabs_address_the_same_draws(hip, key):
    model = model_of(key)
    r = rows_per_item(key[1])
    hist = history(key, "sampler", 2 * r + 1, 65)
    whole = hip_draws(hip, model, hist, 17, 1, 2 ** 32 - 40, 70)
    assert same(hip_draws(hip, model, hist, 17, 1, 2 ** 32 - 40, 70, want=("y",))["y"], whole["y"])
    assert same(hip_draws(hip, model, hist, 0, 3, 2 ** 32 - 40, 70, want=("dis",))["dis"], whole["dis"])
    # a slab of chains from a slice of rows, with the matching id0: the very draws of the whole
    part = hip_draws(hip, model, np.ascontiguousarray(hist[r:, :, 10:]), 0, 2, 2 ** 32 - 40 + r * 70 + 10, 70)
    assert same(part["y"], whole["y"][r:, :, 10:]) and same(part["dis"], whole["dis"][r:, 10:])
    # ... and other ids, or another seed, give other draws
    other = hip_draws(hip, model, hist, 0, 0, 2 ** 32 - 39, 70)
    assert not same(other["dis"], whole["dis"])


# ---------------------------------------------------------------------------------- glabc_predictive_counts
def prefilled(size, dtype=np.uint64, fill=None):
    """a table that already holds something, between guard bands -> (device tensor, pointer, what it holds)"""
    if fill is None:
        before = ((np.arange(size, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1000)) + np.uint64(1)).astype(dtype)
    else:
        before = np.asarray(fill, dtype).reshape(-1)
    canary = np.full(8, U64_CANARY).view(dtype)
    buf = np.concatenate([canary, before, canary])
    t = dev(buf.view(np.int64 if dtype == np.uint64 else np.int32))
    return t, t.data_ptr() + canary.nbytes, before


def after(t, size, dtype=np.uint64):
    a = host(t).view(dtype)
    g = 8 * 8 // np.dtype(dtype).itemsize
    assert (a[:g].view(np.uint64) == U64_CANARY).all() and (a[g + size:].view(np.uint64) == U64_CANARY).all(), "guard bands written"
    return a[g:g + size]


def hip_counts(hip, model, ptr, n_rows, n, stride, id0, id_step, n_bins, lo, hi, thr, want=("counts", "tails", "extremes"), tables=None,
               expect=0):
    """one glabc_predictive_counts call -> {name: what the call added (counts, tails) or left (extremes)}; `tables`: accumulate into
    these instead of fresh ones"""
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
    rc = hip.glabc_predictive_counts(C.byref(model), ptr, n_rows, model.theta_dim, n, stride, SEED, id0, id_step, n_bins, p(lo), p(hi), p(thr),
                                     q("counts"), q("tails"), q("extremes"), None)
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


@functools.lru_cache(maxsize=None)
def counts_reference(key):
    """a ragged shape of several items per wavefront with non-finite draws, its restated statistics and a range and thresholds made
    of restated values: computed once, never modified"""
    model = model_of(key)
    r = rows_per_item(key[1])
    hist = np.array(history(key, "sampler", 4 * r + 1, 321))
    hist[1, :, 5], hist[2 * r, :, 300] = np.nan, np.nan            # every y of these draws is a NaN, however g-and-k sorts them
    if key[0] == "abs":
        hist[0, 0, 70], hist[3, key[1] - 1, 64] = np.inf, -np.inf
    stats = P.statistics(*P.restate(model, hist, 321, SEED, 2 ** 32 - 40, 328))
    finite = [np.sort(x[np.isfinite(x)]) for x in stats]
    lo = np.array([float(s[len(s) // 10]) for s in finite])
    hi = np.array([float(s[9 * len(s) // 10]) for s in finite])      # a restated value: the closed last bin
    thr = np.array([s[len(s) // 2] for s in finite], np.float32)     # a restated value: the "equal" slot
    for a in (hist, stats, lo, hi, thr):
        a.setflags(write=False)
    return hist, stats, lo, hi, thr


@pytest.mark.parametrize("key", [("abs", 1), ("abs", 2), ("abs", 3), ("abs", 8), ("gk", 4)], ids=lambda k: "%s%d" % k)
def test_counts_tails_and_extremes_equal_the_restatement(hip, key):
    model = model_of(key)
    hist, stats, lo, hi, thr = counts_reference(key)
    n_rows, _, n = hist.shape
    buf, ptr, stride = placed(hist, 17, 3)
    want_tails, want_extremes = P.tails(stats, thr), P.extremes(stats)
    assert want_tails[:, 1].all() and want_tails[:, 3].all() and (want_tails.sum(axis=1) == n_rows * n).all()
    for n_bins in (1, 2, 7, 1024):
        got, _ = hip_counts(hip, model, ptr, n_rows, n, stride, 2 ** 32 - 40, 328, n_bins, lo, hi, thr)
        want = P.counts(stats, n_bins, lo, hi)
        assert np.array_equal(got["counts"], want), (key, n_bins, np.argwhere(got["counts"] != want)[:4])
        assert want[:, n_bins].all() and want[:, n_bins + 1].all() and want[:, n_bins + 2].all() and want[:, n_bins - 1].all()
        assert np.array_equal(got["tails"], want_tails) and np.array_equal(got["extremes"], want_extremes), (key, n_bins)
    for want in (("counts",), ("tails",), ("extremes",), ("counts", "extremes")):          # each output alone, what only the others read NULL
        got, _ = hip_counts(hip, model, ptr, n_rows, n, stride, 2 ** 32 - 40, 328, 7, lo if "counts" in want else None,
                            hi if "counts" in want else None, thr if "tails" in want else None, want=want)
        assert set(got) == set(want)
        for name, ref in (("counts", P.counts(stats, 7, lo, hi)), ("tails", want_tails), ("extremes", want_extremes)):
            assert name not in got or np.array_equal(got[name], ref), (key, want, name)


def test_counts_of_the_draws_entry_point_and_nothing_but_nan(hip):
    """the counted draws are glabc_predictive_draws' (binned by the restatement), and a history of NaN leaves the extremes as they were"""
    key = ("abs", 3)
    model = model_of(key)
    hist = history(key, "special", 11, 65)
    d = hip_draws(hip, model, hist, 0, 0, 5, 65)
    stats = P.statistics(d["y"], d["dis"])
    buf, ptr, stride = placed(hist, 17, 2)
    lo, hi, thr = np.full(4, -1.0), np.full(4, 2.5), np.full(4, 2.5, np.float32)
    got, _ = hip_counts(hip, model, ptr, 11, 65, stride, 5, 65, 7, lo, hi, thr)
    assert np.array_equal(got["counts"], P.counts(stats, 7, lo, hi)) and np.array_equal(got["tails"], P.tails(stats, thr))
    assert np.array_equal(got["extremes"], P.extremes(stats)) and got["counts"][:, 9].all()
    nan = np.full((3, 3, 70), np.nan, np.float32)
    buf, ptr, stride = placed(nan, 0, 0)
    got, _ = hip_counts(hip, model, ptr, 3, 70, stride, 0, 70, 2, lo, hi, thr)
    assert (got["counts"][:, 4] == 210).all() and (got["tails"][:, 3] == 210).all() and got["counts"].sum() == 840 == got["tails"].sum()
    assert np.array_equal(got["extremes"], np.tile(np.array(P.KEY_NONE, np.uint32), (4, 1)))


def test_tables_add_over_slabs_of_chains_and_slices_of_rows(hip):
    key = ("abs", 3)
    model = model_of(key)
    hist, stats, lo, hi, thr = counts_reference(key)
    n_rows, d, n = hist.shape
    buf, ptr, stride = placed(hist, 17, 1)
    id0, step = 2 ** 32 - 40, 328
    whole, _ = hip_counts(hip, model, ptr, n_rows, n, stride, id0, step, 7, lo, hi, thr)
    assert np.array_equal(whole["counts"], P.counts(stats, 7, lo, hi))
    tables, total = None, None
    for row0, rows in ((0, 8), (8, n_rows - 8)):
        for chain0, k in ((0, 130), (130, n - 130)):
            got, tables = hip_counts(hip, model, ptr + 4 * (row0 * d * stride + chain0), rows, k, stride, id0 + row0 * step + chain0, step, 7,
                                     lo, hi, thr, tables=tables)
            total = got                                             # what the table holds above its first contents: every call so far
    for name in ("counts", "tails", "extremes"):
        assert np.array_equal(total[name], whole[name]), name


# ---------------------------------------------------------------------------------- refusals
def test_refused_calls_write_nothing_and_no_chains_is_ok(hip):
    key = ("abs", 3)
    model = model_of(key)
    hist = history(key, "sampler", 4, 70)
    user, wrong = model_of(key).__class__.from_buffer_copy(model), model_of(key).__class__.from_buffer_copy(model)
    user.sim_kind, wrong.y_dim = A.SIM_USER, 2
    top = 2 ** 63 - 1
    base = dict(model=model, n_rows=4, dim=3, n=70, stride=70, id0=0, step=70)
    for rc, kw in ((ERR_NULL, dict(model=None, dim=9)), (ERR_NULL, dict(hist=None, n_rows=0)), (ERR_DIM, dict(dim=2, n_rows=0)),
                   (ERR_DIM, dict(model=wrong, n=-1)), (ERR_DIM, dict(model=user, dim=4)), (ERR_KIND, dict(model=user, n_rows=0)),
                   (ERR_ARG, dict(n_rows=0)), (ERR_ARG, dict(n=-1)), (ERR_ARG, dict(stride=69)), (ERR_ARG, dict(id0=-1)), (ERR_ARG, dict(step=69)),
                   (ERR_ARG, dict(id0=top - 200)), (0, dict(n=0)), (0, dict(n=0, stride=0, step=0))):
        a = dict(base)
        a.update(kw)
        buf, ptr, _ = placed(hist, 0, 0)
        if "hist" in kw:
            ptr = None
        m = None if a["model"] is None else C.byref(a["model"])
        y, dis = Guarded(12, 73), Guarded(4, 72)
        assert hip.glabc_predictive_draws(m, ptr, a["n_rows"], a["dim"], a["n"], a["stride"], SEED, a["id0"], a["step"], y.ptr, 73, dis.ptr, 72,
                                          None) == rc, kw
        torch.cuda.synchronize()
        y.untouched(), dis.untouched()
        lo, hi, thr = np.zeros(4), np.ones(4), np.zeros(4, np.float32)
        tables = {"counts": prefilled(4 * 10), "tails": prefilled(16), "extremes": prefilled(8, np.uint32)}
        assert hip.glabc_predictive_counts(m, ptr, a["n_rows"], a["dim"], a["n"], a["stride"], SEED, a["id0"], a["step"], 7, lo.ctypes.data,
                                           hi.ctypes.data, thr.ctypes.data, tables["counts"][1], tables["tails"][1], tables["extremes"][1],
                                           None) == rc, kw
        torch.cuda.synchronize()
        for name, size, dt in (("counts", 40, np.uint64), ("tails", 16, np.uint64), ("extremes", 8, np.uint32)):
            assert np.array_equal(after(tables[name][0], size, dt), tables[name][2]), (kw, name)
    buf, ptr, _ = placed(hist, 0, 0)
    hip_draws(hip, model, hist, 0, 0, 0, 70, want=(), expect=ERR_NULL)
    for y_stride, dis_stride in ((69, 72), (73, 69)):
        y, dis = Guarded(12, 73), Guarded(4, 72)
        assert hip.glabc_predictive_draws(C.byref(model), ptr, 4, 3, 70, 70, SEED, 0, 70, y.ptr, y_stride, dis.ptr, dis_stride, None) == ERR_ARG
        y.untouched(), dis.untouched()
    lo, hi, thr, nan = np.zeros(4), np.ones(4), np.zeros(4, np.float32), np.array([0.0, 0.0, 0.0, np.nan])
    for rc, kw in ((ERR_NULL, dict(want=())), (ERR_NULL, dict(lo=None)), (ERR_NULL, dict(hi=None)), (ERR_NULL, dict(thr=None)),
                   (ERR_ARG, dict(n_bins=0)), (ERR_ARG, dict(n_bins=1025)), (ERR_ARG, dict(lo=hi, hi=lo)), (ERR_ARG, dict(hi=lo)),
                   (ERR_ARG, dict(lo=nan)), (ERR_ARG, dict(hi=np.array([1.0, np.inf, 1.0, 1.0]))), (ERR_ARG, dict(thr=nan.astype(np.float32)))):
        a = dict(n_bins=7, lo=lo, hi=hi, thr=thr, want=("counts", "tails", "extremes"))
        a.update(kw)
        hip_counts(hip, model, ptr, 4, 70, 70, 0, 70, a["n_bins"], a["lo"], a["hi"], a["thr"], want=a["want"], expect=rc)


# ---------------------------------------------------------------------------------- predictive.py end to end
def test_check_end_to_end_in_every_layout(hip):
    key = ("abs", 3)
    Model = R.abs_gauss_model(3, distribution.DiagGaussian(3, torch.zeros(3), torch.zeros(3)), epsilon=1.3)
    desc = Model.descriptor()
    hist = history(key, "sampler", 11, 130)
    y, dis = P.restate(desc, hist, 130, 77, 0, 130)
    stats = P.statistics(y, dis)
    buf = dev(np.array(hist))
    rows = buf.permute(0, 2, 1)                                                         # (T, C, D): used in place
    thr = np.array([1.5, 1.4, 1.3, 1.3], np.float32)
    lim = np.stack([np.nanmin(stats, axis=1), np.nanmax(stats, axis=1)], axis=1).astype(np.float64)
    for history_arg, layout in ((rows, "rows"), (buf, "chain_major")):
        c = predictive.check(Model, history_arg, bins=7, seed=77, layout=layout)       # range=None: the exact extremes
        assert c.n == 1430 and np.array_equal(c.y_edges[:, 0], lim[:3, 0]) and np.array_equal(c.y_edges[:, -1], lim[:3, 1])
        assert c.distance_edges[0] == lim[3, 0] and c.distance_edges[-1] == lim[3, 1]
        want = P.counts(stats, 7, lim[:, 0], lim[:, 1])
        assert np.array_equal(c.y_counts, want[:3, :7]) and np.array_equal(c.distance_counts, want[3, :7])
        assert not c.y_outside.any() and not c.distance_outside.any() and (c.y_counts.sum(axis=1) == 1430).all()
        assert np.array_equal(c.tails, P.tails(stats, thr))                              # the defaults: y_obs and epsilon
        e = predictive.check(Model, history_arg, bins=7, range=lim, seed=77, layout=layout)
        for got, ref in zip(e, c):
            assert np.array_equal(got, ref)
        for j in range(3):
            assert c.p_upper[j] == (stats[j] >= thr[j]).sum() / 1430
        assert c.within_epsilon == (stats[3] <= thr[3]).sum() / 1430
        # simulate, then the marginal histogram of y_rep: check's counts
        y_rep, distance = predictive.simulate(Model, history_arg, seed=77, layout=layout)
        assert y_rep.is_cuda and tuple(y_rep.shape) == ((11, 130, 3) if layout == "rows" else (11, 3, 130)) and tuple(distance.shape) == (11, 130)
        assert same(host(y_rep if layout == "chain_major" else y_rep.permute(0, 2, 1)), y) and same(host(distance), dis)
        h = diagnostics.histogram(y_rep, 7, layout=layout)
        assert np.array_equal(h.counts, c.y_counts) and np.array_equal(h.edges, c.y_edges)
        h = diagnostics.histogram(distance.reshape(11, 130, 1), 7)
        assert np.array_equal(h.counts[0], c.distance_counts)
    # shards of chains, and slices of rows, count the very draws of the whole job
    whole = predictive.terms(Model, rows, bins=7, range=lim, seed=77)
    parts = [predictive.terms(Model, rows[r0:r1, c0:c1], bins=7, range=lim, seed=77, chain0=c0, n_chains_total=130, row0=r0)
             for r0, r1 in ((0, 4), (4, 11)) for c0, c1 in ((0, 50), (50, 130))]
    both = predictive.combine(parts)
    assert both.n == whole.n == 1430 and np.array_equal(both.counts, whole.counts) and np.array_equal(both.tails, whole.tails)
    assert np.array_equal(whole.counts, P.counts(stats, 7, lim[:, 0], lim[:, 1]))
    # a single chain (T, D), a constant statistic widened by +-0.5, and a CPU history on the generic path
    one = predictive.check(Model, rows[:, 5], bins=3, seed=77, chain0=5, n_chains_total=130)
    assert one.n == 11 and np.array_equal(one.tails, P.tails(stats.reshape(4, 11, 130)[:, :, 5], thr))
    y1, d1 = predictive.simulate(Model, rows[:, 5], seed=77, chain0=5, n_chains_total=130)
    assert tuple(y1.shape) == (11, 3) and tuple(d1.shape) == (11,) and same(host(d1), dis[:, 5])
    single = predictive.check(Model, rows[:1, :1], bins=4, seed=77)
    assert single.n == 1 and np.allclose(single.y_edges[:, -1] - single.y_edges[:, 0], 1.0) and (single.y_counts.sum(axis=1) == 1).all()
    cpu = predictive.check(Model, torch.from_numpy(np.array(hist)), bins=7, range=lim, seed=77, layout="chain_major")
    assert cpu.n == 1430 and cpu.distance_counts is not None
    with pytest.raises(ValueError):                                                      # a NaN-only statistic has no range
        predictive.check(Model, torch.full((2, 2, 3), float("nan"), device="cuda"), seed=1)


def test_gk_check_runs_on_the_kernel(hip):
    from glabcmcmc_amd.examples.GK import GK_set
    Model = GK_set(200.0)
    hist = history(("gk", 4), "sampler", 9, 65)
    y, dis = P.restate(Model.descriptor(), hist, 65, 9, 0, 65)
    stats = P.statistics(y, dis)
    c = predictive.check(Model, dev(np.array(hist)), bins=5, seed=9, layout="chain_major")
    lim = np.stack([stats.min(axis=1), stats.max(axis=1)], axis=1).astype(np.float64)
    want = P.counts(stats, 5, lim[:, 0], lim[:, 1])
    assert c.y_counts.shape == (8, 5) and np.array_equal(c.y_counts, want[:8, :5]) and np.array_equal(c.distance_counts, want[8, :5])


# ---------------------------------------------------------------------------------- the law of the draws
def test_law_of_the_predictive_draws(hip):
    Model = R.abs_gauss_model(2, distribution.DiagGaussian(2, torch.zeros(2), torch.zeros(2)), epsilon=0.3, y_obs=[1.5, 1.5])
    desc = Model.descriptor()
    n = 65536
    history_arg = torch.ones(64, 1024, 2, device="cuda")
    for seed in (2026,):
        lim = [(1.0 - float(desc.noise.p2[j]), 1.0 + float(desc.noise.p2[j])) for j in range(2)] + [(0.0, 10.0)]
        assert abs(lim[0][1] - 1.0 - math.sqrt(0.05)) < 1e-6
        c = predictive.check(Model, history_arg, bins=1, range=lim, thresholds=[1.0, 1.0, 0.3], seed=seed)
        assert c.n == n and (c.tails.sum(axis=1) == n).all() and not c.tails[:, 3].any()
        mass = c.y_counts[:, 0] / n
        p = math.erf(1.0 / math.sqrt(2.0))
        print("p_upper %r (0.5 +- %.4f), mass %r (%.4f +- %.4f)" % (c.p_upper.tolist(), 0.5 / 256, mass.tolist(), p, math.sqrt(p * (1 - p) / n)))
        assert (np.abs(c.p_upper - 0.5) <= 5 * 0.5 / 256).all()
        assert (np.abs(mass - p) <= 5 * math.sqrt(p * (1.0 - p) / n)).all()
