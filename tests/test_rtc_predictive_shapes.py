"""glabc_rtc_predictive_draws / glabc_rtc_predictive_counts (csrc/glabc_rtc.hip: predictive_kernel of csrc/glabc_predictive.h compiled
around a user's simulator) on the GPU, bit for bit.

(a) The restated Mixture source equals the built-in glabc_predictive_draws / glabc_predictive_counts on the equivalent
    GLABC_SIM_ABS_GAUSS Model in every output and every table.
(b) NONLINEAR (3, 2, 4), a source with its own discrepancy and kernel (2, 3, 3), ALL_USER (2, 3, 3: its own prior too, which a
    predictive program accepts and never evaluates), and the edge pair theta 1 / noise 1 and theta 8, y 8, noise 5 (five normals
    straddle a Philox block) equal the composed entry points of include/glabc.h -- per history row glabc_dist_forward of a standard
    DiagGaussian under seed ^ GLABC_PREDICTIVE_KEY at row0 = id0 + t id_step, glabc_rtc_simulate, glabc_rtc_model_rows /
    glabc_model_discrepancy -- and a host restatement: the noise as tests/predictive_ref.py draws it, the same source through gcc
    (test_rtc.host_simulator / host_hooks) for the simulator and the discrepancy.  "Equal bits" lets a NaN match a NaN of another
    payload, as in tests/test_predictive_shapes.py.

Shapes, a covering grid and no product (test_grid_covers_every_pair): chains 1, 63, 64, 65, 321; rows 1 .. 9, 15, 16, 17, 33 -- both
sides of R and of 2 R for any rows-per-item rule R <= 16, so the grid does not know the rule the program was compiled with --; 17
padding columns of NaN behind every row segment (a stride that is no multiple of 4; a read of one changes a draw); a base pointer
0 .. 3 floats into a wider buffer; ids from 0, crossing 2^32 inside a call, and past 2^40 with id_step > n_chains.  Tables at 1, 64
and 1024 bins, each table and each draws output alone, every output between guard bands, two chain shards times two row slices
adding up to the whole, and the refusals between the four kinds of program.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle_lib
import predictive_ref as P
import rejection_ref as R
from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import distribution
from glabcmcmc_amd.compiled import CompiledModel
from helpers import dev, host
from test_predictive_shapes import IDS, KEY, SEED, Guarded, after, placed, prefilled, same
from test_rtc import ALL_USER, NONLINEAR, host_hooks, host_simulator, mixture_source, user_model_desc
from test_rtc_draws_host import DIS_AND_KERNEL
from test_rtc_draws_shapes import EDGE1, EDGE8, population_of

pytestmark = pytest.mark.gpu

ERR_NULL, ERR_DIM, ERR_KIND, ERR_ARG = -1, -2, -3, -4
CHAINS = (1, 63, 64, 65, 321)
ROWS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 33)
PAD = 17
OFFSETS = (0, 1, 2, 3)
BINS = (1, 64, 1024)
SOURCES = {"nonlinear": (NONLINEAR, (3, 2, 4)), "dis_and_kernel": (DIS_AND_KERNEL, (2, 3, 3)), "all_user": (ALL_USER, (2, 3, 3)),
           "edge1": (EDGE1, (1, 1, 1)), "edge8": (EDGE8, (8, 8, 5))}
NAMES = ("mixture",) + tuple(SOURCES)


@functools.lru_cache(maxsize=None)
def builtin_mixture():
    prior = distribution.DiagGaussian(2, torch.zeros(2), torch.zeros(2))
    return R.abs_gauss_model(2, prior, epsilon=1.0).descriptor()


@functools.lru_cache(maxsize=None)
def source_of(name):
    if name == "mixture":
        m = builtin_mixture()
        return mixture_source([m.noise.p2[0], m.noise.p2[1]]), (2, 2, 2)
    return SOURCES[name]


@functools.lru_cache(maxsize=None)
def model_of(name):
    """the glabc_model (GLABC_SIM_USER) of a source"""
    if name == "mixture":
        return user_model_desc(builtin_mixture(), 2)
    source, (d, yd, nd) = source_of(name)
    prior = distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d))
    return CompiledModel(theta_dim=d, y_dim=yd, simulator_source=source, prior=prior, y_obs=[1.0 - 0.1 * j for j in range(yd)],
                         epsilon=0.6 + 0.5 * yd, noise_dim=nd).descriptor()


@functools.lru_cache(maxsize=None)
def program_of(name):
    """the predictive program of a source: compiled once per module, never released before the interpreter ends"""
    source, (d, yd, nd) = source_of(name)
    handle, log = C.c_void_p(), C.create_string_buffer(1 << 14)
    rc = A.lib().glabc_rtc_compile_predictive(source.encode(), d, yd, nd, C.byref(handle), log, len(log))
    assert rc == 0, log.value.decode()
    assert b"spills" not in log.value, log.value.decode()
    return handle


@functools.lru_cache(maxsize=None)
def host_source(name):
    source, dims = source_of(name)
    return host_simulator(source, *dims)


@functools.lru_cache(maxsize=None)
def cases():
    """(source, n_rows, n_chains, offset, id case): every source meets every row count, the other axes rotate with different periods"""
    out = []
    for si, name in enumerate(NAMES):
        for ri, n_rows in enumerate(ROWS):
            i = len(out)
            out.append((name, n_rows, CHAINS[(si + 2 * ri + i // 13) % 5], OFFSETS[(i + i // 4) % 4], (i + i // 3) % 3))
    return tuple(out)


def test_grid_covers_every_pair():
    rows = [c[1:] for c in cases()]
    axes = (ROWS, CHAINS, OFFSETS, (0, 1, 2))
    for a in range(len(axes)):
        assert {c[a] for c in rows} == set(axes[a]), (a, {c[a] for c in rows})
        for b in range(len(axes)):
            for v in axes[a]:
                assert a == b or len({c[b] for c in rows if c[a] == v}) >= 2, (a, v, b)
    for name in NAMES:
        mine = [c for c in cases() if c[0] == name]
        assert {c[1] for c in mine} == set(ROWS) and {c[2] for c in mine} == set(CHAINS) and {c[4] for c in mine} == {0, 1, 2}
        assert {c[3] for c in mine} == set(OFFSETS)


@functools.lru_cache(maxsize=None)
def history(name, n_rows, n):
    """chain-major float32 [n_rows][D][n], sampler-like values"""
    d = source_of(name)[1][0]
    h = (1.5 * np.random.default_rng(1000 * n_rows + n + d).standard_normal((n_rows, d, n))).astype(np.float32)
    h.setflags(write=False)
    return h


# ---------------------------------------------------------------------------------- the two twins
def restate(name, hist, id0, id_step):
    """-> (y [n_rows][YD][n], distance [n_rows][n]) from the checker's noise and the source through gcc (module docstring)"""
    L = oracle_lib.load()
    model = model_of(name)
    lib, fn = host_source(name)
    n_rows, d, n = hist.shape
    yd, nd = model.y_dim, model.noise.dim
    theta = np.ascontiguousarray(hist.transpose(0, 2, 1).reshape(n_rows * n, d))
    ids = P.ids_of(n_rows, n, id0, id_step).reshape(-1)
    eps = R.noise_normals((SEED ^ P.PREDICTIVE_KEY ^ R.NOISE_KEY) & R.M64, ids, nd)
    y, dis = np.empty((n_rows * n, yd), np.float32), np.empty(n_rows * n, np.float32)
    L.oracle_set_user_simulator(fn)
    L.oracle_set_user_model(*host_hooks(lib))
    try:
        for i in range(n_rows * n):                                        # row by row: the checker strides eps by y_dim
            assert L.oracle_model_simulate(C.byref(model), theta[i].ctypes.data, eps[i].ctypes.data, 1, y[i].ctypes.data) == 0
        assert L.oracle_model_discrepancy(C.byref(model), y.ctypes.data, n_rows * n, dis.ctypes.data) == 0
    finally:
        L.oracle_set_user_model(None, None, None)
    return np.ascontiguousarray(y.reshape(n_rows, n, yd).transpose(0, 2, 1)), dis.reshape(n_rows, n)


def composed(hip, name, hist, id0, id_step):
    """the entry points a predictive draw is composed of (include/glabc.h), theta, eps and y through device memory"""
    model, prog = model_of(name), program_of(name)
    n_rows, d, n = hist.shape
    yd, nd = model.y_dim, model.noise.dim
    ys, ds = [], []
    for t in range(n_rows):
        theta = dev(np.ascontiguousarray(hist[t].T))
        e, lq = torch.empty(nd, n, device="cuda"), torch.empty(n, device="cuda")
        assert hip.glabc_dist_forward(C.byref(model.noise), n, KEY, id0 + t * id_step, e.data_ptr(), lq.data_ptr(), None) == 0
        eps = e.t().contiguous()
        y, dis = torch.empty(n, yd, device="cuda"), torch.empty(n, device="cuda")
        assert hip.glabc_rtc_simulate(prog, theta.data_ptr(), eps.data_ptr(), n, y.data_ptr(), None) == 0
        if "GLABC_USER_DISCREPANCY" in source_of(name)[0]:
            assert hip.glabc_rtc_model_rows(prog, C.byref(model), A.RTC_DISCREPANCY, y.data_ptr(), n, dis.data_ptr(), None) == 0
        else:
            assert hip.glabc_model_discrepancy(C.byref(model), y.data_ptr(), n, dis.data_ptr(), None) == 0
        ys.append(host(y).T)
        ds.append(host(dis))
    return np.stack(ys), np.stack(ds)


# ---------------------------------------------------------------------------------- the calls
def call_draws(hip, name, hist, pad, offset, id0, id_step, want=("y", "dis"), expect=0, program=None, model=None, builtin=False, dim=None):
    """one call into guarded buffers -> {name: host array}; builtin: glabc_predictive_draws on `model`"""
    model = model_of(name) if model is None else model
    program = program_of(name) if program is None and not builtin else program
    n_rows, d, n = hist.shape
    buf, ptr, stride = placed(hist, pad, offset)
    yd = model.y_dim
    y, dis = Guarded(n_rows * yd, n + 3), Guarded(n_rows, n + 2)
    head = (C.byref(model),) if builtin else (program, C.byref(model))
    fn = hip.glabc_predictive_draws if builtin else hip.glabc_rtc_predictive_draws
    rc = fn(*head, ptr, n_rows, d if dim is None else dim, n, stride, SEED, id0, id_step, y.ptr if "y" in want else None, n + 3,
            dis.ptr if "dis" in want else None, n + 2, None)
    torch.cuda.synchronize()
    assert rc == expect, rc
    out = {}
    for k, b in (("y", y), ("dis", dis)):
        if k in want and rc == 0:
            out[k] = b.read(n).reshape((n_rows, yd, n) if k == "y" else (n_rows, n)).copy()
        else:
            b.untouched()
    return out


def call_counts(hip, name, ptr, n_rows, n, stride, id0, id_step, n_bins, lo, hi, thr, want=("counts", "tails", "extremes"), tables=None,
                expect=0, program=None, model=None, builtin=False):
    """one counts call -> ({name: what the call added (counts, tails) or left (extremes)}, the tables); `tables`: accumulate into these"""
    model = model_of(name) if model is None else model
    program = program_of(name) if program is None and not builtin else program
    k = model.y_dim + 1
    sizes = {"counts": k * (n_bins + 3), "tails": 4 * k, "extremes": 2 * k}
    if tables is None:
        tables = {"counts": prefilled(sizes["counts"]), "tails": prefilled(sizes["tails"]),
                  "extremes": prefilled(sizes["extremes"], np.uint32, np.tile(np.array(P.KEY_NONE, np.uint32), k))}
    lo = None if lo is None else np.ascontiguousarray(lo, np.float64)
    hi = None if hi is None else np.ascontiguousarray(hi, np.float64)
    thr = None if thr is None else np.ascontiguousarray(thr, np.float32)
    p = lambda a: None if a is None else a.ctypes.data          # noqa: E731
    q = lambda key: tables[key][1] if key in want else None      # noqa: E731
    head = (C.byref(model),) if builtin else (program, C.byref(model))
    fn = hip.glabc_predictive_counts if builtin else hip.glabc_rtc_predictive_counts
    rc = fn(*head, ptr, n_rows, model.theta_dim, n, stride, SEED, id0, id_step, n_bins, p(lo), p(hi), p(thr), q("counts"), q("tails"),
            q("extremes"), None)
    torch.cuda.synchronize()
    assert rc == expect, rc
    out = {}
    for key in ("counts", "tails", "extremes"):
        t, _, before = tables[key]
        now = after(t, sizes[key], np.uint32 if key == "extremes" else np.uint64)
        if key in want and rc == 0:
            out[key] = (now.copy() if key == "extremes" else now - before).reshape(k, -1)
        else:
            assert np.array_equal(now, before), "%s was written by a call that must not" % key
    return out, tables


def axes_of(stats):
    """a range and thresholds made of the statistics' own values: the closed last bin and the "equal" slot occur"""
    finite = [np.sort(x[np.isfinite(x)]) for x in stats]
    lo = np.array([float(s[len(s) // 10]) for s in finite])
    hi = np.array([float(s[9 * len(s) // 10]) for s in finite])
    thr = np.array([s[len(s) // 2] for s in finite], np.float32)
    return lo, hi, thr


# ---------------------------------------------------------------------------------- (a) the Mixture source against the built-in kernels
def test_mixture_source_equals_the_builtin_kernel(hip):
    n_cases = 0
    for _, n_rows, n, offset, idc in (c for c in cases() if c[0] == "mixture"):
        hist = history("mixture", n_rows, n)
        id0, id_step = IDS[idc][0], n + IDS[idc][1]
        where = (n_rows, n, offset, id0, id_step)
        got = call_draws(hip, "mixture", hist, PAD, offset, id0, id_step)
        want = call_draws(hip, "mixture", hist, PAD, offset, id0, id_step, model=builtin_mixture(), builtin=True)
        assert same(got["y"], want["y"]) and same(got["dis"], want["dis"]), where
        if n_rows * n > 60:
            lo, hi, thr = axes_of(P.statistics(want["y"], want["dis"]))
            buf, ptr, stride = placed(hist, PAD, offset)
            n_bins = BINS[n_cases % 3]
            a, _ = call_counts(hip, "mixture", ptr, n_rows, n, stride, id0, id_step, n_bins, lo, hi, thr)
            b, _ = call_counts(hip, "mixture", ptr, n_rows, n, stride, id0, id_step, n_bins, lo, hi, thr, model=builtin_mixture(), builtin=True)
            for key in ("counts", "tails", "extremes"):
                assert np.array_equal(a[key], b[key]), (where, n_bins, key)
            assert (a["tails"].sum(axis=1) == n_rows * n).all() and a["tails"][:, 1].all()
        n_cases += 1
    assert n_cases == len(ROWS)


# ---------------------------------------------------------------------------------- (b) composition and restatement
@pytest.mark.parametrize("name", list(SOURCES))
def test_draws_equal_the_composition_and_the_restatement(hip, name):
    n_cases = 0
    for _, n_rows, n, offset, idc in (c for c in cases() if c[0] == name):
        hist = history(name, n_rows, n)
        id0, id_step = IDS[idc][0], n + IDS[idc][1]
        where = (name, n_rows, n, offset, id0, id_step)
        got = call_draws(hip, name, hist, PAD, offset, id0, id_step)
        y, dis = composed(hip, name, hist, id0, id_step)
        assert same(got["y"], y) and same(got["dis"], dis), ("composition", where)
        y, dis = restate(name, hist, id0, id_step)
        assert same(got["y"], y) and same(got["dis"], dis), ("restatement", where)
        assert np.isfinite(got["dis"]).all(), where
        n_cases += 1
    assert n_cases == len(ROWS)


@pytest.mark.parametrize("name", ["nonlinear", "all_user", "edge8"])
def test_each_draws_output_alone_and_slabs_address_the_same_draws(hip, name):
    hist = history(name, 9, 65)
    whole = call_draws(hip, name, hist, PAD, 1, 2 ** 32 - 40, 70)
    assert same(call_draws(hip, name, hist, PAD, 1, 2 ** 32 - 40, 70, want=("y",))["y"], whole["y"])
    assert same(call_draws(hip, name, hist, 0, 3, 2 ** 32 - 40, 70, want=("dis",))["dis"], whole["dis"])
    # a slab of chains from a slice of rows, with the matching id0: the very draws of the whole
    part = call_draws(hip, name, np.ascontiguousarray(hist[4:, :, 10:]), 0, 2, 2 ** 32 - 40 + 4 * 70 + 10, 70)
    assert same(part["y"], whole["y"][4:, :, 10:]) and same(part["dis"], whole["dis"][4:, 10:])
    other = call_draws(hip, name, hist, 0, 0, 2 ** 32 - 39, 70)
    assert not same(other["dis"], whole["dis"])


@functools.lru_cache(maxsize=None)
def counts_reference(name):
    """33 rows x 321 chains with two draws whose theta is NaN, the restated statistics and axes made of restated values: computed
    once, never modified"""
    hist = np.array(history(name, 33, 321))
    hist[1, :, 5], hist[17, :, 300] = np.nan, np.nan
    stats = P.statistics(*restate(name, hist, 2 ** 32 - 40, 328))
    lo, hi, thr = axes_of(stats)
    for a in (hist, stats, lo, hi, thr):
        a.setflags(write=False)
    return hist, stats, lo, hi, thr


@pytest.mark.parametrize("name", list(SOURCES))
def test_counts_tails_and_extremes_equal_the_restatement(hip, name):
    hist, stats, lo, hi, thr = counts_reference(name)
    n_rows, _, n = hist.shape
    buf, ptr, stride = placed(hist, PAD, 3)
    want_tails, want_extremes = P.tails(stats, thr), P.extremes(stats)
    assert want_tails[:, 1].all() and (want_tails.sum(axis=1) == n_rows * n).all()
    for n_bins in BINS:
        got, _ = call_counts(hip, name, ptr, n_rows, n, stride, 2 ** 32 - 40, 328, n_bins, lo, hi, thr)
        want = P.counts(stats, n_bins, lo, hi)
        assert np.array_equal(got["counts"], want), (name, n_bins, np.argwhere(got["counts"] != want)[:4])
        assert want[:, n_bins].all() and want[:, n_bins + 1].all() and want[:, n_bins - 1].all()
        assert np.array_equal(got["tails"], want_tails) and np.array_equal(got["extremes"], want_extremes), (name, n_bins)
    for want in (("counts",), ("tails",), ("extremes",)):                  # each table alone, what only the others read NULL
        got, _ = call_counts(hip, name, ptr, n_rows, n, stride, 2 ** 32 - 40, 328, 64, lo if "counts" in want else None,
                             hi if "counts" in want else None, thr if "tails" in want else None, want=want)
        assert set(got) == set(want)
        for key, ref in (("counts", P.counts(stats, 64, lo, hi)), ("tails", want_tails), ("extremes", want_extremes)):
            assert key not in got or np.array_equal(got[key], ref), (name, want, key)


@pytest.mark.parametrize("name", ["dis_and_kernel", "edge8"])
def test_tables_add_over_two_chain_shards_and_two_row_slices(hip, name):
    hist, stats, lo, hi, thr = counts_reference(name)
    n_rows, d, n = hist.shape
    buf, ptr, stride = placed(hist, PAD, 1)
    id0, step = 2 ** 32 - 40, 328
    whole, _ = call_counts(hip, name, ptr, n_rows, n, stride, id0, step, 64, lo, hi, thr)
    assert np.array_equal(whole["counts"], P.counts(stats, 64, lo, hi))
    tables, total = None, None
    for row0, rows in ((0, 8), (8, n_rows - 8)):
        for chain0, k in ((0, 130), (130, n - 130)):
            got, tables = call_counts(hip, name, ptr + 4 * (row0 * d * stride + chain0), rows, k, stride, id0 + row0 * step + chain0, step, 64,
                                      lo, hi, thr, tables=tables)
            total = got                                                    # what the table holds above its first contents: every call so far
    for key in ("counts", "tails", "extremes"):
        assert np.array_equal(total[key], whole[key]), key


# ---------------------------------------------------------------------------------- refusals
def other_programs(hip):
    """a sampler, a mixture and a draws program of NONLINEAR's shape"""
    out = []
    for fn in (hip.glabc_rtc_compile, hip.glabc_rtc_compile_mix):
        handle, log = C.c_void_p(), C.create_string_buffer(1 << 14)
        assert fn(NONLINEAR.encode(), A.ALGO_GLMCMC, 3, 2, 4, 5, C.byref(handle), log, len(log)) == 0, log.value.decode()
        out.append(handle)
    handle, log = C.c_void_p(), C.create_string_buffer(1 << 14)
    assert hip.glabc_rtc_compile_draws(NONLINEAR.encode(), 3, 2, 4, C.byref(handle), log, len(log)) == 0, log.value.decode()
    out.append(handle)
    return out


def changed(m, **fields):
    c = A.Model()
    C.memmove(C.byref(c), C.byref(m), C.sizeof(A.Model))
    for k, v in fields.items():
        obj, key = (c.prior, k[6:]) if k.startswith("prior_") else (c.noise, k[6:]) if k.startswith("noise_") else (c, k)
        setattr(obj, key, v)
    return c


def test_refusals_in_their_order_and_between_the_kinds_of_program(hip):
    name = "nonlinear"
    m, hist = model_of(name), history(name, 4, 70)
    lo, hi, thr = np.zeros(3), np.ones(3), np.zeros(3, np.float32)
    others = other_programs(hip)
    try:
        buf, ptr, stride = placed(hist, 0, 0)

        def both(expect, **kw):
            """the same refusal from both entry points, nothing written"""
            call_draws(hip, name, hist, 0, 0, 0, 70, expect=expect, **kw)
            call_counts(hip, name, ptr, 4, 70, stride, 0, 70, 7, lo, hi, thr, expect=expect, **kw)

        # a NULL program or model, ahead of everything else
        p8 = C.c_void_p(8)
        assert hip.glabc_rtc_predictive_draws(None, C.byref(m), ptr, 4, 3, 70, 70, SEED, 0, 70, p8, 70, None, 0, None) == ERR_NULL
        assert hip.glabc_rtc_predictive_draws(program_of(name), None, ptr, 4, 3, 70, 70, SEED, 0, 70, p8, 70, None, 0, None) == ERR_NULL
        assert hip.glabc_rtc_predictive_counts(program_of(name), None, ptr, 4, 3, 70, 70, SEED, 0, 70, 7, None, None, None, p8, None, None,
                                               None) == ERR_NULL
        # the simulator's kind, ahead of the program's kind, ahead of the dimensions
        both(ERR_KIND, model=changed(m, sim_kind=A.SIM_ABS_GAUSS), program=others[0])
        both(ERR_KIND, model=changed(m, sim_kind=A.SIM_GK, theta_dim=4))
        for other in others:
            both(ERR_KIND, program=other)
            both(ERR_KIND, program=other, model=changed(m, theta_dim=2))
        # the dimensions, whatever the prior
        for f in (dict(theta_dim=2), dict(y_dim=3), dict(noise_dim=3)):
            call_draws(hip, name, hist, 0, 0, 0, 70, expect=ERR_DIM, model=changed(m, prior_kind=A.DIST_GAMMA, **f))
        both(ERR_DIM, program=program_of("edge1"))
        # ... ahead of what the built-in entry points refuse: every output NULL, the history's theta_dim, the range
        call_draws(hip, name, hist, 0, 0, 0, 70, want=(), expect=ERR_NULL)
        call_draws(hip, name, hist, 0, 0, 0, 70, want=(), expect=ERR_DIM, model=changed(m, y_dim=3))
        call_draws(hip, name, hist, 0, 0, 0, 70, expect=ERR_DIM, dim=2)
        call_draws(hip, name, hist, 0, 0, -1, 70, expect=ERR_ARG)
        call_draws(hip, name, hist, 0, 0, 0, 69, expect=ERR_ARG)
        call_draws(hip, name, hist, 0, 0, 2 ** 63 - 200, 70, expect=ERR_ARG)
        call_counts(hip, name, ptr, 4, 70, stride, 0, 70, 7, lo, hi, thr, want=(), expect=ERR_NULL)
        call_counts(hip, name, ptr, 4, 70, stride, 0, 70, 7, None, hi, thr, expect=ERR_NULL)
        call_counts(hip, name, ptr, 4, 70, stride, 0, 70, 7, lo, hi, None, expect=ERR_NULL)
        call_counts(hip, name, ptr, 0, 70, stride, 0, 70, 7, lo, hi, thr, expect=ERR_ARG)
        call_counts(hip, name, ptr, 4, 70, 69, 0, 70, 7, lo, hi, thr, expect=ERR_ARG)
        for n_bins in (0, 1025):
            call_counts(hip, name, ptr, 4, 70, stride, 0, 70, n_bins, lo, hi, thr, expect=ERR_ARG)
        call_counts(hip, name, ptr, 4, 70, stride, 0, 70, 7, hi, lo, thr, expect=ERR_ARG)
        call_counts(hip, name, ptr, 4, 70, stride, 0, 70, 7, lo, hi, np.array([0.0, np.nan, 0.0], np.float32), expect=ERR_ARG)
        # a Gamma prior or a prior of another dimension in the descriptor is no ground for refusal: theta comes from the history
        ok = call_draws(hip, name, hist, 0, 0, 0, 70)
        for f in (dict(prior_kind=A.DIST_GAMMA), dict(prior_dim=2)):
            assert same(call_draws(hip, name, hist, 0, 0, 0, 70, model=changed(m, **f))["dis"], ok["dis"])
        # no chains: OK, nothing written
        y, dis = Guarded(8, 3), Guarded(4, 2)
        assert hip.glabc_rtc_predictive_draws(program_of(name), C.byref(m), ptr, 4, 3, 0, 70, SEED, 0, 70, y.ptr, 3, dis.ptr, 2, None) == 0
        torch.cuda.synchronize()
        y.untouched(), dis.untouched()
        tables = {"counts": prefilled(30), "tails": prefilled(12), "extremes": prefilled(6, np.uint32)}
        assert hip.glabc_rtc_predictive_counts(program_of(name), C.byref(m), ptr, 4, 3, 0, 70, SEED, 0, 70, 7, lo.ctypes.data, hi.ctypes.data,
                                               thr.ctypes.data, tables["counts"][1], tables["tails"][1], tables["extremes"][1], None) == 0
        torch.cuda.synchronize()
        for key, size, dt in (("counts", 30, np.uint64), ("tails", 12, np.uint64), ("extremes", 6, np.uint32)):
            assert np.array_equal(after(tables[key][0], size, dt), tables[key][2]), key
        # the built-in entry points keep refusing a user simulator
        call_draws(hip, name, hist, 0, 0, 0, 70, expect=ERR_KIND, builtin=True)
        call_counts(hip, name, ptr, 4, 70, stride, 0, 70, 7, lo, hi, thr, expect=ERR_KIND, builtin=True)
    finally:
        for h in others:
            hip.glabc_rtc_release(h)


def test_other_entry_points_refuse_a_predictive_program_and_the_row_kernels_take_it(hip):
    name = "nonlinear"
    m, prog = model_of(name), program_of(name)
    d = 3
    local = distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d)).descriptor()
    th, y = torch.zeros(d, 64, device="cuda"), torch.zeros(2, 64, device="cuda")
    lw, flags = torch.zeros(64, device="cuda"), torch.zeros(64, dtype=torch.int32, device="cuda")
    c = A.Chains()
    c.theta, c.y, c.log_w, c.flags = th.data_ptr(), y.data_ptr(), lw.data_ptr(), flags.data_ptr()
    c.n_chains, c.stride = 64, 64
    r = A.Run()
    r.n_steps, r.batch_size, r.global_frequency = 1, 5, 0.5
    assert hip.glabc_rtc_steps(prog, C.byref(m), C.byref(local), C.byref(local), C.byref(c), C.byref(r), None) == ERR_KIND
    mix = distribution.GaussianMixture(2, d, loc=np.zeros((2, d)), scale=np.ones((2, d)), weights=[1.0, 1.0]).descriptor()
    assert hip.glabc_rtc_mix_steps(prog, C.byref(m), C.byref(local), C.byref(mix), C.byref(c), C.byref(r), None) == ERR_KIND
    out = torch.zeros(d, 64, device="cuda")
    assert hip.glabc_rtc_abc_draws(prog, C.byref(m), SEED, 0, None, 64, 64, out.data_ptr(), None, None, None, None) == ERR_KIND
    pop = population_of(("nonlinear", "gauss"))
    assert hip.glabc_rtc_smc_draws(prog, C.byref(m), C.byref(pop.struct), SEED, 0, None, 64, 64, out.data_ptr(), None, None, None, None,
                                   None) == ERR_KIND
    torch.cuda.synchronize()
    assert not th.any() and not y.any() and not out.any()
    up, ud, uk = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    assert hip.glabc_rtc_hooks(program_of("all_user"), C.byref(up), C.byref(ud), C.byref(uk)) == 0
    assert (up.value, ud.value, uk.value) == (1, 1, 1)
    assert hip.glabc_rtc_hooks(prog, C.byref(up), C.byref(ud), C.byref(uk)) == 0 and (up.value, ud.value, uk.value) == (0, 0, 0)
    # glabc_rtc_simulate and glabc_rtc_model_rows: used by `composed` in every case above, for sources with and without a distance
