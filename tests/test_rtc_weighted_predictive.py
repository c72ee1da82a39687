"""glabc_rtc_compile_weighted_predictive / glabc_rtc_weighted_predictive_counts (csrc/glabc_rtc.hip: weighted_predictive_kernel of
csrc/glabc_weighted_predictive.h compiled around a user's simulator) and predictive.check_weighted on a CompiledModel, on the GPU,
equal integers throughout.

(a) The Mixture simulator restated as C source gives the built-in glabc_weighted_predictive_counts' three tables on the equivalent
    GLABC_SIM_ABS_GAUSS Model, on the same draws, weights, ids and axes.
(b) A source whose distance is the user's (GLABC_USER_DISCREPANCY) is held to integer sums of m over the draws
    glabc_rtc_predictive_draws of the predictive program of the same source makes for the same ids.
(c) CompiledModel.weighted_predictive_program() passes its self-check and serves check_weighted under "auto"; a disagreeing
    self-check hands no program out; a source that does not compile in this program warns under "auto" and runs generic, and raises
    under "fused".
The shapes are those at which a kernel of one segment per item takes another path: n = 1, 63, 64, 65, 8 x 64 + 1, with 17 padding
columns of NaN, base pointers 0 .. 3 floats into wider buffers, ids crossing 2^32 and past 2^40, and the weights of
tests/test_weighted_predictive_shapes.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import weighted_predictive_ref as WP
from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import predictive, weighted
from glabcmcmc_amd.compiled import CompiledModel, SimulatorCompileError, SimulatorSelfCheckError
from helpers import host, make_dist
from test_predictive_shapes import IDS, SEED
from test_rtc import NONLINEAR
from test_rtc_predictive_shapes import builtin_mixture, model_of, source_of
from test_rtc_predictive_shapes import program_of as predictive_program_of
from test_weighted_predictive_shapes import WANTS, axes_of, call, placed_draws, reference, weights_of

pytestmark = pytest.mark.gpu

ERR_NULL, ERR_DIM, ERR_KIND, ERR_ARG = -1, -2, -3, -4
DRAWS = (1, 63, 64, 65, 8 * 64 + 1)


@functools.lru_cache(maxsize=None)
def program_of(name):
    """the weighted predictive program of a source: compiled once per module, never released before the interpreter ends"""
    source, (d, yd, nd) = source_of(name)
    handle, log = C.c_void_p(), C.create_string_buffer(1 << 14)
    rc = A.lib().glabc_rtc_compile_weighted_predictive(source.encode(), d, yd, nd, C.byref(handle), log, len(log))
    assert rc == 0, log.value.decode()
    assert b"spill" not in log.value and b"private segment" not in log.value, log.value.decode()
    return handle


@functools.lru_cache(maxsize=None)
def draws_of(d, n):
    x = (1.5 * np.random.default_rng(100 * n + d).standard_normal((d, n))).astype(np.float32)
    if n > 40:
        x[:, 3] = np.nan                                           # carries no weight
    x.setflags(write=False)
    return x


def rtc_call(hip, name, *args, **kw):
    model, prog = model_of(name), program_of(name)
    return call(hip, model, *args, fn=lambda *a: hip.glabc_rtc_weighted_predictive_counts(prog, C.byref(model), *a), **kw)


def test_the_restated_mixture_source_equals_the_built_in_kernel(hip):
    builtin, user = builtin_mixture(), model_of("mixture")
    for i, n in enumerate(DRAWS):
        scale, id0, want = (1.0, 0.5, 4.0)[i % 3], IDS[i % 3][0], WANTS[i % 5]
        x, w = draws_of(2, n), weights_of(n, scale)
        keep, ptr, stride, wptr = placed_draws(x, w, 17 * (i % 2), i % 4)
        m = WP.multiplicity(w, scale)
        lo, hi, thr = axes_of(WP.statistics(builtin, x, n, SEED, id0), m)
        for n_bins in (1, 64, 512):
            ref, _ = call(hip, builtin, ptr, stride, wptr, n, scale, id0, n_bins, lo, hi, thr, want=want)
            got, _ = rtc_call(hip, "mixture", ptr, stride, wptr, n, scale, id0, n_bins, lo, hi, thr, want=want)
            assert set(got) == set(want)
            for name in want:
                assert np.array_equal(got[name], ref[name]), (n, n_bins, name)
        assert user.sim_kind == A.SIM_USER and builtin.sim_kind != A.SIM_USER


def test_a_user_distance_equals_the_sums_over_the_predictive_programs_draws(hip):
    name = "dis_and_kernel"
    assert "GLABC_USER_DISCREPANCY" in source_of(name)[0]
    model, reference_program = model_of(name), predictive_program_of(name)
    d, yd = model.theta_dim, model.y_dim
    for i, n in enumerate(DRAWS):
        scale, id0 = (0.5, 4.0, 1.0)[i % 3], IDS[(i + 1) % 3][0]
        x, w = draws_of(d, n), weights_of(n, scale)
        keep, ptr, stride, wptr = placed_draws(x, w, 17 * ((i + 1) % 2), (i + 2) % 4)
        y, dis = torch.empty(yd, n, device="cuda"), torch.empty(n, device="cuda")
        assert hip.glabc_rtc_predictive_draws(reference_program, C.byref(model), ptr, 1, d, n, stride, SEED, id0, n, y.data_ptr(), n, dis.data_ptr(), n,
                                              None) == 0
        stats = np.ascontiguousarray(np.concatenate([host(y), host(dis)[None]]).T)
        m = WP.multiplicity(w, scale)
        lo, hi, thr = axes_of(stats, m)
        for want in (WANTS[0], WANTS[i % 5]):
            got, _ = rtc_call(hip, name, ptr, stride, wptr, n, scale, id0, 7, lo, hi, thr, want=want)
            ref = reference(stats, m, 7, lo, hi, thr)
            for table in want:
                assert np.array_equal(got[table], ref[table]), (n, want, table)
        if n > 40:
            assert (reference(stats, m, 7, lo, hi, thr)["tails"].sum(axis=1) == sum(m)).all() and sum(m) > 2 ** 32
    # slices with id0 + a add up to the one-shot tables: inside a segment and on a segment's edge (an item is one segment here)
    n, scale, id0 = 513, 0.5, 2 ** 32 - 40
    x, w = draws_of(d, n), weights_of(n, scale)
    keep, ptr, stride, wptr = placed_draws(x, w, 17, 1)
    whole, _ = rtc_call(hip, name, ptr, stride, wptr, n, scale, id0, 7, lo, hi, thr)
    for a in (37, 128):
        tables, total = None, None
        for first, count in ((0, a), (a, n - a)):
            total, tables = rtc_call(hip, name, ptr + 4 * first, stride, wptr + 4 * first, count, scale, id0 + first, 7, lo, hi, thr, tables=tables)
        for table in WANTS[0]:
            assert np.array_equal(total[table], whole[table]), (a, table)


def test_refusals_between_the_kinds_of_program(hip):
    x, w = draws_of(2, 70), weights_of(70, 1.0)
    keep, ptr, stride, wptr = placed_draws(x, w, 0, 0)
    lo, hi, thr = np.zeros(3), np.ones(3), np.zeros(3, np.float32)
    user, builtin = model_of("mixture"), builtin_mixture()
    weighted_program, plain_program = program_of("mixture"), predictive_program_of("mixture")
    other = program_of("dis_and_kernel")                           # (2, 3, 3): another shape
    for rc, prog, model in ((ERR_KIND, plain_program, user), (ERR_KIND, weighted_program, builtin), (ERR_DIM, other, user), (0, weighted_program, user)):
        call(hip, user, ptr, stride, wptr, 70, 1.0, 0, 7, lo, hi, thr, expect=rc,
             fn=lambda *a: hip.glabc_rtc_weighted_predictive_counts(prog, C.byref(model), *a))
    # ... and the predictive entry points refuse a weighted program
    y = torch.empty(2, 70, device="cuda")
    assert hip.glabc_rtc_predictive_draws(weighted_program, C.byref(user), ptr, 1, 2, 70, stride, SEED, 0, 70, y.data_ptr(), 70, None, 0, None) == ERR_KIND
    for rc, kw in ((ERR_NULL, dict(wptr=None)), (ERR_DIM, dict(dim=3)), (ERR_ARG, dict(n=-1)), (ERR_ARG, dict(scale=0.0)), (ERR_ARG, dict(n_bins=513)),
                   (0, dict(n=0))):
        a = dict(wptr=wptr, dim=2, n=70, scale=1.0, n_bins=7)
        a.update(kw)
        call(hip, user, ptr, stride, a["wptr"], a["n"], a["scale"], 0, a["n_bins"], lo, hi, thr, expect=rc,
             fn=lambda x_, s_, d_, *rest: hip.glabc_rtc_weighted_predictive_counts(weighted_program, C.byref(user), x_, s_, a["dim"], *rest))


# ---------------------------------------------------------------------------------- CompiledModel and predictive.check_weighted
def nonlinear_model(source=NONLINEAR):
    return CompiledModel(3, 2, source, make_dist(("gauss", [0.0, 0.5, 0.0], [1.5, 1.0, 2.0])), [0.9, 0.6], 0.15, noise_dim=4)


@pytest.fixture(scope="module")
def population():
    g = torch.Generator().manual_seed(5)
    theta = (torch.tensor([0.0, 0.5, 0.0]) + torch.tensor([1.5, 1.0, 2.0]) * torch.randn(150, 3, generator=g)).cuda()
    w = (0.1 + 4.0 * torch.rand(150, generator=g)).cuda()
    w[4], theta[4] = 0.0, float("nan")
    w[64:128] = 0.0
    return theta, w


def test_the_self_check_passes_and_auto_is_the_fused_route(hip, population):
    theta, w = population
    cm = nonlinear_model()
    handle = cm.weighted_predictive_program()
    key = (CompiledModel.WEIGHTED_PREDICTIVE,)
    assert handle and key in cm._checked and cm.weighted_predictive_program() is handle
    assert cm.self_check_weighted_predictive(handle) is True
    assert (CompiledModel.PREDICTIVE,) in cm._programs              # the reference of the self-check: the existing program, untouched
    assert predictive._path_weighted(cm, theta, "auto").program is handle and predictive._path_weighted(cm, theta.cpu(), "auto") is None
    auto = predictive.check_weighted(cm, (theta, w), bins=7, seed=SEED)
    fused = predictive.check_weighted(cm, (theta, w), bins=7, seed=SEED, path="fused")
    for a, b in zip(auto, fused):
        assert np.array_equal(a, b)
    # the tables are sums of m over the draws predictive.simulate materialises with row0 = draw0
    m, scale = weighted.quantize(w)
    mult = [int(v) for v in m.cpu().tolist()]
    draw0 = 2 ** 40 + 5
    y, dis = predictive.simulate(cm, theta, seed=SEED, row0=draw0)
    stats = np.concatenate([host(y), host(dis)[:, None]], axis=1)
    lim = np.array([[-2.0, 6.0], [-3.0, 3.0], [0.0, 8.0]])
    t = predictive.terms_weighted(cm, (theta, w), bins=7, range=lim, seed=SEED, scale=scale, draw0=draw0)
    thr = np.array([0.9, 0.6, 0.15], np.float32)
    assert t.n == sum(mult) and np.array_equal(t.counts, WP.as_u64(WP.counts(stats, mult, 7, lim[:, 0], lim[:, 1])))
    assert np.array_equal(t.tails, WP.as_u64(WP.tails(stats, mult, thr)))
    parts = [predictive.terms_weighted(cm, (theta[a:b], w[a:b]), bins=7, range=lim, seed=SEED, scale=scale, draw0=draw0 + a)
             for a, b in ((0, 37), (37, 128), (128, 150))]
    both = predictive.combine_weighted(parts)
    assert both.n == t.n and np.array_equal(both.counts, t.counts) and np.array_equal(both.tails, t.tails)


def test_a_disagreeing_self_check_hands_no_program_out(hip, population, monkeypatch):
    theta, w = population
    cm = nonlinear_model()
    tables = predictive._torch_weighted_tables

    def wrong(*args, **kw):
        counts, tails = tables(*args, **kw)
        return counts + np.uint64(1), tails

    monkeypatch.setattr(predictive, "_torch_weighted_tables", wrong)
    with pytest.raises(SimulatorSelfCheckError, match="disagrees with the weighted sums"):
        cm.weighted_predictive_program()
    with pytest.raises(SimulatorSelfCheckError):                            # the verdict sticks
        cm.weighted_predictive_program()
    key = (CompiledModel.WEIGHTED_PREDICTIVE,)
    assert key not in cm._programs and key not in cm._checked
    monkeypatch.setattr(predictive, "_torch_weighted_tables", tables)       # the generic route counts with it
    with pytest.raises(SimulatorSelfCheckError):
        predictive.check_weighted(cm, (theta, w), bins=7, seed=SEED, path="fused")
    with pytest.warns(RuntimeWarning, match="generic path"):
        c = predictive.check_weighted(cm, (theta, w), bins=7, seed=SEED)
    assert c.n > 0 and c.distance_counts is not None and (c.y_counts.sum(axis=1) == c.n).all()


def test_a_program_that_fails_to_compile_warns_and_runs_generic(hip, population):
    """the source compiles in every other program of the Model and refuses this one: what the row kernels of the generic route need
    is there, the weighted predictive program is not"""
    theta, w = population
    cm = nonlinear_model("#ifdef GLABC_RTC_WEIGHTED_PREDICTIVE\n#error no weighted predictive program for this source\n#endif\n" + NONLINEAR)
    with pytest.raises(SimulatorCompileError, match="no weighted predictive program for this source"):
        cm.weighted_predictive_program()
    with pytest.raises(SimulatorCompileError):                              # not handed to the compiler again
        predictive.check_weighted(cm, (theta, w), bins=7, seed=SEED, path="fused")
    with pytest.warns(RuntimeWarning, match="generic path"):
        c = predictive.check_weighted(cm, (theta, w), bins=7, seed=SEED, scale=1.0)
    assert c.n == int(weighted.quantize(w, 1.0)[0].sum()) and (c.y_counts.sum(axis=1) == c.n).all() and c.distance_counts.sum() == c.n
    assert predictive.check(cm, theta[:4], bins=3, seed=SEED).n == 4        # the predictive program of the same source is untouched
