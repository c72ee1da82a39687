"""Weighted posterior predictive checks on the CPU: the restatement of glabc_weighted_predictive_counts
(tests/weighted_predictive_ref.py) against numpy.histogram(weights=m) and plain comparisons, the refusals of the entry point and of its
run-time compiled twin in the stated order (they launch nothing and so need no GPU), the grid rule's static_asserts and the
compiler's resource report as files, and predictive.check_weighted / terms_weighted / combine_weighted / summary on the generic path.
"""
import ctypes as C
import functools
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import predictive_ref as P
import rejection_ref as R
import weighted_predictive_ref as WP
from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import distribution, predictive, weighted
from glabcmcmc_amd.examples.Mixture import Mixture_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gl-abc-mcmc_amd", "csrc")
SEED = 0x123456789ABCDEF1
ERR_NULL, ERR_DIM, ERR_KIND, ERR_ARG = -1, -2, -3, -4


def abs_model(d):
    prior = distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d))
    return R.abs_gauss_model(d, prior, epsilon=0.4 + 0.3 * d)


@functools.lru_cache(maxsize=None)
def restated(d=3, n=150):
    """draws with a NaN of no weight, a NaN and an infinity of positive weight, weights of every kind, their restated statistics and
    multiplicities: computed once, never modified"""
    rng = np.random.default_rng(11)
    x = (1.5 * rng.standard_normal((d, n + 6))).astype(np.float32)
    w = rng.uniform(0.5, 9.0, n).astype(np.float32)
    x[:, 4], w[4] = np.nan, 0.0                       # skipped, whatever theta holds
    x[1, 9], x[0, 12] = np.nan, np.inf                # counted: the NaN slot, the slot above
    w[20], w[21], w[22] = 0.5, 1.5, 2.5               # ties under scale 1: 0, 2, 2
    w[30], w[31] = -3.0, np.nan                       # m = 0
    w[40] = 0.25                                      # rounds to 0
    w[50], w[51] = 2.0 ** 31, 2.0 ** 31               # 2^31 each
    w[60] = 2.0 ** 33                                 # clamped at 2^32 - 1
    stats = WP.statistics(abs_model(d).descriptor(), x, n, SEED, 2 ** 32 - 40)
    m = WP.multiplicity(w, 1.0)
    for a in (x, w, stats):
        a.setflags(write=False)
    return x, w, stats, tuple(m)


def test_restated_multiplicities_and_draws():
    x, w, stats, m = restated()
    assert [m[i] for i in (4, 20, 21, 22, 30, 31, 40, 50, 51, 60)] == [0, 0, 2, 2, 0, 0, 0, 2 ** 31, 2 ** 31, 2 ** 32 - 1]
    assert all(isinstance(c, int) for c in m) and sum(m) > 2 ** 33
    # the draws are predictive_ref's on the one-row history: draw i has the id id0 + i, whatever lies behind column n
    y, dis = P.restate(abs_model(3).descriptor(), x[None, :, :150], 150, SEED, 2 ** 32 - 40, 150)
    assert np.array_equal(stats[:, :3].view(np.uint32), y[0].T.view(np.uint32)) and np.array_equal(stats[:, 3].view(np.uint32), dis[0].view(np.uint32))
    part = WP.statistics(abs_model(3).descriptor(), x[:, 70:], 80, SEED, 2 ** 32 - 40 + 70)
    assert np.array_equal(part.view(np.uint32), stats[70:].view(np.uint32))
    assert np.isnan(stats[4]).all() and np.isnan(stats[9, 1]) and np.isnan(stats[9, 3]) and np.isinf(stats[12, 0])


def test_restated_counts_against_numpy_histogram_with_weights():
    _, _, stats, m = restated()
    mf = np.array(m, np.float64)                       # exact: every m is below 2^53
    keep = np.array(m) > 0
    for n_bins in (1, 2, 7, 64, 512):
        lo, hi = np.array([0.5, 0.25, 0.3, 1.0]), np.array([3.0, 2.5, 3.0, 4.0])
        hi[0] = float(np.sort(stats[:, 0][np.isfinite(stats[:, 0]) & keep])[100])          # a hi that is a counted value: the closed last bin
        got = WP.counts(stats, m, n_bins, lo, hi)
        assert all(sum(row) == sum(m) for row in got)
        for k in range(4):
            x = stats[:, k].astype(np.float64)
            ok = ~np.isnan(x) & keep
            want, _ = np.histogram(x[ok], bins=n_bins, range=(lo[k], hi[k]), weights=mf[ok])
            assert [float(v) for v in got[k][:n_bins]] == want.tolist(), (n_bins, k)
            assert got[k][n_bins] == int(mf[ok & (x < lo[k])].sum()) and got[k][n_bins + 1] == int(mf[ok & (x > hi[k])].sum())
            assert got[k][n_bins + 2] == sum(c for c, v in zip(m, x) if c > 0 and np.isnan(v))
        assert got[1][n_bins + 2] == m[9] and got[0][n_bins + 2] == 0          # the NaN of weight 0 is in no slot
    assert np.array_equal(WP.as_u64(got), np.array(got, dtype=object).astype(np.uint64))


def test_restated_tails_and_extremes_against_plain_comparisons():
    _, _, stats, m = restated()
    keep = np.array(m) > 0
    thr = np.array([1.5, stats[22, 1], 1.3, stats[50, 3]], np.float32)                     # two thresholds that are counted values
    t = WP.tails(stats, m, thr)
    assert all(sum(row) == sum(m) for row in t)
    assert t[1][1] >= m[22] and t[3][1] >= 2 ** 31 and t[1][3] == m[9] == t[3][3] and t[0][3] == 0 == t[2][3]
    for k in range(4):
        x = stats[:, k]
        with np.errstate(invalid="ignore"):
            assert t[k][0] == sum(c for c, v in zip(m, x) if v < thr[k]) and t[k][2] == sum(c for c, v in zip(m, x) if v > thr[k])
    e = WP.extremes(stats, m)
    import quantile_ref as Q
    with np.errstate(invalid="ignore"):
        assert np.array_equal(Q.unkey(e[:, 0]), np.nanmin(stats[keep], axis=0)) and np.array_equal(Q.unkey(e[:, 1]), np.nanmax(stats[keep], axis=0))
    # a draw of multiplicity 0 is in no extreme: give the smallest value no weight
    j = int(np.nanargmin(np.where(keep, stats[:, 2], np.nan)))
    m2 = list(m)
    m2[j] = 0
    assert Q.unkey(WP.extremes(stats, m2)[2:3, 0])[0] > stats[j, 2]
    assert WP.extremes(stats, [0] * len(m)).tolist() == [list(WP.KEY_NONE)] * 4


# ---------------------------------------------------------------------------------- the entry points without a GPU
def test_abi_surface_and_the_limits():
    names = ("glabc_weighted_predictive_counts", "glabc_rtc_compile_weighted_predictive", "glabc_rtc_weighted_predictive_counts")
    assert set(names) <= set(A.ENTRY_POINTS) and A.VERSION == 301 and A.STREAM_LAYOUT == 2
    assert [len(A.ENTRY_POINTS[k][1]) for k in names] == [17, 7, 18]
    assert A.ENTRY_POINTS[names[1]] == A.ENTRY_POINTS["glabc_rtc_compile_predictive"]
    header = open(os.path.join(ROOT, "include", "glabc.h")).read()
    assert "#define GLABC_MAX_WEIGHTED_PREDICTIVE_BINS %d" % predictive.MAX_WEIGHTED_BINS in header and predictive.MAX_WEIGHTED_BINS == 512
    assert 9 * (512 + 3 + 4) * 8 == 37368 <= 48 * 1024 < 9 * (1024 + 3 + 4) * 8
    lib = A.lib()
    for name in names:
        assert getattr(lib, name).argtypes == A.ENTRY_POINTS[name][1]


def test_refusals_in_order_launch_nothing():
    """a refused call launches nothing and touches no pointer, so the order of the refusals can be walked without a GPU: every
    pointer here is a host array, and the canaries around the outputs stay"""
    hip = A.lib()
    m = abs_model(3).descriptor()
    gk = __import__("glabcmcmc_amd.examples.GK", fromlist=["GK_set"]).GK_set(200.0).descriptor()
    user, wrong, unknown = abs_model(3).descriptor(), abs_model(3).descriptor(), abs_model(3).descriptor()
    user.sim_kind, wrong.y_dim, unknown.sim_kind = A.SIM_USER, 2, 77
    buf = np.zeros(64, np.float32)
    x = wt = buf.ctypes.data
    M = C.byref(m)
    lo, hi, thr = np.zeros(4), np.ones(4), np.zeros(4, np.float32)
    nan_lo, inf_hi, nan_thr = np.array([0.0, 0.0, 0.0, np.nan]), np.array([1.0, 1.0, np.inf, 1.0]), np.array([0, 0, 0, np.nan], np.float32)
    canary = np.uint64(0xDEADC0DEDEADBEEF)
    out = np.full(4 * 11 + 16, canary, np.uint64)
    c = t = e = out.ctypes.data + 64

    def counts(model=M, x=x, stride=4, dim=3, w=wt, n=4, scale=1.0, id0=0, bins=8, lo=lo, hi=hi, thr=thr, c=c, t=t, e=e):
        p = lambda a: None if a is None else a.ctypes.data          # noqa: E731
        return hip.glabc_weighted_predictive_counts(model, x, stride, dim, w, n, scale, 0, id0, bins, p(lo), p(hi), p(thr), c, t, e, None)

    top = 2 ** 63 - 1
    for rc, kw in ((ERR_NULL, dict(model=None, dim=9)), (ERR_NULL, dict(x=None, n=-1)), (ERR_NULL, dict(w=None, dim=9)),
                   (ERR_NULL, dict(w=None, scale=0.0)), (ERR_NULL, dict(c=None, t=None, e=None, dim=9)),
                   (ERR_NULL, dict(lo=None, dim=9)), (ERR_NULL, dict(hi=None, n=-1)), (ERR_NULL, dict(thr=None, bins=0)),
                   (ERR_DIM, dict(dim=2, n=-1)), (ERR_DIM, dict(dim=4, scale=0.0)), (ERR_DIM, dict(model=C.byref(wrong), bins=0)),
                   (ERR_DIM, dict(model=C.byref(gk), dim=8)), (ERR_DIM, dict(model=C.byref(user), dim=2)),
                   (ERR_KIND, dict(model=C.byref(user), n=-1)), (ERR_KIND, dict(model=C.byref(unknown), scale=0.0)),
                   (ERR_ARG, dict(n=-1)), (ERR_ARG, dict(n=2 ** 31 + 1, stride=2 ** 31 + 1)), (ERR_ARG, dict(stride=3)),
                   (ERR_ARG, dict(scale=0.0)), (ERR_ARG, dict(scale=-1.0)), (ERR_ARG, dict(scale=float("inf"))), (ERR_ARG, dict(scale=float("nan"))),
                   (ERR_ARG, dict(id0=-1)), (ERR_ARG, dict(id0=top - 2)), (ERR_ARG, dict(id0=top, n=2, stride=2)),
                   (ERR_ARG, dict(bins=0)), (ERR_ARG, dict(bins=513)), (ERR_ARG, dict(bins=1024)), (ERR_ARG, dict(lo=hi, hi=lo)),
                   (ERR_ARG, dict(lo=lo, hi=lo)), (ERR_ARG, dict(lo=nan_lo)), (ERR_ARG, dict(hi=inf_hi)), (ERR_ARG, dict(thr=nan_thr)),
                   # no draws: GLABC_OK, nothing launched
                   (0, dict(n=0)), (0, dict(n=0, stride=0)), (0, dict(n=0, id0=top)), (0, dict(n=0, bins=512)),
                   # what only a NULL output needs is not looked at
                   (0, dict(n=0, c=None, lo=None, hi=None, bins=0)), (0, dict(n=0, t=None, thr=None)), (0, dict(n=0, c=None, lo=nan_lo, bins=-1)),
                   (0, dict(n=0, c=None, bins=513)), (0, dict(n=0, t=None, thr=nan_thr)), (0, dict(n=0, c=None, t=None)), (0, dict(n=0, e=None))):
        assert counts(**kw) == rc, kw
    assert not buf.any() and (out == canary).all()

    # the run-time compiled twin: a NULL program first; a refused call never reaches a program's kernels
    def rtc(program=None, **kw):
        a = dict(model=M, x=x, stride=4, dim=3, w=wt, n=4, scale=1.0, id0=0, bins=8)
        a.update(kw)
        return hip.glabc_rtc_weighted_predictive_counts(program, a["model"], a["x"], a["stride"], a["dim"], a["w"], a["n"], a["scale"], 0, a["id0"],
                                                        a["bins"], lo.ctypes.data, hi.ctypes.data, thr.ctypes.data, c, t, e, None)
    assert rtc() == ERR_NULL and rtc(model=None) == ERR_NULL and rtc(n=-1) == ERR_NULL
    handle = C.c_void_p()
    log = C.create_string_buffer(256)
    assert hip.glabc_rtc_compile_weighted_predictive(None, 2, 2, 2, C.byref(handle), log, len(log)) == ERR_NULL
    assert hip.glabc_rtc_compile_weighted_predictive(b"x", 2, 2, 2, None, log, len(log)) == ERR_NULL
    for dims in ((0, 2, 2), (9, 2, 2), (2, 0, 2), (2, 9, 2), (2, 2, 0), (2, 2, 9)):
        assert hip.glabc_rtc_compile_weighted_predictive(b"x", *dims, C.byref(handle), log, len(log)) == ERR_DIM
    assert handle.value is None and (out == canary).all()


def test_the_grid_rule_is_pinned_by_static_asserts():
    text = open(os.path.join(CSRC, "glabc_weighted_predictive.hip")).read()
    asserts = re.findall(r"static_assert\((.*?)\);", text, flags=re.S)
    grid = [a for a in asserts if "weighted_predictive_grid(" in a]
    assert len(grid) >= 3 and sum(a.count("weighted_predictive_grid(") for a in grid) >= 10
    assert any("8 * 64 * 16 + 1" in a for a in grid) and any("<< 31" in a for a in grid)
    header = open(os.path.join(CSRC, "glabc_weighted_predictive.h")).read()
    assert "constexpr unsigned weighted_predictive_grid(" in header and "workgroups_per_cu(lds_bytes)" in header
    pack = open(os.path.join(CSRC, "glabc_weighted_predictive_pack.h")).read()
    assert "37368" in pack and "static_assert" in pack          # the largest table needs no grant
    # one text for the quantised weight, in a header a run-time compiled program is given
    walk = open(os.path.join(CSRC, "glabc_weighted_walk.h")).read()
    slots = open(os.path.join(CSRC, "glabc_slots.h")).read()
    assert walk.count("weight_multiplicity(float w, double scale)") == 1 and "weight_multiplicity(float" not in slots
    assert '#include "glabc_weighted_walk.h"' in slots and "glabc_check.h" not in walk and "<c" not in walk


def test_no_instantiation_has_a_private_segment():
    """profiles/weighted_predictive_kernel_resources.txt: the nine instantiations of weighted_predictive_kernel, none with a private
    segment or a spilled vector register"""
    text = open(os.path.join(ROOT, "profiles", "weighted_predictive_kernel_resources.txt")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 9 and all("weighted_predictive_kernel" in n for n in names) and len(set(names)) == 9
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 9 and re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 9
    assert re.findall(r"Dynamic Stack: (\w+)", text) == ["False"] * 9


# ---------------------------------------------------------------------------------- the Python layer
class CallbackModel:
    """a Model of callbacks only: no descriptor, y = theta^2 + noise, three outputs of two parameters, with a distance"""
    theta_dim, y_dim, epsilon = 2, 3, 0.5
    y_obs = torch.tensor([[1.0, 1.0, 2.0]])

    def generate_samples(self, theta, num_samples=1):
        theta = theta.view(-1, 2)
        y = torch.stack([theta[:, 0] ** 2, theta[:, 1] ** 2, theta[:, 0] ** 2 + theta[:, 1] ** 2], dim=1)
        return y + 0.1 * torch.randn(y.shape)

    def discrepancy(self, y):
        return torch.sqrt(((y.view(-1, 3) - self.y_obs) ** 2).sum(dim=1))


class NoDistanceModel(CallbackModel):
    discrepancy = None


def generic_draws(n=77):
    rng = np.random.default_rng(3)
    theta = torch.from_numpy(rng.standard_normal((n, 2)).astype(np.float32))
    w = torch.from_numpy(rng.uniform(0.1, 4.0, n).astype(np.float32))
    theta[5], w[5] = float("nan"), 0.0
    w[9] = 2.5
    return theta, w


def test_generic_route_on_cpu_tensors_against_the_restatement():
    theta, w = generic_draws()
    Model = CallbackModel()
    state = torch.get_rng_state()
    lim = [(0.0, 3.0), (0.0, 3.0), (0.0, 3.0), (0.0, 1.0)]
    c = predictive.check_weighted(Model, (theta, w), bins=4, range=lim, seed=3, scale=2.0, path="generic")
    assert torch.equal(torch.get_rng_state(), state)                                      # the seed is used inside a fork
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(3)
        y = Model.generate_samples(theta, 1)
    stats = np.concatenate([y.numpy(), Model.discrepancy(y).numpy()[:, None]], axis=1).astype(np.float32)
    m = WP.multiplicity(w.numpy(), 2.0)
    assert m[5] == 0 and m[9] == 5 and np.isnan(stats[5]).all()
    want = WP.as_u64(WP.counts(stats, m, 4, [r[0] for r in lim], [r[1] for r in lim]))
    assert c.n == sum(m) and np.array_equal(c.y_counts, want[:3, :4]) and np.array_equal(c.y_outside, want[:3, 4:])
    assert np.array_equal(c.distance_counts, want[3, :4]) and np.array_equal(c.distance_outside, want[3, 4:]) and not want[:, 6].any()
    tails = WP.tails(stats, m, [1.0, 1.0, 2.0, 0.5])
    assert np.array_equal(c.tails, WP.as_u64(tails))
    for j in range(3):
        assert c.p_upper[j] == (tails[j][1] + tails[j][2]) / sum(m)
    assert c.within_epsilon == (tails[3][0] + tails[3][1]) / sum(m)
    # "auto" on CPU tensors is the generic route; range=None: the exact extremes over the draws of positive multiplicity
    auto = predictive.check_weighted(Model, (theta, w), bins=4, seed=3, scale=2.0)
    e = WP.extremes(stats, m)
    import quantile_ref as Q
    assert np.array_equal(auto.y_edges[:, 0], Q.unkey(e[:3, 0]).astype(np.float64)) and auto.distance_edges[-1] == float(Q.unkey(e[3:, 1])[0])
    assert (auto.y_counts.sum(axis=1) == sum(m)).all() and not auto.y_outside.any()
    # the default scale is quantize's; unit weights through None, a Population-shaped and a Rejection-shaped object
    default = predictive.check_weighted(Model, (theta, w), bins=4, range=lim, seed=3)
    assert default.n == int(weighted.quantize(w)[0].sum())
    import collections
    Pop = collections.namedtuple("Pop", "theta weights")
    Rej = collections.namedtuple("Rej", "theta y distance")
    keep = torch.ones(77, dtype=torch.bool)
    keep[5] = False
    assert predictive.check_weighted(Model, Pop(theta, w), bins=4, range=lim, seed=3).n == default.n
    unit = predictive.check_weighted(Model, Rej(theta[keep], None, None), bins=4, range=lim, seed=3, scale=1.0)
    pair = predictive.check_weighted(Model, (theta[keep], None), bins=4, range=lim, seed=3, scale=1.0)
    plain = predictive.check(Model, theta[keep], bins=4, range=lim, seed=3)
    assert unit.n == pair.n == plain.n == 76
    for a, b, p in zip(unit, pair, plain):
        assert np.array_equal(a, b) and np.array_equal(a, p)
    # a Model without a distance has K = y_dim statistics
    nd = predictive.check_weighted(NoDistanceModel(), (theta, w), bins=4, range=lim[:3], seed=3, scale=2.0)
    assert nd.distance_counts is None and nd.within_epsilon is None and np.array_equal(nd.y_counts, c.y_counts)
    # a descriptor Model on CPU tensors runs the generic route too
    d = predictive.check_weighted(Mixture_set(0.3), (torch.ones(6, 2), torch.arange(6.0)), bins=5, seed=1, scale=1.0)
    assert d.n == 15 and (d.y_counts.sum(axis=1) == 15).all() and d.tails.shape == (3, 4)


def test_terms_add_over_ragged_shards_on_the_generic_route(monkeypatch):
    """the shards of a generic run use torch's generator, so they are built from one pre-simulated array of statistics"""
    theta, w = generic_draws(150)
    rng = np.random.default_rng(8)
    stats = torch.from_numpy(rng.standard_normal((150, 4)).astype(np.float32))
    stats[17, 2] = float("nan")
    first = {}

    def fake(Model, history, layout, seed):
        i0 = first["draw0"]
        assert layout == "rows" and np.array_equal(history.numpy(), theta[i0:i0 + history.shape[0]].numpy(), equal_nan=True)
        return stats[i0:i0 + history.shape[0]], True

    monkeypatch.setattr(predictive, "_generic_stats", fake)
    lim, thr = np.array([[-1.0, 1.0]] * 4), [0.0, 0.1, float(stats[3, 2]), -0.2]
    first["draw0"] = 0
    whole = predictive.terms_weighted(CallbackModel(), (theta, w), bins=6, range=lim, thresholds=thr, seed=1, scale=3.0)
    m = WP.multiplicity(w.numpy(), 3.0)
    assert isinstance(whole.n, int) and whole.n == sum(m) and whole.n_draws == 150 and whole.scale == 3.0
    assert np.array_equal(whole.counts, WP.as_u64(WP.counts(stats.numpy(), m, 6, lim[:, 0], lim[:, 1])))
    assert np.array_equal(whole.tails, WP.as_u64(WP.tails(stats.numpy(), m, thr))) and whole.tails[2, 1] >= m[3] and whole.tails[2, 3] == m[17]
    for cuts in ((0, 61, 150), (0, 1, 64, 150)):
        parts = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            first["draw0"] = a
            parts.append(predictive.terms_weighted(CallbackModel(), (theta[a:b], w[a:b]), bins=6, range=lim, thresholds=thr, seed=1, scale=3.0,
                                                   draw0=a))
        both = predictive.combine_weighted(parts)
        assert both.n == whole.n and both.n_draws == 150 and both.scale == 3.0 and both.has_distance
        assert np.array_equal(both.counts, whole.counts) and np.array_equal(both.tails, whole.tails)
        for got, ref in zip(predictive.summary(both), predictive.summary(whole)):
            assert np.array_equal(got, ref)
    # combine_weighted refuses shards that differ in scale, range or bins
    first["draw0"] = 0
    other = lambda **kw: predictive.terms_weighted(CallbackModel(), (theta, w), **dict(dict(bins=6, range=lim, thresholds=thr, seed=1, scale=3.0), **kw))  # noqa: E731
    for kw in (dict(scale=2.0), dict(range=lim + 1.0), dict(bins=7), dict(thresholds=[0.0, 0.1, 0.2, 0.3])):
        with pytest.raises(ValueError):
            predictive.combine_weighted([whole, other(**kw)])
    with pytest.raises(ValueError):
        predictive.combine_weighted([])
    with pytest.raises(ValueError):
        predictive.terms_weighted(CallbackModel(), (theta, w), bins=6, range=None, seed=1, scale=3.0)
    with pytest.raises(ValueError):
        predictive.terms_weighted(CallbackModel(), (theta, w), bins=6, range=lim, seed=1, scale=None)


def test_bad_weights_are_refused_in_quantizes_words():
    theta = torch.zeros(4, 2)
    for w, scale in (([1.0, float("nan"), 1.0, 1.0], None), ([1.0, float("inf"), 1.0, 1.0], None), ([1.0, -1.0, 1.0, 1.0], None),
                     ([0.0, 0.0, 0.0, 0.0], None), ([1.0, 2.0, 3.0, 4.0], 2.0 ** 31), ([1.0, 2.0, 3.0, 4.0], 0.0), ([1.0, 2.0, 3.0, 4.0], "x")):
        with pytest.raises(ValueError) as want:
            weighted.quantize(torch.tensor(w), scale)
        for path in ("generic", "auto"):
            with pytest.raises(ValueError) as got:
                predictive.check_weighted(Mixture_set(0.3), (theta, torch.tensor(w)), seed=1, scale=scale, path=path)
            assert str(got.value) == str(want.value)
    with pytest.raises(ValueError):
        predictive.check_weighted(Mixture_set(0.3), (theta, torch.ones(3)), seed=1)      # one weight per draw
    with pytest.raises(ValueError):
        predictive.check_weighted(Mixture_set(0.3), theta, seed=1)                        # no draws object
    with pytest.raises(ValueError):
        predictive.check_weighted(Mixture_set(0.3), (torch.zeros(4, 3), None), seed=1)   # theta_dim


def test_argument_checks_and_bins_above_512_on_both_routes():
    m = Mixture_set(0.3)
    draws = (torch.zeros(4, 2), torch.ones(4))
    for path in ("generic", "auto", "fused"):
        for bins in (513, 1024, 0, 2.5, True):
            with pytest.raises(ValueError, match="bins must be an integer in 1..512"):
                predictive.check_weighted(m, draws, bins=bins, seed=1, path=path)
    assert predictive.check_weighted(m, draws, bins=512, seed=1, path="generic").y_counts.shape == (2, 512)
    for kw in (dict(thresholds=[1.0, 2.0]), dict(thresholds=[1.0, np.nan, 2.0]), dict(range=(1.0, 1.0)), dict(range=[(0.0, 1.0)] * 2),
               dict(draw0=-1), dict(draw0=1.5), dict(seed="x"), dict(path="fast")):
        args = dict(seed=1)
        args.update(kw)
        with pytest.raises(ValueError):
            predictive.check_weighted(m, draws, **args)
    with pytest.raises(ValueError):
        predictive.check_weighted(CallbackModel(), (torch.zeros(4, 2), None), seed=1, path="fused")      # no kernel for callbacks
    with pytest.raises(ValueError):
        predictive.check_weighted(m, draws, seed=1, path="fused")                                          # nor for CPU tensors


def test_summary_of_weighted_terms_past_2_to_the_53():
    """M = 2^55 + 3 is no float64 (float64 arithmetic on it gives 2^54 / (2^55 - 4) for the first p-value); Check.n keeps it, and the
    p-values are the correctly rounded ratios of the integers: here exact binary fractions of M less the NaNs"""
    big = 2 ** 55 + 3
    counts = np.zeros((3, 5), np.uint64)
    counts[:, 0], counts[:, 1], counts[:, 4] = 2 ** 54, 2 ** 54, 3
    tails = np.array([[2 ** 54, 0, 2 ** 54, 3], [2 ** 53, 2 ** 53, 2 ** 54, 3], [2 ** 54 + 2 ** 53, 0, 2 ** 53, 3]], np.uint64)
    t = predictive.WeightedTerms(big, counts, tails, np.array([[0.0, 1.0]] * 3), np.zeros(3, np.float32), True, 2.0 ** 20, 1000)
    assert t._fields[:6] == predictive.Terms._fields and t._fields[6:] == ("scale", "n_draws")
    s = predictive.summary(t)
    assert s.n == big and isinstance(s.n, int) and float(big) != big
    assert s.p_upper.tolist() == [0.5, 0.75] and s.within_epsilon == 0.75
    assert Fraction(int(tails[1, 1]) + int(tails[1, 2]), big - 3) == Fraction(3, 4)
    assert np.array_equal(s.y_counts, counts[:2, :2]) and s.distance_outside.tolist() == [0, 0, 3] and np.array_equal(s.tails, tails)
    both = predictive.combine_weighted([t, t])
    assert both.n == 2 * big and both.n_draws == 2000 and int(both.tails[0, 0]) == 2 ** 55


def test_module_surface():
    import glabcmcmc_amd
    for name in ("check_weighted", "terms_weighted", "combine_weighted", "WeightedTerms"):
        assert hasattr(glabcmcmc_amd.predictive, name), name
    from glabcmcmc_amd.compiled import CompiledModel
    assert callable(CompiledModel.weighted_predictive_program) and callable(CompiledModel.self_check_weighted_predictive)
    assert "weighted predictive checks" not in weighted.__doc__ and "check_weighted" in predictive.__doc__
