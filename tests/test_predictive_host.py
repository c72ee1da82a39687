"""Posterior predictive checks on the CPU: the restatement of glabc_predictive_draws / glabc_predictive_counts (tests/predictive_ref.py)
against plain NumPy -- numpy.histogram on the restated draws, comparisons, min and max --, the additivity of predictive.terms /
combine, the argument checks of glabcmcmc_amd/predictive.py, the generic path on a callback Model with CPU tensors, and the
refusals of both entry points, which launch nothing and so need no GPU.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import predictive_ref as P
import quantile_ref as Q
import rejection_ref as R
from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import distribution, predictive
from glabcmcmc_amd.examples.Mixture import Mixture_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x123456789ABCDEF1
ERR_NULL, ERR_DIM, ERR_KIND, ERR_ARG = -1, -2, -3, -4


def abs_model(d):
    prior = distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d))
    return R.abs_gauss_model(d, prior, epsilon=0.4 + 0.3 * d)


@functools.lru_cache(maxsize=None)
def restated(d=3, n_rows=11, n=70):
    """a sampler-like history with a NaN and an infinity, and its restated draws: computed once, never modified"""
    rng = np.random.default_rng(5)
    hist = (1.5 * rng.standard_normal((n_rows, d, n))).astype(np.float32)
    hist[3, 1, 7], hist[4, 0, 9] = np.nan, np.inf
    y, dis = P.restate(abs_model(d).descriptor(), hist, n, SEED, 2 ** 32 - 100, n + 3)
    for a in (hist, y, dis):
        a.setflags(write=False)
    return hist, y, dis


def test_restated_draws_are_the_simulator_on_restated_noise():
    hist, y, dis = restated()
    model = abs_model(3).descriptor()
    ids = P.ids_of(11, 70, 2 ** 32 - 100, 73)
    assert ids[0, 0] < 2 ** 32 <= ids[-1, -1] and len(np.unique(ids)) == ids.size
    eps = R.noise_normals((SEED ^ P.PREDICTIVE_KEY ^ R.NOISE_KEY) & R.M64, ids.reshape(-1), 3).reshape(11, 70, 3).transpose(0, 2, 1)
    scale = np.array([model.noise.p2[j] for j in range(3)], np.float32)[None, :, None]
    loc = np.array([model.noise.p0[j] for j in range(3)], np.float32)[None, :, None]
    with np.errstate(invalid="ignore"):
        want = np.abs(hist) + (loc + scale * eps)
        assert np.array_equal(np.isnan(want), np.isnan(y)) and np.array_equal(want[~np.isnan(want)], y[~np.isnan(y)])
        y_obs = np.array([model.y_obs[j] for j in range(3)], np.float64)[None, :, None]
        d64 = np.sqrt(((y.astype(np.float64) - y_obs) ** 2).sum(axis=1))
    finite = np.isfinite(d64)
    assert np.array_equal(finite, np.isfinite(dis)) and np.allclose(dis[finite], d64[finite], rtol=1e-6, atol=0)
    assert np.isnan(y[3, 1, 7]) and np.isnan(dis[3, 7]) and np.isinf(y[4, 0, 9]) and np.isinf(dis[4, 9])
    # another key than the rejection kernel's noise: the same ids give other normals
    assert not np.array_equal(R.noise_normals(SEED, ids.reshape(-1)[:8], 3), eps.transpose(0, 2, 1).reshape(-1, 3)[:8])


def test_restated_counts_against_numpy_histogram():
    _, y, dis = restated()
    stats = P.statistics(y, dis)
    assert stats.shape == (4, 770) and np.array_equal(stats[1], y[:, 1, :].reshape(-1), equal_nan=True) and np.array_equal(stats[3], dis.reshape(-1), equal_nan=True)
    for n_bins in (1, 2, 7, 64, 1024):
        lo, hi = np.array([0.5, 0.25, 0.3, 1.0]), np.array([3.0, 2.5, 3.0, 4.0])
        hi[0] = float(np.sort(stats[0][np.isfinite(stats[0])])[600])                      # a hi that is a value: the closed last bin
        got = P.counts(stats, n_bins, lo, hi)
        assert (got.sum(axis=1) == 770).all()
        for k in range(4):
            x = stats[k].astype(np.float64)
            ok = ~np.isnan(x)
            want, _ = np.histogram(x[ok], bins=n_bins, range=(lo[k], hi[k]))
            assert np.array_equal(got[k, :n_bins], want.astype(np.uint64)), (n_bins, k)
            assert got[k, n_bins] == (x[ok] < lo[k]).sum() and got[k, n_bins + 1] == (x[ok] > hi[k]).sum() and got[k, n_bins + 2] == (~ok).sum()
        assert got[0, n_bins - 1] > 0 and got[:, n_bins].all() and got[:, n_bins + 1].all() and got[1, n_bins + 2] == 1


def test_restated_tails_and_extremes_against_numpy():
    _, y, dis = restated()
    stats = P.statistics(y, dis)
    thr = np.array([1.5, stats[1][5], 1.3, stats[3][100]], np.float32)                   # two thresholds that are values
    t = P.tails(stats, thr)
    assert (t.sum(axis=1) == 770).all() and t[1, 1] >= 1 and t[3, 1] >= 1 and t[1, 3] == 1 and t[3, 3] == 1 and t[2, 3] == 0
    for k in range(4):
        x = stats[k][~np.isnan(stats[k])]
        assert t[k, 0] == (x < thr[k]).sum() and t[k, 2] == (x > thr[k]).sum()
    e = P.extremes(stats)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(Q.unkey(e[:, 0]), np.nanmin(stats, axis=1)) and np.array_equal(Q.unkey(e[:, 1]), np.nanmax(stats, axis=1))
    assert np.isinf(Q.unkey(e[:, 1])[0]) and np.isinf(Q.unkey(e[:, 1])[3])
    assert P.extremes(np.full((1, 5), np.nan, np.float32)).tolist() == [list(P.KEY_NONE)]
    zeros = P.extremes(np.array([[-0.0, 0.0]], np.float32))                               # -0 and +0 are one value
    assert zeros[0, 0] == zeros[0, 1] == 0x80000000


def restated_terms(y, dis, n_bins, lim, thr):
    stats = P.statistics(y, dis)
    return predictive.Terms(stats.shape[1], P.counts(stats, n_bins, lim[:, 0], lim[:, 1]), P.tails(stats, thr), lim, thr, True)


def test_terms_combine_and_summary_on_the_restatement():
    hist, y, dis = restated()
    model = abs_model(3).descriptor()
    lim = np.array([[0.0, 4.0], [0.0, 4.0], [-1.0, 3.0], [0.0, 6.0]])
    thr = np.array([1.5, 1.4, 1.3, 1.3], np.float32)
    whole = restated_terms(y, dis, 7, lim, thr)
    # two slabs of chains x two slices of rows, each restated on its own with the matching id0: the very draws of the whole
    parts = []
    for row0, rows in ((0, 4), (4, 7)):
        for chain0, k in ((0, 33), (33, 37)):
            py, pd = P.restate(model, hist[row0:row0 + rows, :, chain0:chain0 + k], k, SEED, 2 ** 32 - 100 + row0 * 73 + chain0, 73)
            assert np.array_equal(py.view(np.uint32), y[row0:row0 + rows, :, chain0:chain0 + k].view(np.uint32))
            parts.append(restated_terms(py, pd, 7, lim, thr))
    both = predictive.combine(parts)
    assert both.n == whole.n == 770 and np.array_equal(both.counts, whole.counts) and np.array_equal(both.tails, whole.tails)
    s = predictive.summary(both)
    assert s.n == 770 and s.y_counts.shape == (3, 7) and s.y_edges.shape == (3, 8) and s.y_outside.shape == (3, 3)
    assert s.distance_counts.shape == (7,) and s.distance_edges.shape == (8,) and s.distance_outside.shape == (3,)
    assert np.array_equal(s.y_edges[2], np.linspace(-1.0, 3.0, 8)) and np.array_equal(s.distance_edges, np.linspace(0.0, 6.0, 8))
    stats = P.statistics(y, dis)
    for j in range(3):
        x = stats[j][~np.isnan(stats[j])]
        assert s.p_upper[j] == (x >= thr[j]).sum() / x.size
        assert s.y_counts[j].sum() + s.y_outside[j].sum() == 770
    x = stats[3][~np.isnan(stats[3])]
    assert s.within_epsilon == (x <= thr[3]).sum() / x.size and np.array_equal(s.tails, whole.tails)
    with pytest.raises(ValueError):
        predictive.combine([])
    with pytest.raises(ValueError):
        predictive.combine([whole, restated_terms(y, dis, 8, lim, thr)])
    with pytest.raises(ValueError):
        predictive.combine([whole, restated_terms(y, dis, 7, lim + 1.0, thr)])
    with pytest.raises(ValueError):
        predictive.combine([whole, restated_terms(y, dis, 7, lim, thr + np.float32(1.0))])


# ---------------------------------------------------------------------------------- the Python layer
class CallbackModel:
    """a Model of callbacks only: no descriptor, y = theta^2 + noise, three outputs of two parameters"""
    theta_dim, y_dim, epsilon = 2, 3, 0.5
    y_obs = torch.tensor([[1.0, 1.0, 2.0]])

    def generate_samples(self, theta, num_samples=1):
        theta = theta.view(-1, 2)
        y = torch.stack([theta[:, 0] ** 2, theta[:, 1] ** 2, theta[:, 0] ** 2 + theta[:, 1] ** 2], dim=1)
        return y + 0.1 * torch.randn(y.shape)


class CallbackModelWithDistance(CallbackModel):
    def discrepancy(self, y):
        return torch.sqrt(((y.view(-1, 3) - self.y_obs) ** 2).sum(dim=1))


def test_generic_path_on_a_callback_model_with_cpu_tensors():
    rng = np.random.default_rng(2)
    history = torch.from_numpy(rng.standard_normal((9, 5, 2)).astype(np.float32))      # (T, C, D)
    state = torch.get_rng_state()
    c = predictive.check(CallbackModel(), history, bins=8, seed=3)
    assert torch.equal(torch.get_rng_state(), state)                                      # the seed is used inside a fork
    assert c.n == 45 and c.y_counts.shape == (3, 8) and (c.y_counts.sum(axis=1) == 45).all() and not c.y_outside.any()
    assert c.distance_counts is None and c.distance_edges is None and c.distance_outside is None and c.within_epsilon is None
    assert c.tails.shape == (3, 4) and (c.tails.sum(axis=1) == 45).all() and c.p_upper.shape == (3,)
    again = predictive.check(CallbackModel(), history, bins=8, seed=3)
    assert np.array_equal(again.y_counts, c.y_counts) and np.array_equal(again.y_edges, c.y_edges)
    c = predictive.check(CallbackModelWithDistance(), history, bins=4, range=[(0.0, 3.0), (0.0, 3.0), (0.0, 3.0), (0.0, 1.0)], seed=3,
                         path="generic")
    assert c.tails.shape == (4, 4) and c.distance_counts.shape == (4,) and 0.0 <= c.within_epsilon <= 1.0
    assert c.distance_counts.sum() + c.distance_outside.sum() == 45 and c.distance_outside[2] == 0
    assert np.array_equal(c.distance_edges, np.linspace(0.0, 1.0, 5))
    # the generic path's bin arithmetic is the restatement's: the same draws (the same seed) binned by quantile_ref
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(3)
        y = CallbackModelWithDistance().generate_samples(history.reshape(-1, 2), 1)
    stats = np.concatenate([y.numpy().T, CallbackModelWithDistance().discrepancy(y).numpy()[None]]).astype(np.float32)
    want = Q.histogram(stats[None], 4, [0.0, 0.0, 0.0, 0.0], [3.0, 3.0, 3.0, 1.0])
    assert np.array_equal(c.y_counts, want[:3, :4]) and np.array_equal(c.distance_counts, want[3, :4])
    assert np.array_equal(c.y_outside, want[:3, 4:]) and np.array_equal(c.tails, P.tails(stats, [1.0, 1.0, 2.0, 0.5]))
    # a descriptor Model on CPU tensors runs the generic path too ("auto" takes the kernel for a history on the GPU only)
    m = Mixture_set(0.3)
    c = predictive.check(m, torch.ones(6, 4, 2), bins=5, seed=1)
    assert c.n == 24 and (c.y_counts.sum(axis=1) == 24).all() and c.distance_counts.sum() == 24 and c.tails.shape == (3, 4)
    t1 = predictive.terms(m, torch.ones(6, 4, 2), bins=5, range=(-1.0, 4.0), seed=1)
    assert t1.has_distance and t1.counts.shape == (3, 8) and np.array_equal(t1.lim, np.tile([-1.0, 4.0], (3, 1)))


def test_argument_checks_of_the_python_layer():
    m = Mixture_set(0.3)
    h = torch.zeros(4, 3, 2)
    bad = [dict(bins=0), dict(bins=1025), dict(bins=2.5), dict(bins=True), dict(thresholds=[1.0, 2.0]), dict(thresholds=[1.0, np.nan, 2.0]),
           dict(range=(1.0, 1.0)), dict(range=[(0.0, 1.0)] * 2), dict(range=(0.0, np.inf)), dict(chain0=-1), dict(row0=-1), dict(chain0=2.0),
           dict(chain0=1, n_chains_total=3), dict(n_chains_total=0), dict(seed="x"), dict(seed=1.5), dict(path="fast"), dict(layout="columns")]
    for kw in bad:
        args = dict(seed=1)
        args.update(kw)
        with pytest.raises(ValueError):
            predictive.check(m, h, **args)
    with pytest.raises(ValueError):
        predictive.check(m, torch.zeros(4, 3, 3), seed=1)                                # theta_dim
    with pytest.raises(ValueError):
        predictive.check(m, torch.zeros(4), seed=1)
    with pytest.raises(ValueError):
        predictive.terms(m, h, range=None, seed=1)
    with pytest.raises(ValueError):
        predictive.check(CallbackModel(), h, seed=1, path="fused")
    with pytest.raises(ValueError):
        predictive.simulate(CallbackModel(), h, seed=1)
    assert predictive._ids(5, 0, None, 0) == (0, 5) and predictive._ids(5, 10, 64, 3) == (3 * 64 + 10, 64)
    assert predictive.accepted(m) is not None and predictive.accepted(CallbackModel()) is None
    import glabcmcmc_amd
    assert glabcmcmc_amd.predictive is predictive and "predictive" in glabcmcmc_amd.__all__


def test_abi_surface_and_the_key():
    assert len(A.ENTRY_POINTS["glabc_predictive_draws"][1]) == 14 and len(A.ENTRY_POINTS["glabc_predictive_counts"][1]) == 17
    assert A.VERSION == 301 and A.STREAM_LAYOUT == 2
    header = open(os.path.join(ROOT, "include", "glabc.h")).read()
    assert "#define GLABC_PREDICTIVE_KEY 0x%Xull" % P.PREDICTIVE_KEY in header and predictive.PREDICTIVE_KEY == P.PREDICTIVE_KEY
    assert "#define GLABC_MAX_PREDICTIVE_BINS %d" % predictive.MAX_BINS in header
    assert len({P.PREDICTIVE_KEY, R.NOISE_KEY, R.ACCEPT_KEY, 0}) == 4


def test_no_instantiation_has_a_private_segment():
    """profiles/predictive_kernel_resources.txt: the nine instantiations of predictive_kernel, none with a private segment or a
    spilled vector register"""
    import re
    text = open(os.path.join(ROOT, "profiles", "predictive_kernel_resources.txt")).read()
    names = re.findall(r"Function Name: (\S+)", text)
    assert len(names) == 9 and all("predictive_kernel" in n for n in names) and len(set(names)) == 9
    assert re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text) == ["0"] * 9 and re.findall(r"VGPRs Spill: (\d+)", text) == ["0"] * 9
    assert re.findall(r"Dynamic Stack: (\w+)", text) == ["False"] * 9


def test_refusals_in_order_launch_nothing():
    """a refused call launches nothing and touches no pointer, so the order of the refusals can be walked without a GPU: every
    pointer here is a host array"""
    hip = A.lib()
    m = abs_model(3).descriptor()
    gk = __import__("glabcmcmc_amd.examples.GK", fromlist=["GK_set"]).GK_set(200.0).descriptor()
    user, wrong, unknown = abs_model(3).descriptor(), abs_model(3).descriptor(), abs_model(3).descriptor()
    user.sim_kind, wrong.y_dim, unknown.sim_kind = A.SIM_USER, 2, 77
    buf = np.zeros(64, np.float32)
    h = y = d = buf.ctypes.data
    M = C.byref(m)

    def draws(model=M, hist=h, n_rows=2, dim=3, n=4, stride=4, id0=0, step=4, y_out=y, ys=4, d_out=d, ds=4):
        return hip.glabc_predictive_draws(model, hist, n_rows, dim, n, stride, 0, id0, step, y_out, ys, d_out, ds, None)

    top = 2 ** 63 - 1
    for rc, kw in ((ERR_NULL, dict(model=None, dim=9)), (ERR_NULL, dict(hist=None, n_rows=0)), (ERR_NULL, dict(y_out=None, d_out=None, dim=9)),
                   (ERR_DIM, dict(dim=2, n_rows=0)), (ERR_DIM, dict(dim=4)), (ERR_DIM, dict(model=C.byref(wrong), n=-1)),
                   (ERR_DIM, dict(model=C.byref(gk), dim=8)), (ERR_DIM, dict(model=C.byref(user), dim=2)),
                   (ERR_KIND, dict(model=C.byref(user), n_rows=0)), (ERR_KIND, dict(model=C.byref(unknown), n=-1)),
                   (ERR_ARG, dict(n_rows=0)), (ERR_ARG, dict(n=-1)), (ERR_ARG, dict(stride=3)), (ERR_ARG, dict(ys=3)), (ERR_ARG, dict(ds=3)),
                   (ERR_ARG, dict(id0=-1)), (ERR_ARG, dict(step=3)), (ERR_ARG, dict(id0=top - 6)), (ERR_ARG, dict(step=top)),
                   (ERR_ARG, dict(id0=top, n_rows=1, n=2, stride=2, step=2)),
                   (0, dict(n=0)), (0, dict(n=0, stride=0, ys=0, ds=0, step=0)), (0, dict(n=0, y_out=None, ys=-5)), (0, dict(n=0, d_out=None, ds=-5))):
        assert draws(**kw) == rc, kw
    assert not buf.any()

    lo, hi, thr = np.zeros(4), np.ones(4), np.zeros(4, np.float32)
    nan_lo, inf_hi, nan_thr = np.array([0.0, 0.0, 0.0, np.nan]), np.array([1.0, 1.0, np.inf, 1.0]), np.array([0, 0, 0, np.nan], np.float32)
    out = np.zeros(4 * 11, np.uint64)
    c = t = e = out.ctypes.data

    def counts(model=M, hist=h, n_rows=2, dim=3, n=4, stride=4, id0=0, step=4, bins=8, lo=lo, hi=hi, thr=thr, c=c, t=t, e=e):
        p = lambda a: None if a is None else a.ctypes.data          # noqa: E731
        return hip.glabc_predictive_counts(model, hist, n_rows, dim, n, stride, 0, id0, step, bins, p(lo), p(hi), p(thr), c, t, e, None)

    for rc, kw in ((ERR_NULL, dict(model=None, dim=9)), (ERR_NULL, dict(hist=None, n_rows=0)), (ERR_NULL, dict(c=None, t=None, e=None, dim=9)),
                   (ERR_NULL, dict(lo=None, dim=9)), (ERR_NULL, dict(hi=None, n_rows=0)), (ERR_NULL, dict(thr=None, bins=0)),
                   (ERR_DIM, dict(dim=2, n_rows=0)), (ERR_DIM, dict(model=C.byref(wrong), bins=0)), (ERR_KIND, dict(model=C.byref(user), bins=0)),
                   (ERR_ARG, dict(n_rows=0)), (ERR_ARG, dict(n=-1)), (ERR_ARG, dict(stride=3)), (ERR_ARG, dict(id0=-1)), (ERR_ARG, dict(step=3)),
                   (ERR_ARG, dict(id0=top - 6)), (ERR_ARG, dict(bins=0)), (ERR_ARG, dict(bins=1025)), (ERR_ARG, dict(lo=hi, hi=lo)),
                   (ERR_ARG, dict(lo=lo, hi=lo)), (ERR_ARG, dict(lo=nan_lo)), (ERR_ARG, dict(hi=inf_hi)), (ERR_ARG, dict(thr=nan_thr)),
                   (0, dict(n=0)), (0, dict(n=0, stride=0, step=0)),
                   # what only a NULL output needs is not looked at
                   (0, dict(n=0, c=None, lo=None, hi=None, bins=0)), (0, dict(n=0, t=None, thr=None)), (0, dict(n=0, c=None, lo=nan_lo, bins=-1)),
                   (0, dict(n=0, t=None, thr=nan_thr)), (0, dict(n=0, c=None, t=None)), (0, dict(n=0, e=None))):
        assert counts(**kw) == rc, kw
    assert not out.any()
