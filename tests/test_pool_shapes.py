"""The pool side of the library -- KernelDensity (what AGLMCMC runs on) and the GLMCMC_NF pool entry points -- at every
dimension and batch size the entry points accept.

CPU: the checker's KDE (oracle_kde_*) against an independent float64 NumPy restatement of the estimator's formulae
(kernel_density.py:22-68, 96-128) for 1 .. 8 features, and against tests/golden/kde_hidim.npz, written by the reference
itself at 5 .. 8 features.  GPU: the gfx950 kernels against the checker, bit for bit, at every compiled shape, and the
user-facing AGLMCMC with a callback Model of 5 and 8 parameters.

Every output buffer of this file starts as a canary (a NaN with a payload no arithmetic produces, a fixed negative
integer): after GLABC_OK no element the entry point writes may still hold it, after an error every element must.  An
entry point that accepts a shape it has no kernel for fails here, whatever it leaves in the buffer.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from glabcmcmc_amd import _capi as A
from helpers import (CANARY_I32, assert_untouched, assert_written, bits, canary_f32, canary_i32, canary_i64, canary_left,
                     dev, host, kde_struct, load_golden, make_dist, rule)
from test_kde import LP_ATOL, RTOL

ERR_DIM, ERR_ARG = -2, -4            # glabc_status, include/glabc.h

CENTRES_CPU = (2, 63, 64, 65, 257, 3000)


# ---------------------------------------------------------------------------------- canaries (the helpers: helpers.py)
def canary_fit(oracle, X, w, h, bw_fixed):
    """helpers.oracle_fit with canary-filled outputs (np.empty there): the checker must write all of them too"""
    n, d = X.shape
    xs = np.ascontiguousarray(X.T)
    weights, log_w, wq, consts = canary_f32(n), canary_f32(n), canary_i64(n), canary_f32(d + 2)
    bwp = None if bw_fixed is None else np.ascontiguousarray(bw_fixed, np.float32)
    rc = oracle.oracle_kde_fit(xs.ctypes.data, None if w is None else w.ctypes.data, n, d, float(h),
                               None if bwp is None else bwp.ctypes.data, weights.ctypes.data, log_w.ctypes.data, wq.ctypes.data,
                               consts.ctypes.data)
    assert rc == 0
    assert_written(weights, log_w, wq, consts)
    return xs, weights, log_w, wq, consts


def oracle_log_prob(oracle, k, pts):
    ps = np.ascontiguousarray(pts.T)
    out = canary_f32(len(pts))
    assert oracle.oracle_kde_log_prob(C.byref(k), ps.ctypes.data, len(pts), out.ctypes.data) == 0
    assert_written(out)
    return ps, out


# --------------------------------------------------------------------- the estimator, restated in float64 NumPy
def kde_reference(X, w, bandwidth, pts):
    """Weighted Gaussian KDE in float64 from the estimator's formulae; shares no code with oracle/.
    bandwidth: 'silverman' | 'scott' | scalar | (d,) array.  -> weights, bandwidth, sum log bw, 0.5 d log 2pi, log p(pts)"""
    X = np.asarray(X, np.float64)
    n, d = X.shape
    w = np.full(n, 1.0 / n) if w is None else np.asarray(w, np.float64) / np.asarray(w, np.float64).sum()
    if isinstance(bandwidth, str):
        h = (n * (d + 2) / 4.) ** (-1. / (d + 4)) if bandwidth == "silverman" else n ** (-1. / (d + 4))
        v = w / w.sum()
        mean = (v[:, None] * X).sum(0)
        var = (v[:, None] * (X - mean) ** 2).sum(0) / max(1.0 - (v ** 2).sum(), 1e-10)
        bw = h * np.sqrt(var)
    else:
        bw = np.ones(d) * np.asarray(bandwidth, np.float64)
    sum_log_bw, c_2pi = np.log(bw).sum() if (bw > 0).all() else -np.inf, 0.5 * d * math.log(2 * math.pi)
    lp = None
    if pts is not None:
        lp = np.empty(len(pts))
        log_w = np.log(w + 1e-10)
        for lo in range(0, len(pts), 64):                                  # blocks: (64, n, d) float64 at a time
            z = (np.asarray(pts[lo:lo + 64], np.float64)[:, None, :] - X[None]) / bw
            lk = -0.5 * (z ** 2).sum(-1) - c_2pi - sum_log_bw + log_w
            m = lk.max(1)
            lp[lo:lo + 64] = m + np.log(np.exp(lk - m[:, None]).sum(1))
    return w, bw, sum_log_bw, c_2pi, lp


def kde_inputs(rng, n, d, weighted=True, zero_frac=0.1):
    X = (rng.standard_normal((n, d)) * rng.uniform(0.3, 2.0, d) + rng.uniform(-1, 1, d)).astype(np.float32)
    w = None
    if weighted:
        w = np.exp(rng.standard_normal(n)).astype(np.float32)
        if n > 2:                                                          # two centres, one without weight, have no spread
            z = rng.random(n) < zero_frac
            z[:2] = False
            w[z] = 0.0
    return X, w


def kde_points(rng, X, m):
    """m points: at a centre, near the centres, in the bulk, in the far tail"""
    n, d = X.shape
    pts = (rng.standard_normal((m, d)) * 2.5).astype(np.float32)
    near = min(m // 3, n)
    pts[:near] = X[:near] + (0.1 * rng.standard_normal((near, d))).astype(np.float32)
    pts[0] = X[n // 2]
    if m > 1:
        pts[1] = 60.0
    if m > 2:
        pts[2] = (-40.0 * (1 + np.arange(d))).astype(np.float32)
    return pts


FIXED_BW = np.array([0.2, 0.5, 0.1, 1.5, 0.3, 0.8, 0.05, 1.0], np.float32)


@pytest.mark.parametrize("d", range(1, 9))
def test_checker_kde_matches_float64_restatement(oracle, d):
    """oracle_kde_fit / oracle_kde_log_prob against kde_reference: weighted, unweighted and fixed-bandwidth fits with 2 .. 3000
    centres (fewer than, exactly and more than a wavefront), one centre with a fixed bandwidth, NaN points.  The tolerances
    are tests/test_kde.py's."""
    rng = np.random.default_rng(100 + d)
    for n in CENTRES_CPU + (1,):
        for mode in (("weighted", "unweighted", "fixed") if n > 1 else ("fixed",)):
            X, w = kde_inputs(rng, n, d, weighted=mode != "unweighted")
            kind = ("silverman", "scott")[n % 2]
            bw_in = None if mode != "fixed" else (FIXED_BW[:d] if n % 2 else np.repeat(np.float32(0.3), d))
            pts = kde_points(rng, X, 40)
            xs, weights, log_w, wq, consts = canary_fit(oracle, X, w, 0.0 if bw_in is not None else rule(kind, n, d), bw_in)
            rw, rbw, rsl, rc2, rlp = kde_reference(X, w, kind if bw_in is None else bw_in, pts)
            np.testing.assert_allclose(weights, rw, rtol=RTOL, atol=1e-12)
            np.testing.assert_allclose(consts[:d], rbw, rtol=RTOL)
            # logarithms of quantities held to RTOL relative: RTOL absolute (d log x = dx / x)
            np.testing.assert_allclose(consts[d], rsl, rtol=RTOL, atol=RTOL)
            np.testing.assert_allclose(consts[d + 1], rc2, rtol=RTOL)
            np.testing.assert_allclose(log_w, np.log(rw + 1e-10), rtol=RTOL, atol=RTOL)
            assert abs(int(wq.sum()) / 2.0 ** 40 - 1) < 1e-6
            k = kde_struct(xs, log_w, None, consts, d, n)
            _, out = oracle_log_prob(oracle, k, pts)
            assert np.isfinite(out).all()
            np.testing.assert_allclose(out, rlp, rtol=RTOL, atol=LP_ATOL, err_msg="d=%d n=%d %s" % (d, n, mode))
            # NaN in any one coordinate -> NaN, and only there
            bad = pts[:d + 1].copy()
            for j in range(d):
                bad[j, j] = np.nan
            _, out = oracle_log_prob(oracle, k, bad)
            assert np.isnan(out[:d]).all() and np.isnan(kde_reference(X, w, kind if bw_in is None else bw_in, bad)[4][:d]).all()
            assert np.array_equal(bits(out[d:]), bits(oracle_log_prob(oracle, k, pts[d:d + 1])[1]))


@pytest.mark.parametrize("d", range(1, 9))
def test_one_centre_has_no_rule_bandwidth(oracle, d):
    """With one centre the weighted std is 0 by the estimator's own formula, so a rule-based bandwidth is 0: both the float64
    restatement and the checker say so (the device entry points refuse such a descriptor, see the GPU test below)."""
    X = np.arange(1, d + 1, dtype=np.float32).reshape(1, d)
    for w in (None, np.array([3.0], np.float32)):
        assert (kde_reference(X, w, "silverman", None)[1] == 0).all()
        xs, weights, log_w, wq, consts = canary_fit(oracle, X, w, rule("silverman", 1, d), None)
        assert (consts[:d] == 0).all() and weights[0] == 1.0 and wq[0] == 1 << 40


@pytest.mark.parametrize("d", range(5, 9))
def test_checker_kde_sample_follows_the_inverse_cdf(oracle, d):
    """oracle_kde_sample at 5 .. 8 features: row r takes centre j = first index whose integer prefix sum exceeds
    floor(u_r * total) -- recomputed here in exact integers from the u of oracle_kde_draws -- and adds float32(normal * bandwidth)
    of the same row's normals: out == X[j] + float32(nrm * bw) in IEEE float32, bit for bit."""
    rng = np.random.default_rng(200 + d)
    n, m, seed, row0 = 257, 4000, 91, (1 << 33) + 12345
    X, w = kde_inputs(rng, n, d)
    xs, weights, log_w, wq, consts = canary_fit(oracle, X, w, rule("scott", n, d), None)
    cum = np.cumsum(wq)
    k = kde_struct(xs, log_w, cum, consts, d, n)
    out = canary_f32(d, m)
    assert oracle.oracle_kde_sample(C.byref(k), m, seed, row0, out.ctypes.data) == 0
    assert_written(out)
    u, nrm = np.full(m, -1.0), canary_f32(m, d)
    oracle.oracle_kde_draws(seed, row0, m, d, u.ctypes.data, nrm.ctypes.data)
    assert_written(nrm)
    assert (u >= 0).all() and (u < 1).all()
    target = np.array([int(v * float(int(cum[-1]))) for v in u], np.int64)
    idx = np.minimum(np.searchsorted(cum, target, side="right"), n - 1)
    assert (weights[idx] > 0).all()                                        # a centre without weight is never drawn
    assert len(np.unique(idx)) > n // 2
    step = (nrm * consts[:d][None, :]).astype(np.float32)                  # float32 * float32, rounded once
    want = (X[idx] + step).astype(np.float32)
    assert np.array_equal(bits(out.T), bits(want))


def _hidim_cases(g):
    return eval(str(g["cases"]), {"__builtins__": {}}, {})


def _hidim_inputs(g, tag, d, n, weighted, bw):
    X = g[tag + "_X"]
    w = g[tag + "_w"] if weighted else None
    if bw == "fixed":
        b = g[tag + "_bw_in"]
        return X, w, 0.0, (np.repeat(b, d) if b.size == 1 else b).astype(np.float32)
    return X, w, rule(bw, n, d), None


def test_checker_kde_matches_reference_at_5_to_8_features(oracle):
    """tests/golden/kde_hidim.npz (make_golden.kde_hidim_fixture: the reference's own KernelDensity on the CPU)"""
    g = load_golden("kde_hidim")
    cases = _hidim_cases(g)
    assert sorted(c[1] for c in cases) == [5, 6, 7, 8] and {c[4] for c in cases} == {"silverman", "scott", "fixed"}
    for tag, d, n, weighted, bw in cases:
        X, w, h, bw_fixed = _hidim_inputs(g, tag, d, n, weighted, bw)
        xs, weights, log_w, wq, consts = canary_fit(oracle, X, w, h, bw_fixed)
        np.testing.assert_allclose(weights, g[tag + "_weights"], rtol=RTOL, atol=1e-12)
        np.testing.assert_allclose(consts[:d], g[tag + "_bandwidth"], rtol=RTOL)
        assert abs(int(wq.sum()) / 2.0 ** 40 - 1) < 1e-6
        k = kde_struct(xs, log_w, None, consts, d, n)
        _, out = oracle_log_prob(oracle, k, g[tag + "_pts"])
        np.testing.assert_allclose(out, g[tag + "_log_prob"], rtol=RTOL, atol=LP_ATOL)
        assert np.isfinite(out).all()
        # and the float64 restatement reads the same numbers out of the reference's inputs
        rlp = kde_reference(X, w, bw if bw_fixed is None else bw_fixed, g[tag + "_pts"])[4]
        np.testing.assert_allclose(g[tag + "_log_prob"], rlp, rtol=RTOL, atol=LP_ATOL)


# ================================================================================================================ GPU
def device_kde(k, xg, log_w_g, cum_g):
    kg = A.Kde()
    C.memmove(C.byref(kg), C.byref(k), C.sizeof(k))
    kg.x, kg.log_w = xg.data_ptr(), log_w_g.data_ptr()
    kg.cum_q = None if cum_g is None else cum_g.data_ptr()
    return kg


def hip_fit(hip, xg, wg, n, d, h, bw_fixed):
    outs = dev(canary_f32(n)), dev(canary_f32(n)), dev(canary_i64(n)), dev(canary_f32(d + 2))
    bwp = None if bw_fixed is None else (C.c_float * d)(*[float(v) for v in bw_fixed])
    rc = hip.glabc_kde_fit(xg.data_ptr(), None if wg is None else wg.data_ptr(), n, d, float(h), bwp, outs[0].data_ptr(),
                           outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), None)
    return (rc,) + tuple(host(t) for t in outs)


def _gpu_centres(d):
    return (1, 63, 64, 65, 257, 8192 if d in (4, 8) else 5000)


@pytest.mark.gpu
@pytest.mark.parametrize("d,n", [(d, n) for d in range(1, 9) for n in _gpu_centres(d)])
def test_hip_kde_equals_checker_at_every_dimension(hip, oracle, d, n):
    """glabc_kde_fit / _log_prob / _log_prob_indexed / _sample against the checker, bit for bit, for 1 .. 8 features: one
    centre, fewer than / exactly / more than a wavefront of centres (lanes without a term in both passes), AGLMCMC's size;
    ~10 % centres without weight; rule-based and fixed bandwidth; point counts around the four points of a workgroup."""
    for fixed in ((True,) if n == 1 else (False, True)):
        rng = np.random.default_rng(1000 * d + n + int(fixed))
        X, w = kde_inputs(rng, n, d)
        bw_fixed = FIXED_BW[:d] if fixed else None
        h = 0.0 if fixed else rule(("silverman", "scott")[n % 2], n, d)
        xs, weights, log_w, wq, consts = canary_fit(oracle, X, w, h, bw_fixed)
        xg, wg = dev(xs), dev(w)
        rc, weights_g, log_w_g, wq_g, consts_g = hip_fit(hip, xg, wg, n, d, h, bw_fixed)
        assert rc == 0
        assert_written(weights_g, log_w_g, wq_g, consts_g)
        assert np.array_equal(bits(weights_g), bits(weights))
        assert np.array_equal(bits(log_w_g), bits(log_w))
        assert np.array_equal(wq_g, wq)
        assert np.array_equal(bits(consts_g), bits(consts))                # bandwidth[0..d), sum log bw, 0.5 d log 2pi
        cum = np.cumsum(wq)
        k = kde_struct(xs, log_w, cum, consts, d, n)
        lg, cg = dev(log_w_g), dev(cum)
        kg = device_kde(k, xg, lg, cg)
        # ---- log_prob: 1, 3, 4, 5 and 1501 points (1501 against thousands of centres only once: the checker is scalar code)
        big = kde_points(rng, X, 1501)
        big[3, d - 1] = np.nan                                             # NaN in the LAST coordinate
        big[1500, d - 1] = np.nan
        big[1499] = X[n - 1]                                               # the last point of the last workgroup sits on a centre
        for m in (1, 3, 4, 5) + ((1501,) if not fixed or n <= 257 else ()):
            sets = [big[:m]] if m > 1 else [big[0:1], big[1:2], big[3:4]]   # at a centre / far tail / NaN, one point each
            for pts in sets:
                ps, ref = oracle_log_prob(oracle, k, pts)
                og = dev(canary_f32(len(pts)))
                assert hip.glabc_kde_log_prob(C.byref(kg), dev(ps).data_ptr(), len(pts), og.data_ptr(), None) == 0
                got = host(og)
                assert_written(got)
                assert np.array_equal(bits(got), bits(ref)), (d, n, fixed, m)
            if m >= 4:
                assert np.isnan(ref[3]) and np.isfinite(ref[:3]).all()
        # ---- indexed: a shuffled subset, the count on the device; the rest of `out` keeps the canary; count 0 writes nothing
        pts = big[:301]
        ps, ref = oracle_log_prob(oracle, k, pts)
        pg = dev(ps)
        sel = rng.permutation(len(pts))[:131].astype(np.int32)
        idx_g = dev(np.concatenate([sel, np.zeros(len(pts) - len(sel), np.int32)]))
        for count in (len(sel), 0):
            og = dev(canary_f32(len(pts)))
            cnt = dev(np.array([count], np.int32))
            assert hip.glabc_kde_log_prob_indexed(C.byref(kg), pg.data_ptr(), len(pts), idx_g.data_ptr(), cnt.data_ptr(), len(pts),
                                                  og.data_ptr(), None) == 0
            got = host(og)
            hit = sel[:count]
            assert np.array_equal(bits(got[hit]), bits(ref[hit]))
            assert_untouched(got[np.setdiff1d(np.arange(len(pts)), hit)])
        # ---- sample: row offsets beyond 2^32, draw counts around the 256 rows of a workgroup
        seed, row0 = 77 + d, (1 << 34) + 3
        ref_s = canary_f32(d, 5000)
        assert oracle.oracle_kde_sample(C.byref(k), 5000, seed, row0, ref_s.ctypes.data) == 0
        assert_written(ref_s)
        for m in (1, 255, 256, 257, 5000):
            sg = dev(canary_f32(d, m))
            assert hip.glabc_kde_sample(C.byref(kg), m, seed, row0, sg.data_ptr(), None) == 0
            got = host(sg)
            assert_written(got)
            assert np.array_equal(bits(got), bits(ref_s[:, :m])), (d, n, fixed, m)
        sg = dev(canary_f32(d, 257))                                       # a second call continues the stream of the first
        assert hip.glabc_kde_sample(C.byref(kg), 257, seed, row0 + 1000, sg.data_ptr(), None) == 0
        assert np.array_equal(bits(host(sg)), bits(ref_s[:, 1000:1257]))


@pytest.mark.gpu
@pytest.mark.parametrize("d", range(1, 9))
def test_hip_kde_refusals_leave_the_outputs_alone(hip, oracle, d):
    """What the KDE entry points refuse, they refuse before any launch: a rule-based fit of ONE centre has bandwidth 0 (fit
    succeeds and says so), and log_prob / log_prob_indexed / sample with that descriptor return GLABC_ERR_ARG; 0 and 9
    features return GLABC_ERR_DIM.  Every output still holds its canary."""
    X = np.arange(1, d + 1, dtype=np.float32).reshape(1, d)
    xs, weights, log_w, wq, consts = canary_fit(oracle, X, None, rule("silverman", 1, d), None)
    xg = dev(xs)
    rc, weights_g, log_w_g, wq_g, consts_g = hip_fit(hip, xg, None, 1, d, rule("silverman", 1, d), None)
    assert rc == 0
    assert_written(weights_g, log_w_g, wq_g, consts_g)
    assert np.array_equal(bits(consts_g), bits(consts)) and (consts_g[:d] == 0).all()
    k = kde_struct(xs, log_w, np.cumsum(wq), consts, d, 1)
    lg, cg = dev(log_w), dev(np.cumsum(wq))
    kg = device_kde(k, xg, lg, cg)
    pg, idx, cnt = dev(np.zeros((d, 4), np.float32)), dev(np.arange(4, dtype=np.int32)), dev(np.array([4], np.int32))

    def refused(kd, want):
        og, sg = dev(canary_f32(4)), dev(canary_f32(d, 4))
        assert hip.glabc_kde_log_prob(C.byref(kd), pg.data_ptr(), 4, og.data_ptr(), None) == want
        assert hip.glabc_kde_log_prob_indexed(C.byref(kd), pg.data_ptr(), 4, idx.data_ptr(), cnt.data_ptr(), 4, og.data_ptr(),
                                              None) == want
        assert hip.glabc_kde_sample(C.byref(kd), 4, 1, 0, sg.data_ptr(), None) == want
        assert_untouched(host(og), host(sg))

    refused(kg, ERR_ARG)
    # a usable descriptor whose dim field is out of range
    xs2, weights, log_w, wq, consts = canary_fit(oracle, X, None, 0.0, FIXED_BW[:d])
    k2 = device_kde(kde_struct(xs2, log_w, None, consts, d, 1), xg, lg, cg)
    for bad in (0, 9):
        k2.dim = bad
        refused(k2, ERR_DIM)
        outs = dev(canary_f32(1)), dev(canary_f32(1)), dev(canary_i64(1)), dev(canary_f32(11))
        assert hip.glabc_kde_fit(xg.data_ptr(), None, 1, bad, 0.5, None, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                 outs[3].data_ptr(), None) == ERR_DIM
        assert_untouched(*[host(t) for t in outs])


@pytest.mark.gpu
def test_kernel_density_class_matches_reference_at_5_to_8_features(hip):
    """The drop-in class against the reference's numbers (tests/golden/kde_hidim.npz), as test_kde.py does up to 4 features."""
    from glabcmcmc_amd import KernelDensity
    g = load_golden("kde_hidim")
    for tag, d, n, weighted, bw in _hidim_cases(g):
        b = g[tag + "_bw_in"] if bw == "fixed" else None
        bw_arg = bw if b is None else (float(b[0]) if b.size == 1 else torch.from_numpy(b))
        k = KernelDensity(bandwidth=bw_arg, device="cuda", seed=5)
        k.fit(torch.from_numpy(g[tag + "_X"]), torch.from_numpy(g[tag + "_w"]) if weighted else None)
        assert k.bandwidth.shape == (d,)
        np.testing.assert_allclose(k.bandwidth.cpu().numpy(), g[tag + "_bandwidth"], rtol=RTOL)
        np.testing.assert_allclose(k.weights.cpu().numpy(), g[tag + "_weights"], rtol=RTOL, atol=1e-12)
        lp = k.log_prob(torch.from_numpy(g[tag + "_pts"]))
        np.testing.assert_allclose(lp.cpu().numpy(), g[tag + "_log_prob"], rtol=RTOL, atol=LP_ATOL)
        z, lq = k.forward(2000)
        assert z.shape == (2000, d) and lq.shape == (2000,) and torch.isfinite(z).all() and torch.isfinite(lq).all()
        assert np.array_equal(bits(k.log_prob(z).cpu().numpy()), bits(lq.cpu().numpy()))
        assert not torch.equal(z, k.sample(2000))                          # the stream advances between calls


@pytest.mark.gpu
@pytest.mark.parametrize("d", range(1, 9))
def test_hip_dist_forward_equals_checker_at_every_dimension(hip, oracle, d):
    """glabc_dist_forward -- AGLMCMC's initial pool, for a callback Model of any dimension too (generic.run_aglmcmc) -- against
    oracle_dist_forward_philox for 1 .. 8 dimensions, DiagGaussian and Uniform, row counts around the 256 rows of a workgroup;
    dimension 0 / 9 is refused."""
    specs = (("gauss", [0.5 - 0.3 * j for j in range(d)], [0.3 + 0.4 * j for j in range(d)]),
             ("uniform", [-2.0 - j for j in range(d)], [2.0 + 0.5 * j for j in range(d)]))
    for spec in specs:
        dist = make_dist(spec).descriptor()
        assert dist.dim == d
        for n in (1, 255, 256, 257, 3001):
            z, lp = canary_f32(d, n), canary_f32(n)
            assert oracle.oracle_dist_forward_philox(C.byref(dist), n, 9 + d, (1 << 33) + 5, z.ctypes.data, lp.ctypes.data) == 0
            assert_written(z, lp)
            zg, lg = dev(canary_f32(d, n)), dev(canary_f32(n))
            assert hip.glabc_dist_forward(C.byref(dist), n, 9 + d, (1 << 33) + 5, zg.data_ptr(), lg.data_ptr(), None) == 0
            assert_written(host(zg), host(lg))
            assert np.array_equal(bits(host(zg)), bits(z)) and np.array_equal(bits(host(lg)), bits(lp)), (spec[0], d, n)
        for bad in (0, 9):
            dist.dim = bad
            zg, lg = dev(canary_f32(8, 4)), dev(canary_f32(4))
            assert hip.glabc_dist_forward(C.byref(dist), 4, 1, 0, zg.data_ptr(), lg.data_ptr(), None) == ERR_DIM
            assert_untouched(host(zg), host(lg))
        dist.dim = d


# ------------------------------------------------------------------------------------- the GLMCMC_NF pool entry points
def abs_gauss_model(d, eps=0.3):
    """|theta| + noise in d dimensions, as tests/test_hip_parity.py::test_other_dimensions builds it"""
    from glabcmcmc_amd import distribution
    prior = distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d)).descriptor()
    noise = distribution.DiagGaussian(d, torch.zeros(d), torch.log(torch.full((d,), 0.05).sqrt())).descriptor()
    kern = distribution.DiagGaussian(1, torch.tensor([0.0]), torch.log(torch.tensor([eps]))).descriptor()
    model = A.Model()
    model.sim_kind, model.theta_dim, model.y_dim = A.SIM_ABS_GAUSS, d, d
    model.prior, model.noise = prior, noise
    for j in range(d):
        model.y_obs[j] = 1.5 - 0.25 * j
    model.kern_log_scale, model.kern_scale, model.kern_c0, model.epsilon = kern.p1[0], kern.p2[0], kern.c0, eps
    return model, make_dist(("gauss", [0.0] * d, [0.35] * d)).descriptor()


BATCHES = (1, 2, 3, 4, 7, 8, 15, 16)
CHAIN_COUNTS = (1, 63, 65, 300)


def pool_shape(d, N):
    """every D with every N once; within one D each step_size and each chain count at least once (8 batch sizes per D)"""
    j = BATCHES.index(N)
    return (1, 3)[(j + d) % 2], CHAIN_COUNTS[(j + d) % 4]


class PoolCase:
    """Inputs of one (D, N) shape and what the checker makes of them -- host side only, so that the no-idle-run condition
    (some chain moved) can be looked at without a GPU."""

    def __init__(self, oracle, d, N, n_iter=8, shape=None):
        import oracle_lib
        self.d, self.N = d, N
        self.step_size, self.n_chains = shape or pool_shape(d, N)
        self.model, self.local = abs_gauss_model(d)
        self.seed, self.gf, self.chain0 = 5 + d, 0.7, 7 + (1 << 33)
        self.n_iter = n_iter if self.n_chains > 1 else 24                 # one chain: enough iterations for it to move
        rng = np.random.default_rng(17 * d + N)
        C_ = self.n_chains
        self.rows = rows = N * self.step_size * C_
        self.theta = (rng.standard_normal((d, rows)) * 1.5).astype(np.float32)
        self.log_q = (rng.standard_normal(rows) - 3).astype(np.float32)
        self.pw_seed, self.pw_row0 = 11 + N, (1 << 35) + d
        self.x, self.w = canary_f32(d, rows), canary_f32(rows)
        assert oracle.oracle_pool_weights(C.byref(self.model), self.theta.ctypes.data, self.log_q.ctypes.data, rows, self.pw_seed,
                                          self.pw_row0, self.x.ctypes.data, self.w.ctypes.data) == 0
        assert_written(self.x, self.w)
        assert (self.w > 0).any()
        # the pool the iterations run against: ~10 % rows without weight, one row that dominates its slice
        self.w_pool = self.w.copy()
        self.w_pool[rng.random(rows) < 0.1] = 0.0
        self.w_pool[rng.integers(0, min(rows, N * C_))] = 1e6
        # training weights from stored discrepancies under three thresholds
        self.dis = np.abs(rng.standard_normal(rows) * 1.5).astype(np.float32)
        self.thresholds, self.tw = [], []
        for eps in (0.05, 0.7311, 2.5):
            ls = np.log(np.float32(eps))
            self.thresholds.append((float(ls), float(np.exp(ls))))
            m = self.with_threshold(self.thresholds[-1])
            tw = canary_f32(rows)
            assert oracle.oracle_kde_train_weights(C.byref(m), self.theta.ctypes.data, self.dis.ctypes.data, self.log_q.ctypes.data,
                                                   rows, tw.ctypes.data) == 0
            assert_written(tw)
            self.tw.append(tw)
        assert (self.tw[2] > 0).any()
        # iterations
        self.theta0 = rng.standard_normal((C_, d)).astype(np.float32)
        self.y0 = np.abs(self.theta0).astype(np.float32)
        hc = oracle_lib.HostChains(self.theta0, self.y0, chain0=self.chain0, with_isir=False)
        kk = np.zeros(C_, np.int32)
        self.lqo, self.steps = [], []
        for it in range(1, self.n_iter + 1):
            lqo = (rng.standard_normal(C_) - 2).astype(np.float32)
            hrow = canary_f32(d, C_)
            moved, n_moved, reset = canary_i32(C_), np.zeros(1, np.int32), canary_i32(1)
            pool = A.Pool(self.theta.ctypes.data, self.x.ctypes.data, self.w_pool.ctypes.data, lqo.ctypes.data, kk.ctypes.data,
                          self.step_size, 0, moved.ctypes.data, n_moved.ctypes.data, reset.ctypes.data)
            run, keep = oracle_lib.make_run(seed=self.seed, step0=it, n_steps=1, gf=self.gf, batch=N, history=hrow)
            cs = hc.struct()
            assert oracle.oracle_glmcmc_nf_step(C.byref(self.model), C.byref(self.local), C.byref(pool), C.byref(cs), C.byref(run)) == 0
            assert_written(hrow)
            assert reset[0] == 0 and canary_left(moved) == C_ - int(n_moved[0])
            self.lqo.append(lqo)
            self.steps.append(dict(row=hrow, kk=kk.copy(), theta=hc.theta.copy(), y=hc.y.copy(), n_moves=hc.n_moves.copy(),
                                   moved=np.sort(moved[:int(n_moved[0])]), n_moved=int(n_moved[0])))
        self.n_moves = hc.n_moves.copy()
        self.kk_max = int(kk.max())

    def with_threshold(self, t):
        m = A.Model()
        C.memmove(C.byref(m), C.byref(self.model), C.sizeof(m))
        m.kern_log_scale, m.kern_scale = t
        return m


@pytest.mark.parametrize("d", (1, 2, 3, 4))
def test_checker_pool_runs_are_not_idle(oracle, d):
    """The host half of the GPU comparison below: in every shape some chain moved, pool moves and the exhausted-pool guard were
    both reached, and across one D every step_size and every chain count occurs."""
    shapes = [pool_shape(d, N) for N in BATCHES]
    assert {s for s, _ in shapes} == {1, 3} and {c for _, c in shapes} == set(CHAIN_COUNTS)
    for N in BATCHES:
        case = PoolCase(oracle, d, N)
        assert case.n_moves.sum() > 0, (d, N)
        assert sum(s["n_moved"] for s in case.steps) == case.n_moves.sum()
        if case.n_chains > 1:
            assert case.kk_max > case.step_size, (d, N)                    # more global steps than slices: the guard ran


@pytest.mark.gpu
@pytest.mark.parametrize("d,N", [(d, N) for d in (1, 2, 3, 4) for N in BATCHES])
def test_pool_entry_points_equal_checker_at_every_compiled_shape(hip, oracle, d, N):
    """glabc_pool_weights, glabc_kde_train_weights and glabc_glmcmc_nf_step for every compiled <D, N> against the checker, bit
    for bit: states, history row, kk (exhausted-pool guard included), n_moves and the moved-chain list (a set: the kernel's
    order is unspecified) with its count and reset counter."""
    check_pool_case(hip, PoolCase(oracle, d, N))


def check_pool_case(hip, case):
    from glabcmcmc_amd import engine
    d, N = case.d, case.N
    assert case.n_moves.sum() > 0                                          # two idle runs cannot pass
    rows, n = case.rows, case.n_chains
    tg, lg = dev(case.theta), dev(case.log_q)
    xg, wg = dev(canary_f32(d, rows)), dev(canary_f32(rows))
    assert hip.glabc_pool_weights(C.byref(case.model), tg.data_ptr(), lg.data_ptr(), rows, case.pw_seed, case.pw_row0, xg.data_ptr(),
                                  wg.data_ptr(), None) == 0
    assert_written(host(xg), host(wg))
    assert np.array_equal(bits(host(xg)), bits(case.x)) and np.array_equal(bits(host(wg)), bits(case.w))
    dg = dev(case.dis)
    for t, want in zip(case.thresholds, case.tw):
        m = case.with_threshold(t)
        og = dev(canary_f32(rows))
        assert hip.glabc_kde_train_weights(C.byref(m), tg.data_ptr(), dg.data_ptr(), lg.data_ptr(), rows, og.data_ptr(), None) == 0
        assert_written(host(og))
        assert np.array_equal(bits(host(og)), bits(want))
    wpg = dev(case.w_pool)
    gc = engine.ChainBatch(torch.from_numpy(case.theta0), torch.from_numpy(case.y0), torch.device("cuda", 0), chain0=case.chain0)
    kk_g = torch.zeros(n, dtype=torch.int32, device="cuda")
    n_moved_g = torch.zeros(2, dtype=torch.int32, device="cuda")
    for it, (lqo, want) in enumerate(zip(case.lqo, case.steps), start=1):
        lq2, hg, moved_g = dev(lqo), dev(canary_f32(d, n)), dev(canary_i32(n))
        # two counters that swap roles: this call counts into `cur` (0 by the previous call's reset, never a canary: the
        # kernel indexes moved_idx with it) and must zero `nxt`, which starts as a canary
        cur, nxt = n_moved_g[it & 1:], n_moved_g[(it + 1) & 1:]
        n_moved_g[(it + 1) & 1] = CANARY_I32
        assert host(n_moved_g).tolist()[it & 1] == 0
        pool_g = A.Pool(tg.data_ptr(), xg.data_ptr(), wpg.data_ptr(), lq2.data_ptr(), kk_g.data_ptr(), case.step_size, 0,
                        moved_g.data_ptr(), cur.data_ptr(), nxt.data_ptr())
        run_g = A.Run()
        run_g.seed, run_g.step0, run_g.n_steps, run_g.global_frequency, run_g.batch_size = case.seed, it, 1, case.gf, N
        run_g.history, run_g.hist_stride = hg.data_ptr(), n
        csg = gc.struct()
        assert hip.glabc_glmcmc_nf_step(C.byref(case.model), C.byref(case.local), C.byref(pool_g), C.byref(csg), C.byref(run_g),
                                        None) == 0
        row = host(hg)
        assert_written(row)
        assert np.array_equal(bits(row), bits(want["row"])), (d, N, it)
        assert np.array_equal(host(kk_g), want["kk"])
        assert np.array_equal(bits(host(gc.theta)), bits(want["theta"])) and np.array_equal(bits(host(gc.y)), bits(want["y"]))
        assert np.array_equal(host(gc.n_moves).astype(np.uint32), want["n_moves"])
        k = int(cur[0].item())
        listed = host(moved_g)
        assert k == want["n_moved"] and int(nxt[0].item()) == 0
        assert np.array_equal(np.sort(listed[:k]), want["moved"])
        assert_untouched(listed[k:])


# glabc_glmcmc_nf_step picks nf_step_kernel<D, N> out of N = 1 .. 16 at run time (launch_nf_step); the grid above reaches the
# batch sizes of BATCHES.  The others, each at one D (every D twice) and at the smallest shape that can still go wrong: one
# full wavefront plus one lane, three iterations, both step sizes
OTHER_BATCHES = tuple(N for N in range(1, 17) if N not in BATCHES)


def other_batch_case(oracle, N):
    return PoolCase(oracle, 1 + OTHER_BATCHES.index(N) % 4, N, n_iter=3, shape=((1, 3)[N % 2], 65))


def test_checker_pool_runs_at_the_other_batch_sizes_are_not_idle(oracle):
    assert OTHER_BATCHES == (5, 6, 9, 10, 11, 12, 13, 14)
    for N in OTHER_BATCHES:
        case = other_batch_case(oracle, N)
        assert (case.d, case.n_chains, case.n_iter) == (1 + OTHER_BATCHES.index(N) % 4, 65, 3)
        assert case.n_moves.sum() > 0 and sum(s["n_moved"] for s in case.steps) == case.n_moves.sum(), N


@pytest.mark.gpu
@pytest.mark.parametrize("N", OTHER_BATCHES)
def test_nf_step_equals_checker_at_the_other_batch_sizes(hip, oracle, N):
    """with the grid above, every N of 1 .. 16 runs against the checker, bit for bit, canaries on every output"""
    check_pool_case(hip, other_batch_case(oracle, N))


@pytest.mark.gpu
@pytest.mark.parametrize("d", (5, 6, 7, 8))
def test_pool_entry_points_refuse_what_is_not_compiled(hip, d):
    """theta_dim 5 .. 8 -> GLABC_ERR_DIM from the three pool entry points; batch size 0 / 17 -> GLABC_ERR_ARG from
    glabc_glmcmc_nf_step at a compiled dimension.  Every output keeps its canary."""
    from glabcmcmc_amd import engine
    rng = np.random.default_rng(d)

    def attempt(dim, N):
        model, local = abs_gauss_model(dim)
        n, step_size = 65, 2
        rows = n * step_size * max(N, 1)
        tg, lg, dg = (dev(rng.standard_normal(s).astype(np.float32)) for s in ((dim, rows), (rows,), (rows,)))
        xg, wg, og = dev(canary_f32(dim, rows)), dev(canary_f32(rows)), dev(canary_f32(rows))
        rcs = [hip.glabc_pool_weights(C.byref(model), tg.data_ptr(), lg.data_ptr(), rows, 1, 0, xg.data_ptr(), wg.data_ptr(), None),
               hip.glabc_kde_train_weights(C.byref(model), tg.data_ptr(), dg.data_ptr(), lg.data_ptr(), rows, og.data_ptr(), None)]
        theta0 = rng.standard_normal((n, dim)).astype(np.float32)
        gc = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(np.abs(theta0)), torch.device("cuda", 0), chain0=0)
        kk_g, hg, moved_g, cnt = dev(canary_i32(n)), dev(canary_f32(dim, n)), dev(canary_i32(n)), dev(canary_i32(2))
        pool_g = A.Pool(tg.data_ptr(), tg.data_ptr(), lg.data_ptr(), lg.data_ptr(), kk_g.data_ptr(), step_size, 0, moved_g.data_ptr(),
                        cnt.data_ptr(), cnt[1:].data_ptr())
        run_g = A.Run()
        run_g.seed, run_g.step0, run_g.n_steps, run_g.global_frequency, run_g.batch_size = 1, 1, 1, 0.7, N
        run_g.history, run_g.hist_stride = hg.data_ptr(), n
        csg = gc.struct()
        rcs.append(hip.glabc_glmcmc_nf_step(C.byref(model), C.byref(local), C.byref(pool_g), C.byref(csg), C.byref(run_g), None))
        step_outs = [host(t) for t in (kk_g, hg, moved_g, cnt)]
        assert np.array_equal(bits(host(gc.theta).T), bits(theta0))
        return rcs, [host(xg), host(wg), host(og)], step_outs

    rcs, weight_outs, step_outs = attempt(d, 5)
    assert rcs == [ERR_DIM] * 3
    assert_untouched(*weight_outs, *step_outs)
    for N in (0, 17):
        rcs, weight_outs, step_outs = attempt(d - 4, N)                    # 1 .. 4: compiled; the batch size is what is refused
        assert rcs[:2] == [0, 0] and rcs[2] == ERR_ARG
        assert_written(*weight_outs)
        assert_untouched(*step_outs)


# ----------------------------------------------------------------------------------------------- the user-facing path
class TorchGaussian:
    """an importance proposal without a descriptor: N(0, scale^2 I) in plain torch (forward / log_prob callbacks)"""

    def __init__(self, d, scale):
        self.d, self.scale = d, scale

    def log_prob(self, z):
        z = z.reshape(-1, self.d)
        return -0.5 * self.d * math.log(2 * math.pi) - self.d * math.log(self.scale) - 0.5 * ((z / self.scale) ** 2).sum(1)

    def forward(self, n):
        z = torch.randn(n, self.d) * self.scale
        return z, self.log_prob(z)


@pytest.mark.gpu
@pytest.mark.parametrize("proposal", ("descriptor", "callback"))
@pytest.mark.parametrize("d", (5, 8))
def test_aglmcmc_callback_model_of_5_and_8_parameters_runs_on_the_defined_density(hip, d, proposal):
    """AGLMCMC with a user's plain-torch Model of 5 / 8 parameters (generic.run_aglmcmc builds a KernelDensity of that
    dimension): the proposal density left in state_out is the one the estimator defines -- the class's log_prob at its own
    centres and at the chains' final states equals the float64 restatement fed the class's X and weights -- its bandwidth
    has d finite positive entries, and forward()'s log density is log_prob of its draws, bit for bit.  No posterior moments."""
    from glabcmcmc_amd import AGLMCMC, KernelDensity, distribution
    from glabcmcmc_amd.examples.UserModel import TorchMixture
    torch.manual_seed(d)
    user = TorchMixture(d, 0.5)
    lp = distribution.DiagGaussian(d, loc=torch.zeros(1, d), log_scale=torch.log(torch.full((d,), 0.2)))
    # the initial pool: drawn by glabc_dist_forward (a proposal with a descriptor), or by the proposal's own forward()
    ip = distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d)) if proposal == "descriptor" else TorchGaussian(d, 1.0)
    n, T = 96, 300
    th0 = torch.zeros(n, d) + 1.5
    st = {}
    out = AGLMCMC(user, T, th0, user.generate_samples(th0), lp, ip, None, 0.6, 10, 5, 0.9, 1.0, seed=40 + d, verbose=False,
                  state_out=st)
    assert out.shape == (T, n, d) and torch.isfinite(out).all()
    assert st["num_train"] >= 1 and "callback_device" in st
    k = st["kde"]
    assert isinstance(k, KernelDensity) and k.dim == d and k.X.shape[1] == d and k.n_samples >= 2
    bw = k.bandwidth.cpu().numpy()
    assert bw.shape == (d,) and np.isfinite(bw).all() and (bw > 0).all()
    X, w = k.X.cpu().numpy(), k.weights.cpu().numpy()
    rw, rbw, _, _, _ = kde_reference(X, w, "silverman", None)
    np.testing.assert_allclose(bw, rbw, rtol=RTOL)                         # the fit is the Silverman fit of its own centres
    final = st["chains"].theta.t().contiguous()
    for pts in (k.X[:500], final):
        got = k.log_prob(pts).cpu().numpy()
        assert np.isfinite(got).all()
        want = kde_reference(X, w, bw, pts.cpu().numpy())[4]
        np.testing.assert_allclose(got, want, rtol=RTOL, atol=LP_ATOL)
    z, lq = k.forward(1000)
    assert z.shape == (1000, d) and torch.isfinite(z).all()
    assert np.array_equal(bits(k.log_prob(z).cpu().numpy()), bits(lq.cpu().numpy()))
    with pytest.raises(ValueError):
        KernelDensity(device="cuda").fit(torch.zeros(10, 9))
