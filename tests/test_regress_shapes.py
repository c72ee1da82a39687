"""glabc_weighted_gram and glabc_regression_apply (csrc/glabc_regress.hip) at every shape at which their kernels take another path,
held bit for bit to the NumPy restatement of their specifications (tests/regress_ref.py).

gram_kernel<COLS> is instantiated per column count y_dim + theta_dim = 2 .. 16, gives a segment of 1024 rows to a workgroup and a
slice of the statistics to each of its wavefronts (1 wavefront up to 6 columns, 5 at 16), lane l owning column l of 64.  So the grid
has every column count, several (theta_dim, y_dim) splits of one count -- (4, 8), (8, 8), (1, 1), (8, 1), (1, 8) among them --, and
row counts 0, 1, on both sides of a wavefront (63, 64, 65), of a segment (1023, 1024, 1025) and several segments with a ragged end
(2 x 1024 + 1, 5 x 1024 + 63); a stride above n whose pad columns hold NaN (a read of one makes a statistic NaN); the distance and the
weight each present and NULL; both kinds.  Where a case has rows of weight 0 they hold NaN theta and y (a row at distance exactly
delta under Epanechnikov, a row beyond delta, a row whose distance is NaN, a row whose weight is 0): no NaN may reach the Gram.
The cases are a covering grid, not a full product: each split meets four row counts, rotating, and the options rotate with other
periods; the two largest shapes meet every row count.  The output and the workspace sit between guard bands of canaries and are
compared whole: the workspace must hold the restatement's partial sums, bit for bit.

Tolerances: none.  Every comparison is of float bits, a NaN matching a NaN.
"""
import functools
import math

import numpy as np
import pytest

import regress_ref as R
from helpers import CANARY_BITS, CANARY_BITS64, canary_f32, canary_f64, dev, host

pytestmark = pytest.mark.gpu

OK, ERR_NULL, ERR_DIM, ERR_KIND, ERR_ARG = 0, -1, -2, -3, -4          # glabc_status, include/glabc.h
GUARD = 64
ROWS = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2 * 1024 + 1, 5 * 1024 + 63)
SPLITS = tuple((c - c // 2, c // 2) for c in range(2, 17)) + ((4, 8), (8, 1), (1, 8), (8, 4), (2, 7), (7, 8), (1, 4))
DELTA = 1.0
# (distance present, weight present, kind): the full product, and the usual calls once more
OPTIONS = tuple((d, w, k) for d in (True, False) for w in (True, False) for k in (0, 1)) + ((True, True, 0), (True, True, 1), (True, False, 0),
                                                                                          (False, True, 1))


@functools.lru_cache(maxsize=None)
def gram_cases():
    """(theta_dim, y_dim, n, pad, has_dis, has_weight, kind)"""
    out = []
    for i, (td, yd) in enumerate(SPLITS):
        rows = ROWS if (td, yd) in ((8, 8), (4, 8)) else tuple(ROWS[(3 * i + 5 * k) % len(ROWS)] for k in range(4))
        for k, n in enumerate(rows):
            j = len(out)
            out.append((td, yd, n, (0, 3, 17)[(i + k) % 3]) + OPTIONS[5 * j % len(OPTIONS)])
    return tuple(out)


def test_grid_covers():
    cases = gram_cases()
    assert {c[0] + c[1] for c in cases} == set(range(2, 17))
    assert {(1, 1), (8, 8), (4, 8), (8, 1), (1, 8)} <= {(c[0], c[1]) for c in cases}
    assert {c[2] for c in cases} == set(ROWS)
    for n in ROWS:
        assert {(c[0], c[1]) for c in cases if c[2] == n} >= {(8, 8), (4, 8)}
    for has_dis in (False, True):
        for has_w in (False, True):
            for kind in (0, 1):
                assert sum(1 for c in cases if c[4:] == (has_dis, has_w, kind)) >= 2, (has_dis, has_w, kind)
    assert {c[3] for c in cases} == {0, 3, 17}


def rows_of(seed, td, yd, n):
    rng = np.random.default_rng(seed)
    theta = rng.standard_normal((td, n)).astype(np.float32)
    y = (0.5 * rng.standard_normal((yd, n)) + 0.25).astype(np.float32)
    dis = rng.uniform(0.0, 1.3, n).astype(np.float32)
    weight = rng.uniform(0.25, 2.0, n).astype(np.float32)
    y_obs = rng.uniform(-0.5, 0.5, yd)
    return theta, y, dis, weight, y_obs


def padded(a, pad, fill=np.nan):
    """[rows][n] -> [rows][max(n + pad, 1)] with `fill` in the pad columns"""
    out = np.full((a.shape[0], max(a.shape[1] + pad, 1)), fill, a.dtype)
    out[:, :a.shape[1]] = a
    return out


def guarded64(size):
    t = dev(canary_f64(GUARD + size + GUARD))
    return t, t.data_ptr() + 8 * GUARD


def body64(t, size):
    flat = host(t)
    assert (flat[:GUARD].view(np.uint64) == CANARY_BITS64).all() and (flat[GUARD + size:].view(np.uint64) == CANARY_BITS64).all(), "guard band"
    return flat[GUARD:GUARD + size]


def run_gram(hip, theta, y, dis, weight, n, pad, y_obs, delta, kind):
    """-> (status, gram [Q], workspace [S][Q]) of one call on padded device copies"""
    td, yd = theta.shape[0], y.shape[0]
    q, s = R.n_stats(td, yd), (n + 1023) // 1024
    th, ys = dev(padded(theta, pad)), dev(padded(y, pad))
    d = None if dis is None else dev(padded(dis[None, :], pad))
    w = None if weight is None else dev(padded(weight[None, :], pad))
    gram, gram_ptr = guarded64(q)
    work, work_ptr = guarded64(s * q)
    y_obs = np.ascontiguousarray(y_obs, np.float64)
    rc = hip.glabc_weighted_gram(th.data_ptr(), th.shape[1], td, ys.data_ptr(), ys.shape[1], yd, None if d is None else d.data_ptr(),
                                 None if w is None else w.data_ptr(), n, y_obs.ctypes.data, delta, kind, gram_ptr, work_ptr, None)
    return rc, body64(gram, q), body64(work, s * q).reshape(s, q)


@pytest.mark.parametrize("case", range(len(gram_cases())))
def test_weighted_gram_bits(hip, case):
    td, yd, n, pad, has_dis, has_w, kind = gram_cases()[case]
    theta, y, dis, weight, y_obs = rows_of(case, td, yd, n)
    if not has_dis:
        dis = None
    if not has_w:
        weight = None
    zero = []                                       # rows of weight 0: whatever they hold must not matter
    if n >= 64:
        if has_dis:
            dis[3] = DELTA                          # exactly delta: Epanechnikov gives 1 - 1 = 0 and skips, uniform keeps
            dis[5] = np.nan
            dis[n - 1] = 2.0
            zero += [5, n - 1] + ([3] if kind == R.EPANECHNIKOV else [])
        if has_w:
            weight[40] = 0.0
            zero.append(40)
    for r in zero:
        theta[:, r] = np.nan
        y[r % yd, r] = np.inf
    want, want_partial = R.weighted_gram(theta, y, dis, weight, n, y_obs, DELTA, kind)
    assert not np.isnan(want).any()
    rc, got, partial = run_gram(hip, theta, y, dis, weight, n, pad, y_obs, DELTA, kind)
    assert rc == OK
    assert R.same_bits(partial, want_partial), "partial sums"
    assert R.same_bits(got, want), np.nonzero(got != want)
    if n == 0:
        assert (got.view(np.uint64) == 0).all()      # Q zeros
    if has_dis and n >= 64 and not has_w:
        kept = R.row_weights(dis, None, n, DELTA, kind) != 0
        assert bool(kept[3]) == (kind == R.UNIFORM)


@pytest.mark.parametrize("kind", [R.EPANECHNIKOV, R.UNIFORM])
def test_infinite_delta_keeps_every_finite_distance(hip, kind):
    theta, y, dis, weight, y_obs = rows_of(100 + kind, 3, 5, 1500)
    dis[11] = np.nan
    theta[1, 11] = np.nan
    want, want_partial = R.weighted_gram(theta, y, dis, weight, 1500, y_obs, math.inf, kind)
    rc, got, partial = run_gram(hip, theta, y, dis, weight, 1500, 3, y_obs, math.inf, kind)
    assert rc == OK and R.same_bits(got, want) and R.same_bits(partial, want_partial)
    assert not np.isnan(got).any()
    plain, _ = R.weighted_gram(np.delete(theta, 11, 1), np.delete(y, 11, 1), None, np.delete(weight, 11), 1499, y_obs, 1.0, R.UNIFORM)
    assert np.allclose(got, plain, rtol=1e-12, atol=0)                 # every finite distance has k = 1


def test_nan_in_a_weighted_row_stays_in_its_statistics(hip):
    td, yd, n = 4, 8, 1300
    theta, y, dis, weight, y_obs = rows_of(7, td, yd, n)
    dis[:] = 0.5 * dis / 1.3
    theta[2, 1100] = np.nan                         # coordinate 1 + yd + 2 of z
    y[5, 64] = np.nan                               # coordinate 1 + 5
    want, want_partial = R.weighted_gram(theta, y, dis, weight, n, y_obs, DELTA, R.EPANECHNIKOV)
    rc, got, partial = run_gram(hip, theta, y, dis, weight, n, 0, y_obs, DELTA, R.EPANECHNIKOV)
    assert rc == OK and R.same_bits(got, want) and R.same_bits(partial, want_partial)
    bad = {1 + yd + 2, 1 + 5}
    involved = np.array([a in bad or b in bad for a, b in R.pairs(1 + yd + td)] + [False])
    assert np.array_equal(np.isnan(got), involved)


def test_nan_weight_propagates(hip):
    theta, y, dis, weight, y_obs = rows_of(8, 2, 2, 200)
    weight[130] = np.nan
    dis[130] = 0.1
    want, _ = R.weighted_gram(theta, y, dis, weight, 200, y_obs, DELTA, R.UNIFORM)
    rc, got, _ = run_gram(hip, theta, y, dis, weight, 200, 3, y_obs, DELTA, R.UNIFORM)
    assert rc == OK and R.same_bits(got, want) and np.isnan(got).all()


# ---- glabc_regression_apply
@pytest.mark.parametrize("td", range(1, 9))
@pytest.mark.parametrize("yd", range(1, 9))
def test_regression_apply_bits(hip, td, yd):
    n, pad = 130, 5
    theta, y, _, _, y_obs = rows_of(1000 + 8 * td + yd, td, yd, n)
    beta = np.ascontiguousarray(np.random.default_rng(td * 8 + yd).standard_normal((yd, td)))
    want = R.regression_apply(theta, y, n, y_obs, beta)
    ys = dev(padded(y, pad))
    # out of place: the pad columns of `out` keep the canary, theta is unchanged
    th = dev(padded(theta, pad))
    out = dev(canary_f32(GUARD + td * (n + pad) + GUARD))
    rc = hip.glabc_regression_apply(th.data_ptr(), n + pad, td, ys.data_ptr(), n + pad, yd, n, y_obs.ctypes.data, beta.ctypes.data,
                                    out.data_ptr() + 4 * GUARD, n + pad, None)
    assert rc == OK
    flat = host(out).view(np.uint32)
    assert (flat[:GUARD] == CANARY_BITS).all() and (flat[-GUARD:] == CANARY_BITS).all()
    body = flat[GUARD:-GUARD].reshape(td, n + pad)
    assert (body[:, n:] == CANARY_BITS).all(), "pad columns written"
    assert R.same_bits(body[:, :n].view(np.float32), want)
    assert R.same_bits(host(th), padded(theta, pad))
    # in place: the pad columns of theta keep what they held
    rc = hip.glabc_regression_apply(th.data_ptr(), n + pad, td, ys.data_ptr(), n + pad, yd, n, y_obs.ctypes.data, beta.ctypes.data,
                                    th.data_ptr(), n + pad, None)
    assert rc == OK
    got = host(th)
    assert R.same_bits(got[:, :n], want) and np.isnan(got[:, n:]).all()


# ---- refusals: in the documented order, and nothing is written
def test_refusals(hip):
    td, yd, n = 3, 2, 100
    theta, y, dis, weight, y_obs = rows_of(9, td, yd, n)
    th, ys, d = dev(theta), dev(y), dev(dis)
    gram, gram_ptr = guarded64(R.n_stats(td, yd))
    work, work_ptr = guarded64(R.n_stats(td, yd))
    out = dev(canary_f32(td * n))
    beta = np.zeros((yd, td))
    nan = math.nan

    def gram_call(theta=th.data_ptr(), stride_t=n, td=td, y=ys.data_ptr(), stride_y=n, yd=yd, n=n, y_obs=y_obs.ctypes.data, delta=1.0,
                  kind=0, gram=gram_ptr, work=work_ptr):
        return hip.glabc_weighted_gram(theta, stride_t, td, y, stride_y, yd, d.data_ptr(), None, n, y_obs, delta, kind, gram, work, None)

    def apply_call(theta=th.data_ptr(), stride_t=n, td=td, y=ys.data_ptr(), stride_y=n, yd=yd, n=n, y_obs=y_obs.ctypes.data,
                   beta=beta.ctypes.data, out=out.data_ptr(), stride_o=n):
        return hip.glabc_regression_apply(theta, stride_t, td, y, stride_y, yd, n, y_obs, beta, out, stride_o, None)

    # a NULL pointer before a dimension before a kind before a number
    for null in ("theta", "y", "y_obs", "gram", "work"):
        assert gram_call(**{null: None, "td": 9, "kind": 7, "stride_t": n - 1}) == ERR_NULL, null
    assert gram_call(work=None, n=-1) == ERR_ARG                    # a NULL workspace is refused only where there are rows
    assert gram_call(td=0, kind=7, n=-1) == ERR_DIM and gram_call(td=9) == ERR_DIM
    assert gram_call(yd=0, delta=nan) == ERR_DIM and gram_call(yd=9) == ERR_DIM
    assert gram_call(kind=2, n=-1) == ERR_KIND and gram_call(kind=-1, delta=0.0) == ERR_KIND
    for bad in (dict(n=-1), dict(stride_t=n - 1), dict(stride_y=n - 1), dict(delta=nan), dict(delta=0.0), dict(delta=-1.0)):
        assert gram_call(**bad) == ERR_ARG, bad
    for null in ("theta", "y", "y_obs", "beta", "out"):
        assert apply_call(**{null: None, "td": 9, "n": -1}) == ERR_NULL, null
    assert apply_call(td=0, n=-1) == ERR_DIM and apply_call(td=9) == ERR_DIM and apply_call(yd=0) == ERR_DIM and apply_call(yd=9) == ERR_DIM
    for bad in (dict(n=-1), dict(stride_t=n - 1), dict(stride_y=n - 1), dict(stride_o=n - 1)):
        assert apply_call(**bad) == ERR_ARG, bad
    assert apply_call(n=0) == OK
    # nothing was written by any refused call
    assert (body64(gram, R.n_stats(td, yd)).view(np.uint64) == CANARY_BITS64).all()
    assert (body64(work, R.n_stats(td, yd)).view(np.uint64) == CANARY_BITS64).all()
    assert (host(out).view(np.uint32) == CANARY_BITS).all()
    assert gram_call(work=None, n=0) == OK                          # no workspace is needed for no rows: Q zeros
    assert (body64(gram, R.n_stats(td, yd)).view(np.uint64) == 0).all()
