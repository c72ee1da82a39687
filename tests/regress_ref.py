"""NumPy restatement of the two specifications of ABC regression adjustment in include/glabc.h: glabc_weighted_gram and
glabc_regression_apply.  IEEE double, one ufunc call per rounded operation (NumPy's element-wise ufuncs do not fuse), in the order
the header states: the column loop is 16 vectorised steps, the butterfly is ``c + c[:, idx ^ h]`` and the segment loop runs ascending.

Arrays are dimension-major as the entry points read them: theta [theta_dim][>= n], y [y_dim][>= n]; only columns < n are read.
"""
import numpy as np

EPANECHNIKOV, UNIFORM = 0, 1
SEGMENT, LANES, STEPS = 1024, 64, 16


def n_stats(theta_dim, y_dim):
    p = 1 + y_dim + theta_dim
    return p * (p + 1) // 2 + 1


def pairs(p):
    """(a, b), a <= b, in packed order"""
    return [(a, b) for a in range(p) for b in range(a, p)]


def row_weights(dis, weight, n, delta, kind):
    """w_r [n] float64"""
    if dis is None:
        k = np.ones(n)
    else:
        d = np.asarray(dis[:n], np.float32).astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            u = d / np.float64(delta)
            inside = d <= np.float64(delta)
            k = np.where(inside, 1.0 - u * u if kind == EPANECHNIKOV else 1.0, 0.0)
    if weight is None:
        return k
    with np.errstate(invalid="ignore"):
        return k * np.asarray(weight[:n], np.float32).astype(np.float64)


def design(theta, y, n, y_obs):
    """z [n][P] float64"""
    y_obs = np.asarray(y_obs, np.float64)
    with np.errstate(invalid="ignore"):
        zy = np.asarray(y, np.float32)[:, :n].astype(np.float64) - y_obs[:, None]
    zt = np.asarray(theta, np.float32)[:, :n].astype(np.float64)
    return np.concatenate([np.ones((1, n)), zy, zt]).T


def row_terms(z, w):
    """term_r of every statistic [Q][n]: (w z_a) z_b in packed order, then w w"""
    with np.errstate(invalid="ignore", over="ignore"):
        wz = w[:, None] * z
        out = [wz[:, a] * z[:, b] for a, b in pairs(z.shape[1])]
        out.append(w * w)
    return np.stack(out)


def ordered_sum(terms, w):
    """[Q][n] terms, [n] weights -> (G [Q], partial [S][Q]) in the specified order; a row with w == 0 is skipped"""
    q, n = terms.shape
    s = (n + SEGMENT - 1) // SEGMENT
    t = np.zeros((q, s * SEGMENT))
    t[:, :n] = terms
    keep = np.zeros(s * SEGMENT, bool)
    keep[:n] = w != 0.0                                             # a NaN weight is kept
    t = t.reshape(q, s, STEPS, LANES)
    keep = keep.reshape(s, STEPS, LANES)
    c = np.zeros((q, s, LANES))
    with np.errstate(invalid="ignore", over="ignore"):
        for step in range(STEPS):
            c = np.where(keep[None, :, step, :], c + t[:, :, step, :], c)
        idx = np.arange(LANES)
        h = 1
        while h < LANES:
            c = c + c[:, :, idx ^ h]
            h *= 2
        partial = c[:, :, 0].T.copy()                               # [S][Q]
        g = np.zeros(q)
        for seg in range(s):
            g = g + partial[seg]
    return g, partial


def weighted_gram(theta, y, dis, weight, n, y_obs, delta, kind):
    """-> (gram [Q], partial [S][Q]) float64, the bits glabc_weighted_gram writes to `gram` and to its workspace"""
    w = row_weights(dis, weight, n, delta, kind)
    z = design(theta, y, n, y_obs)
    return ordered_sum(row_terms(z, w), w)


def regression_apply(theta, y, n, y_obs, beta):
    """-> out [theta_dim][n] float32"""
    theta, y = np.asarray(theta, np.float32), np.asarray(y, np.float32)
    beta, y_obs = np.asarray(beta, np.float64), np.asarray(y_obs, np.float64)
    yd, td = beta.shape
    with np.errstate(invalid="ignore", over="ignore"):
        dy = y[:, :n].astype(np.float64) - y_obs[:, None]
        out = np.empty((td, n), np.float32)
        for j in range(td):
            a = theta[j, :n].astype(np.float64)
            for k in range(yd):
                a = a - beta[k, j] * dy[k]
            out[j] = a.astype(np.float32)
    return out


def same_bits(a, b):
    """equal float bits, a NaN matching any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return bool((nan_a == nan_b).all() and (np.ascontiguousarray(a).view(u)[~nan_a] == np.ascontiguousarray(b).view(u)[~nan_a]).all())


def addition_bound(terms, w):
    """per statistic, (number of additions) 2^-53 sum |term| over the weighted rows: the bound of a float64 sum in any order"""
    keep = w != 0.0
    t = np.abs(terms[:, keep])
    return max(int(keep.sum()) - 1, 1) * 2.0 ** -53 * t.sum(axis=1)
