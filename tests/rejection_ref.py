"""Restatement of glabc_abc_draws (include/glabc.h) from functions the CPU checker already has, the selection rules of
glabcmcmc_amd.rejection on numpy.sort, and the analytic posterior of Mixture_set.  Not a test.

One draw of id `id` under `seed`:
    theta   oracle_dist_forward_philox(prior, seed, row0 = id)
    noise   oracle_philox4x32_10(counter (id_lo, id_hi, 0, b), key seed ^ NOISE_KEY) -> oracle_normal_pair_v of words (0, 1), (2, 3)
    y       oracle_model_simulate(model, theta, noise);   distance   oracle_model_discrepancy(model, y)
    accept  u = oracle_uniforms_v(word 0 of Philox(counter (id_lo, id_hi, 0, 0), key seed ^ ACCEPT_KEY));
            e = (dis - 0) / kern_scale;  p = oracle_expf_v(-(0.5 (e e)));  u < p       every operation rounded to float32 by NumPy

Analytic posterior of Mixture_set (y = |theta| + N(0, s2 I), s2 = 0.05, prior N(0, I), Gaussian kernel of width eps on the
Euclidean distance): the kernel factorises over coordinates, so per coordinate the posterior is proportional to
N(theta; 0, 1) N(y_obs; |theta|, s2 + eps^2) and the acceptance rate of kernel="model" is
(sqrt(eps^2 / (s2 + eps^2)) Z / sqrt(2 pi))^D with Z = int exp(-theta^2 / 2) exp(-(y_obs - |theta|)^2 / (2 (s2 + eps^2))) dtheta.
"""
import ctypes as C

import numpy as np

import oracle_lib

NOISE_KEY = 0x9E3779B97F4A7C15
ACCEPT_KEY = 0xD1B54A32D192ED03
M64 = (1 << 64) - 1


def philox_blocks(key, ids, block):
    """words [n][4] of Philox(key; id_lo, id_hi, 0, block) for every id"""
    L = oracle_lib.load()
    ids = np.asarray(ids, np.uint64)
    n = ids.size
    ctr = np.zeros((n, 4), np.uint32)
    ctr[:, 0] = (ids & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    ctr[:, 1] = (ids >> np.uint64(32)).astype(np.uint32)
    ctr[:, 3] = block
    k = np.array([key & 0xFFFFFFFF, (key >> 32) & 0xFFFFFFFF], np.uint32)
    out = np.empty((n, 4), np.uint32)
    f, c0, o0, kp = L.oracle_philox4x32_10, ctr.ctypes.data, out.ctypes.data, k.ctypes.data
    for i in range(n):
        f(c0 + 16 * i, kp, o0 + 16 * i)
    return out


def prior_draws(dist, seed, ids):
    """row `id` of oracle_dist_forward_philox for every id -> [n][dim]; consecutive ids go through one call"""
    L = oracle_lib.load()
    ids = np.asarray(ids, np.int64)
    uniq, inverse = np.unique(ids, return_inverse=True)
    rows = np.empty((uniq.size, dist.dim), np.float32)
    starts = np.concatenate([[0], np.nonzero(np.diff(uniq) != 1)[0] + 1, [uniq.size]]) if uniq.size else np.array([0])
    for a, b in zip(starts[:-1], starts[1:]):
        z, lp = np.empty((dist.dim, b - a), np.float32), np.empty(b - a, np.float32)
        assert L.oracle_dist_forward_philox(C.byref(dist), int(b - a), seed & M64, int(uniq[a]), z.ctypes.data, lp.ctypes.data) == 0
        rows[a:b] = z.T
    return rows[inverse]


def noise_normals(seed, ids, y_dim):
    L = oracle_lib.load()
    n = len(ids)
    eps = np.empty((n, 8), np.float32)
    for b in range((y_dim + 3) // 4):
        w = philox_blocks((seed ^ NOISE_KEY) & M64, ids, b)
        for pair in range(2):
            wa, wb = np.ascontiguousarray(w[:, 2 * pair]), np.ascontiguousarray(w[:, 2 * pair + 1])
            z0, z1 = np.empty(n, np.float32), np.empty(n, np.float32)
            L.oracle_normal_pair_v(wa.ctypes.data, wb.ctypes.data, n, z0.ctypes.data, z1.ctypes.data)
            eps[:, 4 * b + 2 * pair], eps[:, 4 * b + 2 * pair + 1] = z0, z1
    return np.ascontiguousarray(eps[:, :y_dim])


def restate(model, seed, ids, accept=True):
    """-> theta [n][D], y [n][YD], distance [n], accept [n] uint8 (None if not asked) of the draws `ids` (any integers >= 0)"""
    L = oracle_lib.load()
    ids = np.asarray(ids, np.int64)
    n = ids.size
    theta = np.ascontiguousarray(prior_draws(model.prior, seed, ids))
    eps = noise_normals(seed, ids, model.y_dim)
    y, dis = np.empty((n, model.y_dim), np.float32), np.empty(n, np.float32)
    assert L.oracle_model_simulate(C.byref(model), theta.ctypes.data, eps.ctypes.data, n, y.ctypes.data) == 0
    assert L.oracle_model_discrepancy(C.byref(model), y.ctypes.data, n, dis.ctypes.data) == 0
    if not accept:
        return theta, y, dis, None
    w = philox_blocks((seed ^ ACCEPT_KEY) & M64, ids, 0)
    w0, w1 = np.ascontiguousarray(w[:, 0]), np.ascontiguousarray(w[:, 1])
    u, upos, u64 = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.float64)
    L.oracle_uniforms_v(w0.ctypes.data, w1.ctypes.data, n, u.ctypes.data, upos.ctypes.data, u64.ctypes.data)
    with np.errstate(all="ignore"):
        e = (dis - np.float32(0.0)) / np.float32(model.kern_scale)
        arg = np.ascontiguousarray(-(np.float32(0.5) * (e * e)), np.float32)
    p = np.empty(n, np.float32)
    L.oracle_expf_v(arg.ctypes.data, n, p.ctypes.data)
    return theta, y, dis, (u < p).astype(np.uint8)


# ---------------------------------------------------------------------------------- the selection rules, on numpy.sort
def hard_select(dis, epsilon=None, n_accept=None, quantile=None):
    """-> (epsilon float32, kept positions ascending) by the rules of glabcmcmc_amd.rejection; ValueError where the rank is a NaN"""
    dis = np.asarray(dis, np.float32)
    n = dis.size
    if epsilon is not None:
        eps = np.float32(epsilon)
        return eps, np.nonzero(dis <= eps)[0]
    rank = n_accept - 1 if n_accept is not None else int(np.floor(quantile * (n - 1)))
    eps = np.sort(dis)[rank]                                       # NaNs sort last
    if np.isnan(eps):
        raise ValueError("rank %d is a NaN" % rank)
    if n_accept is None:
        return eps, np.nonzero(dis <= eps)[0]
    less, ties = np.nonzero(dis < eps)[0], np.nonzero(dis == eps)[0]
    return eps, np.sort(np.concatenate([less, ties[:n_accept - less.size]]))


# ---------------------------------------------------------------------------------- the analytic posterior of Mixture_set
def analytic(eps, y_obs=1.5, s2=0.05, dim=2):
    """-> (acceptance rate of kernel="model" at `dim` coordinates, E theta_j^2, E theta_j^4) by quadrature (float64)"""
    v = s2 + eps * eps
    t = np.linspace(-12.0, 12.0, 2400001)
    w = np.exp(-0.5 * t * t) * np.exp(-(y_obs - np.abs(t)) ** 2 / (2.0 * v))
    h = t[1] - t[0]
    integral = lambda f: float(np.sum(f) - 0.5 * (f[0] + f[-1])) * h          # noqa: E731 -- trapezoid; the integrand is smooth but for the kink at 0
    z = integral(w)
    rate1 = np.sqrt(eps * eps / v) * z / np.sqrt(2.0 * np.pi)
    return rate1 ** dim, integral(w * t ** 2) / z, integral(w * t ** 4) / z


def law_check(theta, n_draws, eps, n_se=5.0, dim=2):
    """the two law checks (accepted count, E theta_j^2) on accepted draws theta [m][dim] of n_draws: -> list of (name, value, expected, se)"""
    rate, m2, m4 = analytic(eps, dim=dim)
    m = theta.shape[0]
    out = [("accepted", m, n_draws * rate, np.sqrt(n_draws * rate * (1.0 - rate)))]
    se = np.sqrt((m4 - m2 * m2) / m)
    for j in range(dim):
        out.append(("E theta_%d^2" % j, float(np.mean(np.asarray(theta[:, j], np.float64) ** 2)), m2, se))
    for name, value, want, s in out:
        print("%s: %.6g, expected %.6g, %.2f SE" % (name, value, want, (value - want) / s))
        assert abs(value - want) <= n_se * s, (name, value, want, s)
    return out


def abs_gauss_model(dim, prior, epsilon=0.05, y_obs=None):
    """the d-parameter |theta| + noise Model (helpers.AbsGaussModel) with `prior` a distribution.* object as its prior"""
    import helpers
    m = helpers.AbsGaussModel(epsilon, [1.5 - 0.1 * j for j in range(dim)] if y_obs is None else y_obs)
    m._prior = lambda: prior
    return m
