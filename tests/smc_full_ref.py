"""Restatement of glabc_kde_sample_full / glabc_smc_draws_full (include/glabc.h) from functions the CPU checker already has plus
NumPy float32 arithmetic, and of the full-covariance mixture density in float64.  Not a test.

One draw of id `id` under `seed` from a population (a smc_ref.HostPopulation) and a lower factor L (float32 [D][D]):
    ancestor, normals   those of oracle_kde_sample's row id, read off two probe populations that share the population's integer
                        weights: zero centres under unit bandwidth return the normals (0 + nrm * 1), centres (j, j, ...) under a
                        vanishing bandwidth return the ancestor j
    theta_d             X[j][d] + acc, acc = nrm_0 L[d][0], then acc = acc + nrm_e L[d][e] for e = 1 .. d: NumPy float32 operations,
                        each rounded once
    the rest            the lines of smc_ref.restate behind its theta
"""
import ctypes as C

import numpy as np

import oracle_lib
import rejection_ref as R
import smc_ref as S
from helpers import kde_struct


def pack(L):
    """the HOST array the `_full` entry points take: float32, lower triangle row-major"""
    L = np.asarray(L, np.float32)
    return np.ascontiguousarray([L[d, e] for d in range(L.shape[0]) for e in range(d + 1)], np.float32)


def dense_factor(scales, rho=0.95, seed=0):
    """a dense lower factor whose L L^T has the marginal scales `scales` and the correlations +-rho^|i - j| (neighbours: rho)"""
    s = np.asarray(scales, np.float64)
    d = s.size
    sign = np.where(np.random.default_rng(seed).random(d) < 0.5, -1.0, 1.0)
    i = np.arange(d)
    corr = np.outer(sign, sign) * rho ** np.abs(i[:, None] - i[None, :])
    return np.linalg.cholesky(corr * np.outer(s, s)).astype(np.float32)


class _Probe:
    """a population's glabc_kde with other centres and another bandwidth over the same integer weights"""

    def __init__(self, pop, xs, bw):
        self.dim, self.S = pop.dim, pop.S
        self.xs = np.ascontiguousarray(xs, np.float32)
        self.consts = np.concatenate([np.full(pop.dim, bw, np.float32), pop.consts[pop.dim:]]).astype(np.float32)
        self.log_w, self.cum_q = pop.log_w, pop.cum_q
        self.struct = kde_struct(self.xs, self.log_w, self.cum_q, self.consts, self.dim, self.S)


def ancestors_and_normals(pop, seed, ids):
    """-> j [n] int64, nrm [n][D] float32 of oracle_kde_sample's rows"""
    assert pop.S < 1 << 24
    nrm = S.kde_rows(_Probe(pop, np.zeros((pop.dim, pop.S)), 1.0), seed, ids)
    index = np.broadcast_to(np.arange(pop.S, dtype=np.float32), (pop.dim, pop.S))
    j = np.rint(S.kde_rows(_Probe(pop, index, 1e-30), seed, ids)[:, 0]).astype(np.int64)
    assert (j >= 0).all() and (j < pop.S).all()
    return j, nrm


def theta_rows(pop, L, seed, ids):
    """row `id` of glabc_kde_sample_full(pop, L) for every id -> [n][D] float32"""
    L = np.asarray(L, np.float32)
    j, nrm = ancestors_and_normals(pop, seed, ids)
    theta = np.empty((j.size, pop.dim), np.float32)
    for d in range(pop.dim):
        acc = nrm[:, 0] * L[d, 0]
        for e in range(1, d + 1):
            acc = acc + nrm[:, e] * L[d, e]
        theta[:, d] = pop.X[j, d] + acc
    assert theta.dtype == np.float32
    return theta


def restate(model, pop, L, seed, ids):
    """-> theta [n][D], y [n][YD], log_prior [n], distance [n] (+inf outside the prior's support), accept [n] uint8: smc_ref.restate
    with theta_rows for its theta"""
    lib = oracle_lib.load()
    ids = np.asarray(ids, np.int64)
    n = ids.size
    theta = np.ascontiguousarray(theta_rows(pop, L, seed, ids))
    lp = np.empty(n, np.float32)
    assert lib.oracle_model_prior_log_prob(C.byref(model), theta.ctypes.data, n, lp.ctypes.data) == 0
    eps = R.noise_normals(seed, ids, model.y_dim)
    y, d0 = np.empty((n, model.y_dim), np.float32), np.empty(n, np.float32)
    assert lib.oracle_model_simulate(C.byref(model), theta.ctypes.data, eps.ctypes.data, n, y.ctypes.data) == 0
    assert lib.oracle_model_discrepancy(C.byref(model), y.ctypes.data, n, d0.ctypes.data) == 0
    dis = np.where(lp == -np.inf, np.float32(np.inf), d0).astype(np.float32)
    w = R.philox_blocks((seed ^ R.ACCEPT_KEY) & R.M64, ids, 0)
    w0, w1 = np.ascontiguousarray(w[:, 0]), np.ascontiguousarray(w[:, 1])
    u, upos, u64 = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.float64)
    lib.oracle_uniforms_v(w0.ctypes.data, w1.ctypes.data, n, u.ctypes.data, upos.ctypes.data, u64.ctypes.data)
    with np.errstate(all="ignore"):
        e = (dis - np.float32(0.0)) / np.float32(model.kern_scale)
        arg = np.ascontiguousarray(-(np.float32(0.5) * (e * e)), np.float32)
    p = np.empty(n, np.float32)
    lib.oracle_expf_v(arg.ctypes.data, n, p.ctypes.data)
    return theta, y, lp, dis, (u < p).astype(np.uint8)


def hard_generation(model, pop, L, N, eps, seed, t, block=4096):
    """the first N ids with restated distance <= eps -> ids [N], and their restated rows (smc_ref.hard_generation)"""
    kept, start = np.empty(0, np.int64), 0
    while kept.size < N:
        ids = np.arange(start, start + block)
        kept = np.concatenate([kept, ids[restate(model, pop, L, S.generation_key(seed, t), ids)[3] <= np.float32(eps)]])
        start += block
    kept = kept[:N]
    return kept, restate(model, pop, L, S.generation_key(seed, t), kept)


# ---------------------------------------------------------------------------------- the density, float64
def log_q(theta, X, weights, L):
    """log sum_j w_j N(theta; x_j, L L^T) in float64 -> [n]; theta [n][D], X [S][D], weights [S] (normalised here), L [D][D] lower"""
    theta, X, L = np.asarray(theta, np.float64), np.asarray(X, np.float64), np.asarray(L, np.float64)
    w = np.asarray(weights, np.float64)
    w = w / w.sum()
    Linv = np.linalg.inv(L)
    e = (theta[:, None, :] - X[None, :, :]) @ Linv.T                       # [n][S][D]: L^-1 (theta - x_j)
    with np.errstate(divide="ignore"):
        t = np.log(w)[None, :] - 0.5 * (e * e).sum(axis=2)
    m = t.max(axis=1)
    return m + np.log(np.exp(t - m[:, None]).sum(axis=1)) - np.log(np.diagonal(L)).sum() - 0.5 * X.shape[1] * np.log(2.0 * np.pi)


def weighted_moments(theta, weights):
    """-> weighted mean [D], covariance [D][D], and the standard errors of both (delta method on the normalised weights: sqrt(sum
    w_i^2 (f_i - mean f)^2)), float64"""
    w = np.asarray(weights, np.float64)
    x = np.asarray(theta, np.float64)
    mean = w @ x
    xc = x - mean
    outer = xc[:, :, None] * xc[:, None, :]
    cov = np.einsum("i,ijk->jk", w, outer)
    se_mean = np.sqrt((w * w) @ (xc * xc))
    se_cov = np.sqrt(np.einsum("i,ijk->jk", w * w, (outer - cov) ** 2))
    return mean, cov, se_mean, se_cov


# ---------------------------------------------------------------------------------- the correlated linear Model
# theta in R^2, prior N(0, 3^2 I), y = (theta_1 + theta_2, 0.1 (theta_1 - theta_2)) + 0.05 z, y_obs = (1, 0), Gaussian ABC kernel at
# epsilon = 0.05 on the Euclidean distance: y | theta ~ N(A theta, (0.05^2 + 0.05^2) I), so the posterior is Gaussian
CORR_A = np.array([[1.0, 1.0], [0.1, -0.1]])
CORR_Y_OBS = np.array([1.0, 0.0])
CORR_NOISE, CORR_EPS, CORR_PRIOR = 0.05, 0.05, 3.0


def correlated_posterior():
    """-> mean [2], covariance [2][2] of the ABC posterior the samplers target (correlation -0.980)"""
    s2 = CORR_NOISE ** 2 + CORR_EPS ** 2
    cov = np.linalg.inv(np.eye(2) / CORR_PRIOR ** 2 + CORR_A.T @ CORR_A / s2)
    return cov @ (CORR_A.T @ CORR_Y_OBS / s2), cov
