"""Restatement of glabc_smc_draws (include/glabc.h) from functions the CPU checker already has, and of the generations of
glabcmcmc_amd.smc on numpy arrays.  Not a test.

One draw of id `id` under `seed` from a population (a glabc_kde over host arrays, helpers.kde_struct):
    theta      row id of oracle_kde_sample(population, ., seed, .)
    log_prior  oracle_model_prior_log_prob(model, theta)
    noise, y   as tests/rejection_ref.py: rejection_ref.noise_normals under seed ^ NOISE_KEY, oracle_model_simulate
    distance   oracle_model_discrepancy(model, y), +inf where log_prior == -inf
    accept     the acceptance lines of rejection_ref.restate on that distance, under seed ^ ACCEPT_KEY
"""
import ctypes as C
import math

import numpy as np

import oracle_lib
import rejection_ref as R
from helpers import kde_struct, oracle_fit, rule

SEED_STEP = 0x632BE59BD9B4E019


class HostPopulation:
    """the checker's fit of centres X [S][D] with raw weights w (None: uniform) and its glabc_kde over host arrays; `h`: the rule
    factor, or None with the fixed bandwidth `bw`"""

    def __init__(self, X, w, h=None, bw=None):
        L = oracle_lib.load()
        self.X = np.ascontiguousarray(X, np.float32)
        self.S, self.dim = self.X.shape
        self.w_raw = None if w is None else np.ascontiguousarray(w, np.float32)
        self.xs, self.weights, self.log_w, self.wq, self.consts = oracle_fit(L, self.X, self.w_raw, 0.0 if h is None else h, bw)
        self.cum_q = np.cumsum(self.wq)
        self.bandwidth = self.consts[:self.dim].copy()
        self.struct = kde_struct(self.xs, self.log_w, self.cum_q, self.consts, self.dim, self.S)


def kde_rows(pop, seed, ids):
    """row `id` of oracle_kde_sample for every id -> [n][dim]; consecutive ids go through one call"""
    L = oracle_lib.load()
    ids = np.asarray(ids, np.int64)
    uniq, inverse = np.unique(ids, return_inverse=True)
    rows = np.empty((uniq.size, pop.dim), np.float32)
    starts = np.concatenate([[0], np.nonzero(np.diff(uniq) != 1)[0] + 1, [uniq.size]]) if uniq.size else np.array([0])
    for a, b in zip(starts[:-1], starts[1:]):
        z = np.empty((pop.dim, b - a), np.float32)
        assert L.oracle_kde_sample(C.byref(pop.struct), int(b - a), seed & R.M64, int(uniq[a]), z.ctypes.data) == 0
        rows[a:b] = z.T
    return rows[inverse]


def restate(model, pop, seed, ids):
    """-> theta [n][D], y [n][YD], log_prior [n], distance [n] (+inf outside the prior's support), accept [n] uint8"""
    L = oracle_lib.load()
    ids = np.asarray(ids, np.int64)
    n = ids.size
    theta = np.ascontiguousarray(kde_rows(pop, seed, ids))
    lp = np.empty(n, np.float32)
    assert L.oracle_model_prior_log_prob(C.byref(model), theta.ctypes.data, n, lp.ctypes.data) == 0
    eps = R.noise_normals(seed, ids, model.y_dim)
    y, d0 = np.empty((n, model.y_dim), np.float32), np.empty(n, np.float32)
    assert L.oracle_model_simulate(C.byref(model), theta.ctypes.data, eps.ctypes.data, n, y.ctypes.data) == 0
    assert L.oracle_model_discrepancy(C.byref(model), y.ctypes.data, n, d0.ctypes.data) == 0
    dis = np.where(lp == -np.inf, np.float32(np.inf), d0).astype(np.float32)
    w = R.philox_blocks((seed ^ R.ACCEPT_KEY) & R.M64, ids, 0)
    w0, w1 = np.ascontiguousarray(w[:, 0]), np.ascontiguousarray(w[:, 1])
    u, upos, u64 = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.float64)
    L.oracle_uniforms_v(w0.ctypes.data, w1.ctypes.data, n, u.ctypes.data, upos.ctypes.data, u64.ctypes.data)
    with np.errstate(all="ignore"):
        e = (dis - np.float32(0.0)) / np.float32(model.kern_scale)
        arg = np.ascontiguousarray(-(np.float32(0.5) * (e * e)), np.float32)
    p = np.empty(n, np.float32)
    L.oracle_expf_v(arg.ctypes.data, n, p.ctypes.data)
    return theta, y, lp, dis, (u < p).astype(np.uint8)


# ---------------------------------------------------------------------------------- the generations, on sorted arrays
def generation_key(seed, t):
    return (seed + t * SEED_STEP) & R.M64


def first_generation(model, N, quantile, seed):
    """generation 0 -> theta [N][D], distance [N], epsilon, n_draws: the N nearest of ceil(N / quantile) prior draws, ties by id"""
    n0 = int(math.ceil(N / quantile))
    theta, _, dis, _ = R.restate(model, generation_key(seed, 0), np.arange(n0), accept=False)
    eps, ids = R.hard_select(dis, n_accept=N)
    return theta[ids], dis[ids], float(eps), n0


def next_epsilon(dis, quantile, eps_stop):
    return max(float(np.float32(eps_stop)), float(np.sort(dis)[int(math.floor(quantile * (dis.size - 1)))]))


def hard_generation(model, pop, N, eps, seed, t, block=4096):
    """the first N ids with restated distance <= eps -> ids [N], and their restated rows"""
    kept, start = np.empty(0, np.int64), 0
    while kept.size < N:
        ids = np.arange(start, start + block)
        kept = np.concatenate([kept, ids[restate(model, pop, generation_key(seed, t), ids)[3] <= np.float32(eps)]])
        start += block
    kept = kept[:N]
    return kept, restate(model, pop, generation_key(seed, t), kept)


def silverman_population(theta, weights):
    """the population smc.sample fits by default: Silverman's factor (helpers.rule) times the weighted std"""
    return HostPopulation(theta, np.asarray(weights, np.float32), h=rule("silverman", theta.shape[0], theta.shape[1]))


# ---------------------------------------------------------------------------------- weighted moments
def weighted_second_moment(theta, weights):
    """-> (weighted mean of theta_j^2, its standard error sqrt(sum w_i^2 (f_i - mean)^2)) per coordinate, float64"""
    w = np.asarray(weights, np.float64)
    f = np.asarray(theta, np.float64) ** 2
    mu = (w[:, None] * f).sum(axis=0)
    return mu, np.sqrt(((w * w)[:, None] * (f - mu) ** 2).sum(axis=0))
