"""Restatement of glabc_predictive_draws and glabc_predictive_counts (include/glabc.h) from functions the CPU checker already has
and the histogram and key rules of tests/quantile_ref.py.  Shares no code with csrc/ or with glabcmcmc_amd/predictive.py.  Not a test.

Draw (row t, chain c) of a chain-major history [n_rows][D][stride] has the id  id0 + t * id_step + c  and
    theta   history[t][:][c]
    noise   oracle_philox4x32_10(counter (id_lo, id_hi, 0, b), key seed ^ PREDICTIVE_KEY) -> oracle_normal_pair_v of words (0, 1), (2, 3)
            (rejection_ref.noise_normals, handed the seed that makes its key the predictive one)
    y       oracle_model_simulate(model, theta, noise);   distance   oracle_model_discrepancy(model, y)
The K = y_dim + 1 statistics of a draw are y and then the distance; their tables are quantile_ref.histogram on [lo_k, hi_k], float32
comparisons against threshold_k, and the minimum and maximum of quantile_ref.keys over the values that are no NaN.
"""
import ctypes as C

import numpy as np

import oracle_lib
import quantile_ref as Q
import rejection_ref as R

PREDICTIVE_KEY = 0xA0761D6478BD642F
KEY_NONE = (0xFFFFFFFF, 0)


def ids_of(n_rows, n_chains, id0, id_step):
    """int64 [n_rows][n_chains]"""
    return np.int64(id0) + np.arange(n_rows, dtype=np.int64)[:, None] * np.int64(id_step) + np.arange(n_chains, dtype=np.int64)[None, :]


def restate(model, hist, n_chains, seed, id0, id_step):
    """-> (y float32 [n_rows][y_dim][n_chains], distance float32 [n_rows][n_chains]): the history's layout, columns n_chains .. never read"""
    L = oracle_lib.load()
    hist = np.asarray(hist, np.float32)
    n_rows, d, _ = hist.shape
    n = n_rows * n_chains
    theta = np.ascontiguousarray(hist[:, :, :n_chains].transpose(0, 2, 1).reshape(n, d))
    ids = ids_of(n_rows, n_chains, id0, id_step).reshape(-1)
    eps = R.noise_normals((seed ^ PREDICTIVE_KEY ^ R.NOISE_KEY) & R.M64, ids, model.y_dim)
    y, dis = np.empty((n, model.y_dim), np.float32), np.empty(n, np.float32)
    assert L.oracle_model_simulate(C.byref(model), theta.ctypes.data, eps.ctypes.data, n, y.ctypes.data) == 0
    assert L.oracle_model_discrepancy(C.byref(model), y.ctypes.data, n, dis.ctypes.data) == 0
    return np.ascontiguousarray(y.reshape(n_rows, n_chains, model.y_dim).transpose(0, 2, 1)), dis.reshape(n_rows, n_chains)


def statistics(y, dis):
    """float32 [K][N]: the coordinates of y, then the distance, of every draw"""
    yd = y.shape[1]
    return np.ascontiguousarray(np.concatenate([y.transpose(1, 0, 2).reshape(yd, -1), dis.reshape(1, -1)]))


def counts(stats, n_bins, lo, hi):
    """uint64 [K][n_bins + 3]: the bins, then below, above, NaN -- glabc_histogram's rule, each statistic a coordinate of a one-row history"""
    return Q.histogram(stats[None], n_bins, lo, hi)


def tails(stats, thresholds):
    """uint64 [K][4]: below, equal, above the float32 threshold, NaN"""
    thr = np.asarray(thresholds, np.float32)[:, None]
    x = np.asarray(stats, np.float32)
    with np.errstate(invalid="ignore"):
        return np.stack([(x < thr).sum(axis=1), (x == thr).sum(axis=1), (x > thr).sum(axis=1), np.isnan(x).sum(axis=1)], axis=1).astype(np.uint64)


def extremes(stats):
    """uint32 [K][2]: the smallest and the largest key among the values that are no NaN; KEY_NONE where there is none"""
    out = np.empty((stats.shape[0], 2), np.uint32)
    for k, x in enumerate(stats):
        keys = Q.keys(x[~np.isnan(x)])
        out[k] = (keys.min(), keys.max()) if keys.size else KEY_NONE
    return out
