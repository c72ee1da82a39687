"""Restatement of glabc_weighted_predictive_counts (include/glabc.h) in NumPy.  Not a test.

The float32 statistics [n][K] of the draws -- y and then the distance -- come from tests/predictive_ref.py's functions on the one-row
history [1][D][stride] (draw i has the id id0 + i), the multiplicities m from tests/weighted_ref.py's quantised weight.  The three
tables are then sums of Python integers over the draws with m > 0: a draw of multiplicity 0 is left out everywhere, whatever its
statistics hold.  The bins are tests/joint_ref.py's (what weighted_ref.histogram uses), the key tests/quantile_ref.py's; nothing is
shared with csrc/ or with glabcmcmc_amd/predictive.py.  tests/test_weighted_predictive_host.py holds it to
numpy.histogram(weights=m) and to plain comparisons.
"""
import numpy as np

import joint_ref as J
import predictive_ref as P
import quantile_ref as Q
import weighted_ref as W

KEY_NONE = P.KEY_NONE


def statistics(model, x, n, seed, id0):
    """float32 [n][K] of the draws of the dimension-major x [D][stride], columns n .. never read"""
    x = np.asarray(x, np.float32)
    y, dis = P.restate(model, x[None], n, seed, id0, n)
    return np.ascontiguousarray(P.statistics(y, dis).T)


def multiplicity(w, scale, n=None):
    """Python integers [n]"""
    w = np.asarray(w, np.float32)
    return [int(v) for v in W.multiplicity(w[:len(w) if n is None else n], scale).tolist()]


def slots(v, n_bins, lo, hi):
    """glabc_histogram's slot of float32 values among the n_bins + 3: the bins, then below, above, NaN"""
    v = np.asarray(v, np.float32)
    b = J.axis_bins(v, n_bins, lo, hi)
    with np.errstate(invalid="ignore"):
        below = v.astype(np.float64) < np.float64(lo)
    return np.where(b == J.NAN, n_bins + 2, np.where(b == J.OUTSIDE, np.where(below, n_bins, n_bins + 1), b))


def counts(stats, m, n_bins, lo, hi):
    """Python integers [K][n_bins + 3]"""
    out = [[0] * (n_bins + 3) for _ in range(stats.shape[1])]
    for k in range(stats.shape[1]):
        for s, c in zip(slots(stats[:, k], n_bins, lo[k], hi[k]).tolist(), m):
            if c > 0:
                out[k][s] += c
    return out


def tails(stats, m, thresholds):
    """Python integers [K][4]: below, equal, above the float32 threshold, NaN"""
    thr = np.asarray(thresholds, np.float32)
    out = [[0, 0, 0, 0] for _ in range(stats.shape[1])]
    for k in range(stats.shape[1]):
        for v, c in zip(np.asarray(stats[:, k], np.float32), m):
            if c > 0:
                out[k][0 if v < thr[k] else 1 if v == thr[k] else 2 if v > thr[k] else 3] += c
    return out


def extremes(stats, m):
    """uint32 [K][2]: the smallest and the largest key among the values of positive multiplicity that are no NaN; KEY_NONE where
    there is none"""
    keep = np.array([c > 0 for c in m], bool)
    out = np.empty((stats.shape[1], 2), np.uint32)
    for k in range(stats.shape[1]):
        x = np.asarray(stats[:, k], np.float32)[keep]
        keys = Q.keys(x[~np.isnan(x)])
        out[k] = (keys.min(), keys.max()) if keys.size else KEY_NONE
    return out


def as_u64(table):
    """a table of Python integers -> uint64 array; refuses what no uint64 holds"""
    assert all(0 <= int(v) < 1 << 64 for row in table for v in row)
    return np.array([[int(v) for v in row] for row in table], dtype=np.uint64)
