"""Restatement of glabc_coverage_counts (include/glabc.h) from functions the CPU checker already has.  Not a test.

    table     rejection_ref.restate(model, seed, row0 + arange(n)): theta_i, y_i of glabc_abc_draws
    distance  oracle_model_discrepancy(a copy of the Model with y_obs := y*_r, y_i)
    hard      m = d <= width_r
    model     e = (d - 0) / width_r;  p = oracle_expf_v(-(0.5 (e e)));  m = rint(p 65536), a NaN p: 0      every operation rounded to
              float32 by NumPy
    sums      mass, mass2, below in Python integers

``counts`` takes the table and a distance function, so that the tests can feed it another distance (the generic path's) or another
table; ``sort_rank`` is the per-test tolerance of ``quantile=`` on numpy.sort.
"""
import copy
import ctypes as C

import numpy as np

import oracle_lib
import rejection_ref as R


def table(model, seed, row0, n):
    """-> theta [n][D], y [n][YD] of table draws row0 .. row0 + n - 1"""
    theta, y, _, _ = R.restate(model, seed, np.arange(n, dtype=np.int64) + row0, accept=False)
    return theta, y


def oracle_distance(model):
    """-> distance(y [n][YD], y_star [YD]) -> [n] float32: oracle_model_discrepancy of a copy of `model` whose y_obs is y_star"""
    L = oracle_lib.load()

    def distance(y, y_star):
        m = copy.copy(model)
        m.y_obs = type(model.y_obs)(*([float(v) for v in y_star] + [0.0] * (8 - len(y_star))))
        y = np.ascontiguousarray(y, np.float32)
        out = np.empty(y.shape[0], np.float32)
        assert L.oracle_model_discrepancy(C.byref(m), y.ctypes.data, y.shape[0], out.ctypes.data) == 0
        return out
    return distance


def multiplicity(d, width, kernel):
    """-> int64 [n]"""
    d, width = np.asarray(d, np.float32), np.float32(width)
    with np.errstate(all="ignore"):
        if kernel == "hard":
            return (d <= width).astype(np.int64)
        e = (d - np.float32(0.0)) / width
        arg = np.ascontiguousarray(-(np.float32(0.5) * (e * e)), np.float32)
        p = np.empty(d.size, np.float32)
        oracle_lib.load().oracle_expf_v(arg.ctypes.data, d.size, p.ctypes.data)
        m = np.rint(p * np.float32(65536.0))
    return np.where(np.isnan(p), 0.0, m).astype(np.int64)


def pair_multiplicities(y, y_star, widths, kernel, distance):
    """-> m [R][n] int64: every pair's multiplicity"""
    return np.stack([multiplicity(distance(y, y_star[t]), widths[t], kernel) for t in range(y_star.shape[0])])


def sums(m, theta, theta_star):
    """pair multiplicities m [R][n] -> mass [R], mass2 [R], below [R][D] as Python integers in object arrays.  The partial sums are
    formed in int64, which is exact here: m <= 2^16, so n < 2^31 squares stay below 2^63"""
    r, d = theta_star.shape
    assert m.shape[1] < (1 << 31) and (m.size == 0 or (0 <= m.min() and m.max() <= 65536))
    mass, mass2, below = np.zeros(r, object), np.zeros(r, object), np.zeros((r, d), object)
    for t in range(r):
        mass[t], mass2[t] = int(m[t].sum()), int((m[t] * m[t]).sum())
        with np.errstate(invalid="ignore"):
            lower = theta < theta_star[t]                               # a tie or a NaN is not below
        for j in range(d):
            below[t, j] = int(m[t][lower[:, j]].sum())
    return mass, mass2, below


def counts(theta, y, theta_star, y_star, widths, kernel, distance):
    """-> mass [R], mass2 [R], below [R][D] as Python integers in object arrays"""
    return sums(pair_multiplicities(y, y_star, widths, kernel, distance), theta, theta_star)


def restate(model, seed, row0, n, theta_star, y_star, widths, kernel):
    theta, y = table(model, seed, row0, n)
    return counts(theta, y, np.asarray(theta_star, np.float32), np.asarray(y_star, np.float32), np.asarray(widths, np.float32), kernel,
                  oracle_distance(model))


def sort_rank(dis, rank):
    """the distance of rank `rank` in ascending order, NaNs last (numpy.sort's order)"""
    return np.sort(np.asarray(dis, np.float32))[rank]
