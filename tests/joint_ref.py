"""The joint posterior restated in NumPy: the specifications of glabc_histogram2d and glabc_cross_moments (include/glabc.h) -- the
bin arithmetic of glabc_histogram on two axes and the three special slots; float64 sums of centred products in exactly the stated
order -- and the pooled covariance and highest-density formulas of glabcmcmc_amd/diagnostics.py.  Shares no code with csrc/ or with
diagnostics.py.  The counts are vectorised over values only, the moments over chains only (a loop over rows).
tests/test_joint_host.py checks it against numpy.histogram2d, numpy.cov, the marginal restatement (tests/quantile_ref.py) and
glabc_autocov's (tests/diag_ref.py); tests/test_joint_shapes.py holds the kernels and the module to it.

Histories here are chain-major float32 [n_rows][d][stride], as the samplers write them.
"""
import numpy as np

OUTSIDE, NAN = -1, -2


# ---------------------------------------------------------------------------------- glabc_histogram2d
def axis_bins(x, n_bins, lo, hi):
    """float32 values -> int64 bins on one axis; OUTSIDE below lo or above hi, NAN"""
    with np.errstate(invalid="ignore"):                               # a signalling NaN
        x = np.asarray(x).astype(np.float64)
    l, h = np.float64(lo), np.float64(hi)
    scale = np.float64(n_bins) / (h - l)
    out = np.empty(x.size, np.int64)
    nan = np.isnan(x)
    with np.errstate(invalid="ignore"):
        off, top = (x < l) | (x > h), x == h
        inside = ~(nan | off | top)
        out[nan], out[off], out[top] = NAN, OUTSIDE, n_bins - 1
        u = (x[inside] - l) * scale
    out[inside] = np.minimum(np.floor(u).astype(np.int64), n_bins - 1)
    return out


def histogram2d(hist, pairs, n_bins, lo, hi, n_chains=None):
    """-> uint64 [P][n_bins^2 + 2]: the cells (bin_a * n_bins + bin_b), then outside, then NaN; columns n_chains .. are never read"""
    n_rows, d, stride = hist.shape
    n = stride if n_chains is None else n_chains
    cells = n_bins * n_bins
    out = np.zeros((len(pairs), cells + 2), np.uint64)
    for p, (a, b) in enumerate(pairs):
        ba = axis_bins(np.asarray(hist)[:, a, :n].reshape(-1), n_bins, lo[a], hi[a])
        bb = axis_bins(np.asarray(hist)[:, b, :n].reshape(-1), n_bins, lo[b], hi[b])
        slot = ba * n_bins + bb
        slot[(ba == OUTSIDE) | (bb == OUTSIDE)] = cells
        slot[(ba == NAN) | (bb == NAN)] = cells + 1                   # a NaN on either axis comes first
        out[p] = np.bincount(slot, minlength=cells + 2).astype(np.uint64)
    return out


# ---------------------------------------------------------------------------------- glabc_cross_moments
def packed_index(i, j, d):
    return i * d - i * (i - 1) // 2 + (j - i)


def cross_moments(hist, n_chains=None):
    """-> (mean [d][n], cov [d (d + 1) / 2][n]) float64, every sum t ascending, one rounded operation per step"""
    n_rows, d, stride = hist.shape
    n = stride if n_chains is None else n_chains
    with np.errstate(all="ignore"):
        x = np.asarray(hist)[:, :, :n].astype(np.float64)
        s = np.zeros((d, n))
        for t in range(n_rows):
            s = s + x[t]
        m = s / float(n_rows)
        u = x - m
        cov = np.empty((d * (d + 1) // 2, n))
        for i in range(d):
            for j in range(i, d):
                a = np.zeros(n)
                for t in range(n_rows):
                    prod = u[t, i] * u[t, j]
                    a = a + prod
                cov[packed_index(i, j, d)] = a / float(n_rows)
    return m, cov


# ---------------------------------------------------------------------------------- the pooled covariance
def covariance(hist):
    """-> float64 [d][d]: (n sum_c cov_c + n sum_c (m_c - m)(m_c - m)^T) / (M n - 1), m the mean over chains of the m_c"""
    n_rows, d, m_chains = hist.shape
    mean, cov = cross_moments(hist)
    dev = mean - mean.mean(axis=1, keepdims=True)
    out = np.empty((d, d))
    for i in range(d):
        for j in range(i, d):
            within = cov[packed_index(i, j, d)].sum()
            between = (dev[i] * dev[j]).sum()
            out[i, j] = out[j, i] = (n_rows * within + n_rows * between) / (m_chains * n_rows - 1.0)
    return out


def correlation(hist):
    v = covariance(hist)
    with np.errstate(all="ignore"):
        sd = np.sqrt(np.diag(v))
        r = v / sd[:, None] / sd[None, :]
    r[sd == 0.0, :] = np.nan
    r[:, sd == 0.0] = np.nan
    return r


# ---------------------------------------------------------------------------------- highest-density levels
def hpd_level(grid, p):
    """one grid of Python integers, one probability -> (need, level, mass, bins inside), by trying every count value"""
    g = [int(v) for v in np.asarray(grid).reshape(-1)]
    total = sum(g)
    need = min(int(np.ceil(np.float64(p) * np.float64(total))), total)          # one rounded product
    for v in sorted(set(g), reverse=True):
        mass = sum(x for x in g if x >= v)
        if mass >= need:
            return need, v, mass, sum(1 for x in g if x >= v)
    raise AssertionError("no level reaches need = %d of %d" % (need, total))
