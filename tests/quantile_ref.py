"""Posterior quantiles and histograms restated in NumPy, vectorised over values only: the specification of glabc_key_counts and
glabc_histogram (include/glabc.h) -- the order-preserving key of a float32, the three levels of digits, the bin arithmetic -- and
the quantile formula of glabcmcmc_amd/diagnostics.py.  Shares no code with csrc/ or with diagnostics.py;
tests/test_quantile_host.py checks it against numpy.sort, numpy.quantile and numpy.histogram, tests/test_quantile_shapes.py holds
the kernels and the module to it.

Histories here are chain-major float32 [n_rows][d][stride], as the samplers write them.
"""
import numpy as np

LEVELS = ((0, 11), (11, 11), (22, 10))          # (prefix bits, digit bits)
UNUSED = 0xFFFFFFFF


# ---------------------------------------------------------------------------------- inputs
def special_values():
    """float32 [40]: +-0, +-denormals, +-inf, two NaNs of either sign, ties, a constant run, neighbours in the last bit"""
    bits = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,
                     0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7F7FFFFF, 0xFF7FFFFF,
                     0x3F800000, 0x3F800001, 0x3F7FFFFF, 0xBF800000, 0xBF800001, 0xBF7FFFFF, 0x3F800000, 0x3F800000,
                     0x40490FDB, 0x40490FDB, 0xC0490FDB, 0x00000000, 0x80000000, 0x42280000], np.uint32).view(np.float32)
    out = np.concatenate([bits, np.full(10, np.float32(2.5))])
    out.setflags(write=False)
    return out


def special_history(n_rows, d, n_chains):
    """the special values tiled over a chain-major history, a different rotation per coordinate and row"""
    v = special_values()
    i = (np.arange(n_rows)[:, None, None] * 7 + np.arange(d)[None, :, None] * 3 + np.arange(n_chains)[None, None, :]) % v.size
    return np.ascontiguousarray(v[i])


# ---------------------------------------------------------------------------------- the key
def keys(x):
    x = np.asarray(x, np.float32)
    u = np.ascontiguousarray(x).view(np.uint32).copy()
    u[x == 0] = 0
    k = np.where(u >> 31 == 1, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(x)] = UNUSED
    return k


def unkey(k):
    k = np.asarray(k, np.uint32)
    u = np.where(k >> 31 == 1, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    out = u.view(np.float32).copy()
    out[k == UNUSED] = np.nan
    return out


# ---------------------------------------------------------------------------------- glabc_key_counts
def key_counts(hist, level, prefixes=None, n_chains=None):
    """-> uint64 [d][P][2^digit_bits]; prefixes: integers [d][P] (None at level 0: P = 1); columns n_chains .. are never read"""
    n_rows, d, stride = hist.shape
    n = stride if n_chains is None else n_chains
    prefix_bits, digit_bits = LEVELS[level]
    table = np.zeros((d, 1), np.uint32) if prefixes is None else np.asarray(prefixes).astype(np.uint32)
    out = np.zeros((d, table.shape[1], 1 << digit_bits), np.uint64)
    for j in range(d):
        k = keys(np.asarray(hist)[:, j, :n].reshape(-1)).astype(np.uint64)
        digit = (k >> np.uint64(32 - prefix_bits - digit_bits)) & np.uint64((1 << digit_bits) - 1)
        for s, p in enumerate(table[j]):
            if level > 0 and int(p) == UNUSED:
                continue
            mine = digit if level == 0 else digit[k >> np.uint64(32 - prefix_bits) == np.uint64(p)]
            out[j, s] = np.bincount(mine.astype(np.int64), minlength=1 << digit_bits).astype(np.uint64)
    return out


def selection_prefixes(hist, level, ranks, n_chains=None):
    """the prefixes a selection of `ranks` walks at `level`, from a sort: ascending distinct integers per coordinate, [d] lists"""
    n_rows, d, stride = hist.shape
    n = stride if n_chains is None else n_chains
    out = []
    for j in range(d):
        k = np.sort(keys(np.asarray(hist)[:, j, :n].reshape(-1)))
        out.append(sorted({int(k[r]) >> (32 - LEVELS[level][0]) for r in ranks}))
    return out


# ---------------------------------------------------------------------------------- glabc_histogram
def histogram(hist, n_bins, lo, hi, n_chains=None):
    """-> uint64 [d][n_bins + 3]: the bins, then below, above, NaN"""
    n_rows, d, stride = hist.shape
    n = stride if n_chains is None else n_chains
    out = np.zeros((d, n_bins + 3), np.uint64)
    for j in range(d):
        x = np.asarray(hist)[:, j, :n].reshape(-1).astype(np.float64)
        l, h = np.float64(lo[j]), np.float64(hi[j])
        scale = np.float64(n_bins) / (h - l)
        slot = np.empty(x.size, np.int64)
        nan, below, above, top = np.isnan(x), x < l, x > h, x == h
        inside = ~(nan | below | above | top)
        slot[nan], slot[below], slot[above], slot[top] = n_bins + 2, n_bins, n_bins + 1, n_bins - 1
        u = (x[inside] - l) * scale
        slot[inside] = np.minimum(np.floor(u).astype(np.int64), n_bins - 1)
        out[j] = np.bincount(slot, minlength=n_bins + 3).astype(np.uint64)
    return out


# ---------------------------------------------------------------------------------- the quantile formula
def quantile_of_sorted(s, q):
    """s: float32 ascending (NaNs last) -> float64, NumPy's default linear rule on two order statistics"""
    n = s.size
    if np.isnan(s[-1]):
        return np.float64(np.nan)
    h = np.float64(q) * np.float64(n - 1)
    lo = int(np.floor(h))
    hi = min(lo + 1, n - 1)
    return np.float64(s[lo]) + (h - np.floor(h)) * (np.float64(s[hi]) - np.float64(s[lo]))


def quantile(hist, q, n_chains=None):
    """-> float64 [Q][d]"""
    n_rows, d, stride = hist.shape
    n = stride if n_chains is None else n_chains
    out = np.empty((len(q), d))
    with np.errstate(invalid="ignore"):
        for j in range(d):
            s = np.sort(np.asarray(hist)[:, j, :n].reshape(-1))
            out[:, j] = [quantile_of_sorted(s, v) for v in q]
    return out
