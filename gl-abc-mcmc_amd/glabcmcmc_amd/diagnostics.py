"""diagnostics -- split-R-hat and effective sample size of many chains, from a history that stays on the GPU.

The per-chain work -- means and lagged autocovariances in float64, ``glabc_autocov`` of include/glabc.h -- runs in the
gfx950 kernels of csrc/glabc_diag.hip whatever device the history lives on (a CPU array is staged to the GPU; there is no CPU
implementation).  What is left is a few hundred numbers per coordinate: the chains' sums leave the device and the formulas
below run in NumPy float64.

History layouts: what ``esjd`` takes, ``(T, D)`` or ``(T, C, D)``, torch or NumPy, CPU or CUDA; ``layout="chain_major"`` for
``(T, D, C)``.  The ``(T, C, D)`` view the samplers return with ``return_device=True`` is used in place: its
``permute(0, 2, 1)`` is the contiguous chain-major buffer the kernels read, so the history is not copied.

Formulas (BDA3 / Stan, without rank normalisation).  M chains of n draws; mean_c and acov_k,c are chain c's mean and
biased (1/n) autocovariance at lag k, per coordinate:

    s2_c   = acov_0,c * n / (n - 1)
    W      = mean_c s2_c
    B / n  = the unbiased variance over chains of mean_c        (0 when M = 1)
    var+   = (n - 1) / n * W + B / n
    R-hat  = sqrt(var+ / W)
    rho_0  = 1,   rho_k = 1 - (W - n / (n - 1) * mean_c acov_k,c) / var+
    P_j    = rho_2j + rho_2j+1                                  for 2j + 1 <= max_lag

Geyer's initial positive, monotone sequence: stop at the first j >= 1 with P_j < 0; before that P_j = min(P_j, P_j-1);
tau = -1 + 2 sum_j P_j and ESS = M n / tau.  ``truncated`` says that no negative pair was met within ``max_lag``: ESS is then
an upper bound.  W == 0 (every chain constant) gives NaN for R-hat and ESS, no exception.  Split-R-hat is the same R-hat
of the 2M half-chains of length n // 2 (rows [0, n // 2) and [n - n // 2, n)).

``terms`` reduces a shard of chains to additive sufficient statistics and ``combine`` adds shards up, so ranks that hold
different chains all-reduce ``pack(terms)`` (or gather it with ``parallel.gather_rows``) and every rank evaluates ``rhat`` /
``ess`` of the whole job.

Posterior quantiles and marginal histograms.  ``quantile`` / ``interval`` / ``order_statistics`` / ``histogram`` read the same
history in place and give what ``numpy.sort`` of all T * C draws of a coordinate would, exactly, without sorting: a radix
selection on an order-preserving uint32 key of the float32 values (include/glabc.h: -0 and +0 are one value, NaNs sort last) in
three passes of 11, 11 and 10 bits.  Each pass is one ``glabc_key_counts`` launch (csrc/glabc_quant.hip) that counts, per
coordinate and per wanted key prefix, how many values fall on each digit; ``select`` walks the cumulative counts on the host.
The counts are integers: the same bits in every launch geometry, and additive over shards of chains, so a sharded job passes
``select`` a ``count_fn`` that all-reduces ``key_counts`` of its shard and every rank walks the same prefixes to the exact
quantiles of the whole job.  ``histogram`` is one ``glabc_histogram`` launch, its default range the exact minimum and maximum.
No slab of chains is ever cut for these: the kernels index with 64-bit scalars and size their own grid.

The joint posterior.  ``histogram2d`` counts pairs of coordinates into bins x bins grids (``glabc_histogram2d``,
csrc/glabc_joint.hip: the marginal histogram's bin arithmetic on both axes, integer counts, additive over shards of chains under
an explicit range); ``hpd_levels`` / ``hpd_mask`` read the highest-density levels and regions off a grid on the host -- what a
filled contour plot of (theta_i, theta_j) draws.  ``cross_moments`` gives every chain's means and covariance of all pairs of
coordinates in float64 in a specified order (``glabc_cross_moments``); ``joint_terms`` reduces a shard of chains to additive
sums, ``combine_joint`` adds shards, and ``covariance`` / ``correlation`` are those of all M n pooled draws:

    cov = (n sum_c cov_c + n sum_c (m_c - m)(m_c - m)^T) / (M n - 1),      m the grand mean

Out of scope: rank-normalised bulk / tail ESS (selection gives a few ranks, not all of them), per-chain ESS (``autocovariance``
returns the per-chain numbers), multivariate ESS, weighted draws, grids in more than two dimensions or with unequal bin counts
per axis, kernel smoothing of a grid, and accumulating lagged products or any of the above inside the sampler kernels.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _capi, engine

MAX_LAG = 4096                    # GLABC_MAX_LAG
DEFAULT_MAX_LAG = 256
_SLAB_BYTES = 256 << 20           # device scratch of one glabc_autocov call inside terms(): at most this, and a quarter of the history

# additive over shards of chains (M adds up, n and half_n must agree); the half_* fields have a leading axis of 2
Terms = namedtuple("Terms", "M n sum_mean sum_mean_sq sum_acov half_n half_sum_mean half_sum_mean_sq half_sum_acov0")
Ess = namedtuple("Ess", "ess tau truncated max_lag")

KEY_LEVELS = ((0, 11), (11, 11), (22, 10))         # (prefix bits, digit bits) of the three passes, include/glabc.h
MAX_PREFIXES = 8                  # GLABC_MAX_PREFIXES: prefixes per coordinate of one glabc_key_counts launch
MAX_BINS = 4096                   # GLABC_MAX_BINS
UNUSED_PREFIX = 0xFFFFFFFF        # a slot of a prefix table that counts nothing; also the key of every NaN
Histogram = namedtuple("Histogram", "counts edges below above nan")
MAX_PAIRS = 28                    # GLABC_MAX_PAIRS: pairs of one glabc_histogram2d launch
MAX_JOINT_BINS = 128              # GLABC_MAX_JOINT_BINS, per axis
JointHistogram = namedtuple("JointHistogram", "counts pairs edges outside nan")
# additive over shards of chains (M adds up, n must agree)
JointTerms = namedtuple("JointTerms", "M n sum_mean sum_mean_outer sum_cov")


# ---------------------------------------------------------------------------------- arguments
def _shape(history, layout):
    """(n rows, C chains, D coordinates) of a history, from its shape alone"""
    shape = tuple(getattr(history, "shape", ()))
    if layout == "rows":
        if len(shape) == 2:
            return shape[0], 1, shape[1]
        if len(shape) == 3:
            return shape
        raise ValueError("a history is (T, D) or (T, C, D), got shape %r" % (shape,))
    if layout == "chain_major":
        if len(shape) == 3:
            return shape[0], shape[2], shape[1]
        raise ValueError("a chain-major history is (T, D, C), got shape %r" % (shape,))
    raise ValueError("layout is 'rows' or 'chain_major', got %r" % (layout,))


def _check(history, layout, max_lag, default_lag=False):
    n, c, d = _shape(history, layout)
    if n < 1 or c < 1 or not 1 <= d <= _capi.MAX_DIM:
        raise ValueError("a history needs a row, a chain and 1..%d coordinates, got %d x %d x %d" % (_capi.MAX_DIM, n, c, d))
    if max_lag is None and default_lag:
        max_lag = min(n - 1, DEFAULT_MAX_LAG)
    if max_lag != int(max_lag) or not 0 <= max_lag <= min(n - 1, MAX_LAG):
        raise ValueError("max_lag must be an integer in 0..min(n - 1, %d) = %d, got %r" % (MAX_LAG, min(n - 1, MAX_LAG), max_lag))
    return n, c, d, int(max_lag)


def _chain_major(history, layout):
    """float32 CUDA tensor [T][D][C], contiguous; a view of `history` wherever its memory already is that"""
    if isinstance(history, np.ndarray):
        history = torch.tensor(history)
    x = torch.as_tensor(history)
    dev = x.device if x.is_cuda else engine.require_device(None)
    x = x.detach().to(device=dev, dtype=torch.float32)
    if layout == "rows":
        x = x.unsqueeze(-1) if x.dim() == 2 else x.permute(0, 2, 1)
    return x.contiguous()


def _autocov(h, chain0, n_chains, max_lag, mean, acov):
    """glabc_autocov on chains [chain0, chain0 + n_chains) of the chain-major rows `h`"""
    n_rows, d, stride = h.shape
    stream = torch.cuda.current_stream(h.device).cuda_stream
    with torch.cuda.device(h.device):
        _capi.check(_capi.lib().glabc_autocov(h.data_ptr() + 4 * chain0, n_rows, d, n_chains, stride, max_lag, mean.data_ptr(),
                                              acov.data_ptr(), C.c_void_p(stream)), "glabc_autocov")


# ---------------------------------------------------------------------------------- the device part
def autocovariance(history, max_lag, layout="rows"):
    """-> (mean [D][C], acov [max_lag + 1][D][C]): float64 device tensors straight from the kernels, per chain"""
    n, c, d, max_lag = _check(history, layout, max_lag)
    h = _chain_major(history, layout)
    mean = torch.empty(d, c, dtype=torch.float64, device=h.device)
    acov = torch.empty(max_lag + 1, d, c, dtype=torch.float64, device=h.device)
    _autocov(h, 0, c, max_lag, mean, acov)
    return mean, acov


def _sums(h, max_lag):
    """sum over chains of mean, mean^2 and acov_k, k <= max_lag, of the chain-major rows `h` -> float64 host arrays.
    The chains go through the kernels in slabs, so the per-chain outputs never take more than a quarter of the history"""
    n, d, c = h.shape
    per_chain = 8 * d * (max_lag + 3)                 # mean, acov and the squared means, float64
    slab = min(_SLAB_BYTES, h.numel()) // per_chain // 64 * 64          # numel() float32 values are a quarter of their bytes
    slab = min(c, max(slab, 64))
    mean = torch.empty(d, slab, dtype=torch.float64, device=h.device)
    acov = torch.empty(max_lag + 1, d, slab, dtype=torch.float64, device=h.device)
    total = torch.zeros(max_lag + 3, d, dtype=torch.float64, device=h.device)
    for chain0 in range(0, c, slab):
        k = min(slab, c - chain0)
        m, a = (mean, acov) if k == slab else (mean.view(-1)[:d * k].view(d, k), acov.view(-1)[:(max_lag + 1) * d * k].view(-1, d, k))
        _autocov(h, chain0, k, max_lag, m, a)
        total[0] += m.sum(dim=1)
        total[1] += (m * m).sum(dim=1)
        total[2:] += a.sum(dim=2)
    total = total.cpu().numpy()
    return total[0], total[1], total[2:]


def terms(history, max_lag, first_half_rows=None, layout="rows"):
    """The additive sufficient statistics of a shard of chains (float64 host arrays, see Terms): M, n, the sums over chains of
    mean, mean^2 and acov_k [max_lag + 1][D], and the first three for each half of the rows -- rows [0, h) and [n - h, n),
    h = first_half_rows (default n // 2), which split-R-hat reads; h < 2 leaves the halves empty (half_n = 0)."""
    n, c, d, max_lag = _check(history, layout, max_lag)
    half = n // 2 if first_half_rows is None else int(first_half_rows)
    if not 0 <= half <= n:
        raise ValueError("first_half_rows must be in 0..n = %d, got %r" % (n, first_half_rows))
    h = _chain_major(history, layout)
    s_mean, s_sq, s_acov = _sums(h, max_lag)
    hm, hs, ha = np.zeros((2, d)), np.zeros((2, d)), np.zeros((2, d))
    if half >= 2:
        for i, rows in enumerate((h[:half], h[n - half:])):      # row slices of the buffer are contiguous
            hm[i], hs[i], a0 = _sums(rows, 0)
            ha[i] = a0[0]
    else:
        half = 0
    return Terms(c, n, s_mean, s_sq, s_acov, half, hm, hs, ha)


# ---------------------------------------------------------------------------------- shards
def combine(list_of_terms):
    """Terms of the concatenated shards: a plain sum"""
    parts = list(list_of_terms)
    if not parts:
        raise ValueError("combine needs at least one Terms")
    first = parts[0]
    for t in parts[1:]:
        if (t.n, t.half_n) != (first.n, first.half_n) or np.shape(t.sum_acov) != np.shape(first.sum_acov):
            raise ValueError("shards differ in rows, half rows or lags: (%d, %d, %r) and (%d, %d, %r)"
                             % (first.n, first.half_n, np.shape(first.sum_acov), t.n, t.half_n, np.shape(t.sum_acov)))
    add = lambda field: sum(np.asarray(getattr(t, field), np.float64) for t in parts)          # noqa: E731
    return Terms(sum(int(t.M) for t in parts), first.n, add("sum_mean"), add("sum_mean_sq"), add("sum_acov"), first.half_n,
                 add("half_sum_mean"), add("half_sum_mean_sq"), add("half_sum_acov0"))


def pack(t):
    """Terms as one float64 vector whose sum over shards is the packed Terms of all chains (n and half_n travel outside)"""
    return np.concatenate([[float(t.M)], np.ravel(t.sum_mean), np.ravel(t.sum_mean_sq), np.ravel(t.sum_acov),
                           np.ravel(t.half_sum_mean), np.ravel(t.half_sum_mean_sq), np.ravel(t.half_sum_acov0)])


def unpack(vector, n, half_n, dim):
    v = np.asarray(vector, np.float64)
    lags = (v.size - 1 - 8 * dim) // dim
    cut = np.cumsum([1, dim, dim, lags * dim, 2 * dim, 2 * dim])
    m, s_mean, s_sq, s_acov, hm, hs, ha = np.split(v, cut)
    return Terms(int(round(m[0])), int(n), s_mean, s_sq, s_acov.reshape(lags, dim), int(half_n), hm.reshape(2, dim),
                 hs.reshape(2, dim), ha.reshape(2, dim))


# ---------------------------------------------------------------------------------- the formulas
def _within_between(m, n, s_mean, s_sq, s_acov0):
    """(W, var+) of m chains of n draws from their sums, [D] each"""
    with np.errstate(divide="ignore", invalid="ignore"):
        w = n / (n - 1.0) * (s_acov0 / m)
        b_over_n = (s_sq - s_mean * s_mean / m) / (m - 1.0) if m > 1 else np.zeros_like(w)
        return w, (n - 1.0) / n * w + b_over_n


def _as_terms(x, max_lag, layout):
    return x if isinstance(x, Terms) else terms(x, max_lag, layout=layout)


def rhat(x, split=True, layout="rows"):
    """R-hat per coordinate, float64 [D], of a history or of its Terms; split: of the 2M half-chains"""
    if not isinstance(x, Terms):
        n = _check(x, layout, 0)[0]
        if n < (4 if split else 2):
            raise ValueError("%sR-hat needs %d rows, got %d" % (("split-", 4, n) if split else ("", 2, n)))
    t = _as_terms(x, 0, layout)
    if split:
        if t.half_n < 2:
            raise ValueError("split-R-hat needs n >= 4 rows (two halves of two), got n = %d" % t.n)
        w, var = _within_between(2 * t.M, t.half_n, t.half_sum_mean.sum(0), t.half_sum_mean_sq.sum(0), t.half_sum_acov0.sum(0))
    else:
        if t.n < 2:
            raise ValueError("R-hat needs n >= 2 rows, got n = %d" % t.n)
        w, var = _within_between(t.M, t.n, t.sum_mean, t.sum_mean_sq, t.sum_acov[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(w == 0.0, np.nan, np.sqrt(var / w))


def geyer_tau(rho):
    """Geyer's initial positive, monotone sequence on rho [K + 1] or [K + 1][D] (rho[0] = 1) -> (tau, truncated)"""
    rho = np.asarray(rho, np.float64)
    if rho.ndim == 1:
        tau, trunc = geyer_tau(rho[:, None])
        return tau[0], trunc[0]
    pairs = rho.shape[0] // 2                         # P_j needs lag 2j + 1 <= K
    if pairs < 1:
        raise ValueError("the sequence needs max_lag >= 1")
    total = rho[0] + rho[1]                           # P_0 is never cut
    prev = total.copy()
    alive = np.ones(rho.shape[1], bool)
    for j in range(1, pairs):
        p = rho[2 * j] + rho[2 * j + 1]
        alive &= ~(p < 0.0)
        p = np.minimum(p, prev)
        total = np.where(alive, total + p, total)
        prev = p
    return -1.0 + 2.0 * total, alive


def ess(x, max_lag=None, layout="rows"):
    """-> Ess(ess [D], tau [D], truncated [D] bool, max_lag) of a history or of its Terms (max_lag: the history's default is
    min(n - 1, 256); Terms bring their own)"""
    if isinstance(x, Terms):
        t = x
        lag = t.sum_acov.shape[0] - 1 if max_lag is None else int(max_lag)
        if not 1 <= lag <= t.sum_acov.shape[0] - 1:
            raise ValueError("max_lag must be in 1..%d for these Terms, got %r" % (t.sum_acov.shape[0] - 1, max_lag))
    else:
        n, _, _, lag = _check(x, layout, max_lag, default_lag=True)
        if n < 2 or lag < 1:
            raise ValueError("ESS needs n >= 2 rows and max_lag >= 1, got n = %d, max_lag = %d" % (n, lag))
        t = terms(x, lag, first_half_rows=0, layout=layout)
    n, m = float(t.n), float(t.M)
    w, var = _within_between(t.M, t.n, t.sum_mean, t.sum_mean_sq, t.sum_acov[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        rho = 1.0 - (w - n / (n - 1.0) * (t.sum_acov[:lag + 1] / m)) / var
        rho[0] = 1.0
        rho[:, w == 0.0] = np.nan
        tau, truncated = geyer_tau(rho)
        return Ess(m * n / tau, tau, truncated, lag)


def summary(history, max_lag=None, layout="rows"):
    """-> dict of mean, sd = sqrt(var+), mcse = sd / sqrt(ess), rhat (split), ess, tau, truncated: [D] each"""
    n, _, _, lag = _check(history, layout, max_lag, default_lag=True)
    if n < 4 or lag < 1:
        raise ValueError("a summary needs n >= 4 rows and max_lag >= 1, got n = %d, max_lag = %d" % (n, lag))
    t = terms(history, lag, layout=layout)
    e = ess(t)
    _, var = _within_between(t.M, t.n, t.sum_mean, t.sum_mean_sq, t.sum_acov[0])
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = np.sqrt(var)
        return {"mean": t.sum_mean / t.M, "sd": sd, "mcse": sd / np.sqrt(e.ess), "rhat": rhat(t, split=True), "ess": e.ess,
                "tau": e.tau, "truncated": e.truncated}


# ---------------------------------------------------------------------------------- quantiles: the device part
def _check_prefixes(level, prefixes, d):
    """-> uint32 [D][P] (level 0: one ignored word per coordinate)"""
    if level != int(level) or not 0 <= level <= 2:
        raise ValueError("level is 0, 1 or 2, got %r" % (level,))
    if level == 0:
        if prefixes is not None and np.shape(prefixes) != (d, 1):
            raise ValueError("level 0 has no prefixes (None, or one ignored word per coordinate), got shape %r" % (np.shape(prefixes),))
        return np.zeros((d, 1), np.uint32)
    table = np.asarray(prefixes)
    if table.ndim != 2 or table.shape[0] != d or table.shape[1] < 1 or table.dtype.kind not in "ui":
        raise ValueError("prefixes are integers [D = %d][P >= 1], got shape %r of %s" % (d, table.shape, table.dtype))
    table = table.astype(np.int64)
    used = table != UNUSED_PREFIX
    if ((table < 0) | (used & (table >> KEY_LEVELS[level][0] != 0))).any():
        raise ValueError("a level-%d prefix has %d bits (or is 0xFFFFFFFF, unused)" % (level, KEY_LEVELS[level][0]))
    for row in table:
        if len(np.unique(row[row != UNUSED_PREFIX])) != (row != UNUSED_PREFIX).sum():
            raise ValueError("the used prefixes of a coordinate must be distinct")
    return table.astype(np.uint32)


def _key_counts(h, level, table):
    """glabc_key_counts on the chain-major rows `h`, at most MAX_PREFIXES columns of `table` per launch -> uint64 [D][P][2^digit_bits]"""
    n_rows, d, stride = h.shape
    bins = 1 << KEY_LEVELS[level][1]
    out = np.zeros((d, table.shape[1], bins), np.uint64)
    stream = torch.cuda.current_stream(h.device).cuda_stream
    with torch.cuda.device(h.device):
        for p0 in range(0, table.shape[1], MAX_PREFIXES):
            part = np.ascontiguousarray(table[:, p0:p0 + MAX_PREFIXES])
            k = part.shape[1]
            counts = torch.zeros(d, k, bins, dtype=torch.int64, device=h.device)
            _capi.check(_capi.lib().glabc_key_counts(h.data_ptr(), n_rows, d, stride, stride, int(level), k, part.ctypes.data,
                                                     counts.data_ptr(), C.c_void_p(stream)), "glabc_key_counts")
            out[:, p0:p0 + k] = counts.cpu().numpy().view(np.uint64)
    return out


def key_counts(history, level, prefixes=None, layout="rows"):
    """-> uint64 [D][P][2^digit_bits]: per coordinate and prefix, how many of the history's values (all rows, all chains) belong to
    the prefix and have each digit of `level` (include/glabc.h; level 0: P = 1, every value).  A prefix of 0xFFFFFFFF is an unused
    slot, its row stays zero.  Additive over shards of chains: what a sharded job all-reduces inside the count_fn of `select`"""
    _, _, d, _ = _check(history, layout, 0)
    table = _check_prefixes(level, prefixes, d)
    return _key_counts(_chain_major(history, layout), int(level), table)


# ---------------------------------------------------------------------------------- quantiles: the host driver
def unkey(keys):
    """float32 values of uint32 keys: +0.0 for the zero's key, NaN for 0xFFFFFFFF"""
    k = np.asarray(keys, np.uint32)
    u = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return np.where(k == np.uint32(UNUSED_PREFIX), np.float32(np.nan), u.view(np.float32))


def _walk(count_fn, ranks_of):
    """The radix selection.  ranks_of(N [D], n_nan [D]) -> int64 ranks [R][D], asked once the level-0 counts are there;
    -> (float32 order statistics [R][D], N [D], n_nan [D])"""
    prefix = rem = slot = None
    for level, (prefix_bits, digit_bits) in enumerate(KEY_LEVELS):
        if level == 0:
            counts = np.asarray(count_fn(0, None)).astype(np.int64)
            if counts.ndim != 3 or counts.shape[1:] != (1, 1 << digit_bits):
                raise ValueError("count_fn(0, None) must return [D][1][%d] counts, got shape %r" % (1 << digit_bits, counts.shape))
            d = counts.shape[0]
            total, n_nan = counts[:, 0].sum(axis=1), counts[:, 0, -1].copy()          # the last level-0 digit holds the NaNs alone
            rem = np.array(ranks_of(total, n_nan), np.int64).reshape(-1, d)
            if ((rem < 0) | (rem >= total)).any():
                raise ValueError("a rank outside 0..N - 1 = %d" % (int(total.min()) - 1))
            prefix, slot = np.zeros(rem.shape, np.int64), np.zeros(rem.shape, np.int64)
        else:
            distinct = [np.unique(prefix[:, j]) for j in range(d)]                    # deduplicated per coordinate, ascending
            table = np.full((d, max(1, max(len(u) for u in distinct))), UNUSED_PREFIX, np.uint32)
            for j, u in enumerate(distinct):
                table[j, :len(u)] = u
                slot[:, j] = np.searchsorted(u, prefix[:, j])
            counts = np.asarray(count_fn(level, table)).astype(np.int64)
            if counts.shape != (d, table.shape[1], 1 << digit_bits):
                raise ValueError("count_fn(%d, prefixes) must return %r counts, got shape %r"
                                 % (level, (d, table.shape[1], 1 << digit_bits), counts.shape))
        cum = np.cumsum(counts, axis=2)
        for r in range(rem.shape[0]):
            for j in range(d):
                row = cum[j, slot[r, j]]
                digit = int(np.searchsorted(row, rem[r, j], side="right"))             # the first digit with cum > remaining rank
                if digit >= row.size:
                    raise RuntimeError("the level-%d counts of prefix %#x hold %d values, rank %d is not among them: count_fn is "
                                       "inconsistent between levels" % (level, prefix[r, j], row[-1], rem[r, j]))
                rem[r, j] -= row[digit - 1] if digit else 0
                prefix[r, j] = (prefix[r, j] << digit_bits) | digit
    return unkey(prefix.astype(np.uint32)), total, n_nan


def _check_q(q):
    q = np.atleast_1d(np.asarray(q, np.float64))
    if q.ndim != 1 or not ((q >= 0.0) & (q <= 1.0)).all():
        raise ValueError("quantiles are numbers in [0, 1], got %r" % (q,))
    return q


def _check_ranks(ranks, n=None):
    r = np.atleast_1d(np.asarray(ranks))
    if r.ndim != 1 or r.dtype.kind not in "ui" or (r.astype(np.int64) < 0).any() or (n is not None and (r.astype(np.int64) >= n).any()):
        raise ValueError("ranks are integers in 0..N - 1%s, got %r" % ("" if n is None else " = %d" % (n - 1), ranks))
    return r.astype(np.int64)


def select(count_fn, ranks=None, q=None):
    """Exact order statistics from digit counts.  count_fn(level, prefixes) -> counts [D][P][2^digit_bits] is called once per
    level (0, 1, 2; prefixes is None at level 0, else uint32 [D][P] with unused slots 0xFFFFFFFF) -- ``key_counts`` of a history,
    or the all-reduced sum of the shards' ``key_counts``.  At each level the digit d of a rank is the first with cum[d] > the
    remaining rank, the remaining rank drops by cum[d - 1] and the prefix becomes (prefix << digit_bits) | d.
    ranks: integers in 0..N - 1 -> float32 [R][D], the order statistics themselves.
    q: numbers in [0, 1] -> float64 [Q][D] by NumPy's default linear rule, h = q (N - 1), x_lo + (h - floor(h)) (x_hi - x_lo)
    with x_lo, x_hi the order statistics of ranks floor(h) and min(floor(h) + 1, N - 1); NaN where the coordinate holds a NaN."""
    if (ranks is None) == (q is None):
        raise ValueError("select takes ranks or q, one of them")
    if ranks is not None:
        r = _check_ranks(ranks)
        return _walk(count_fn, lambda total, n_nan: np.repeat(r[:, None], len(total), axis=1))[0]
    q = _check_q(q)

    def ranks_of(total, n_nan):
        h = q[:, None] * (total[None, :] - 1.0)
        lo = np.floor(h).astype(np.int64)
        return np.concatenate([lo, np.minimum(lo + 1, total[None, :] - 1)])
    x, total, n_nan = _walk(count_fn, ranks_of)
    x = x.astype(np.float64)
    h = q[:, None] * (total[None, :] - 1.0)
    with np.errstate(invalid="ignore"):
        out = x[:len(q)] + (h - np.floor(h)) * (x[len(q):] - x[:len(q)])
    out[:, n_nan > 0] = np.nan
    return out


def _counter(history, layout):
    """count_fn of a history, staged once"""
    h = _chain_major(history, layout)
    return lambda level, table: _key_counts(h, level, np.zeros((h.shape[1], 1), np.uint32) if table is None else table)


def order_statistics(history, ranks, layout="rows"):
    """-> float32 [R][D]: element ranks[r] of each coordinate's T * C draws in ascending order (NaNs last), exactly"""
    n, c, _, _ = _check(history, layout, 0)
    r = _check_ranks(ranks, n * c)
    return select(_counter(history, layout), ranks=r)


def quantile(history, q, layout="rows"):
    """-> float64 [Q][D]: numpy.quantile(draws, q) of each coordinate's T * C draws (the default linear rule, see select)"""
    _check(history, layout, 0)
    q = _check_q(q)
    return select(_counter(history, layout), q=q)


def interval(history, prob=0.95, layout="rows"):
    """-> (lower [D], upper [D]): the equal-tailed credible interval, the quantiles at (1 - prob) / 2 and (1 + prob) / 2"""
    _check(history, layout, 0)
    if not 0.0 < prob < 1.0:
        raise ValueError("prob must be in (0, 1), got %r" % (prob,))
    lower, upper = quantile(history, ((1.0 - prob) / 2.0, (1.0 + prob) / 2.0), layout)
    return lower, upper


def _check_range(range, d):
    """-> float64 [D][2] of an explicit range, (lo, hi) or [D][2]"""
    try:
        lim = np.array(np.broadcast_to(np.asarray(range, np.float64), (d, 2)))
    except (TypeError, ValueError):
        raise ValueError("range is (lo, hi) or [D = %d][2], got %r" % (d, range)) from None
    if not (np.isfinite(lim).all() and (lim[:, 0] < lim[:, 1]).all()):
        raise ValueError("range needs finite lo < hi, got %r" % (range,))
    return lim


def _exact_range(h):
    """-> float64 [D][2]: each coordinate's exact minimum and maximum (NaNs aside) of the chain-major rows `h`, by the selection;
    a constant coordinate widened by +-0.5"""
    def first_and_last(total, n_nan):
        if (total == n_nan).any():
            raise ValueError("a coordinate holds nothing but NaN: no range to bin")
        return np.stack([np.zeros_like(total), total - n_nan - 1])
    ends, _, _ = _walk(_counter(h, "chain_major"), first_and_last)
    lim = np.ascontiguousarray(ends.astype(np.float64).T)
    if not np.isfinite(lim).all():
        raise ValueError("the draws' range %r is not finite: pass range=" % (lim.tolist(),))
    lim[lim[:, 0] == lim[:, 1]] += (-0.5, 0.5)
    return lim


def histogram(history, bins=64, range=None, layout="rows"):
    """-> Histogram(counts uint64 [D][bins], edges float64 [D][bins + 1], below, above, nan uint64 [D]): `bins` equal bins per
    coordinate over `range` = (lo, hi) or [D][2], the last one closed as NumPy's; values under lo, over hi and NaNs are counted
    apart.  range=None: each coordinate's exact minimum and maximum (NaNs aside), a constant coordinate widened by +-0.5"""
    _, _, d, _ = _check(history, layout, 0)
    if isinstance(bins, bool) or bins != int(bins) or not 1 <= bins <= MAX_BINS:
        raise ValueError("bins must be an integer in 1..%d, got %r" % (MAX_BINS, bins))
    bins = int(bins)
    lim = None if range is None else _check_range(range, d)
    h = _chain_major(history, layout)
    if lim is None:
        lim = _exact_range(h)
    lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
    n_rows, _, stride = h.shape
    counts = torch.zeros(d, bins + 3, dtype=torch.int64, device=h.device)
    with torch.cuda.device(h.device):
        _capi.check(_capi.lib().glabc_histogram(h.data_ptr(), n_rows, d, stride, stride, bins, lo.ctypes.data, hi.ctypes.data,
                                                counts.data_ptr(), C.c_void_p(torch.cuda.current_stream(h.device).cuda_stream)),
                    "glabc_histogram")
    counts = counts.cpu().numpy().view(np.uint64)
    edges = np.stack([np.linspace(lo[j], hi[j], bins + 1) for j in np.arange(d)])
    return Histogram(counts[:, :bins].copy(), edges, counts[:, bins].copy(), counts[:, bins + 1].copy(), counts[:, bins + 2].copy())


# ---------------------------------------------------------------------------------- the joint posterior: the device part
def _check_pairs(pairs, d):
    """-> int32 [P][2]; None: every i < j"""
    if d < 2:
        raise ValueError("a joint histogram needs two coordinates, the history has %d" % d)
    if pairs is None:
        return np.array([(i, j) for i in np.arange(d) for j in np.arange(i + 1, d)], np.int32)
    table = np.asarray(pairs)
    if table.ndim != 2 or table.shape[1] != 2 or table.shape[0] < 1 or table.dtype.kind not in "ui":
        raise ValueError("pairs are integers [P >= 1][2], got shape %r of %s" % (table.shape, table.dtype))
    table = table.astype(np.int64)
    if ((table < 0) | (table >= d)).any() or (table[:, 0] == table[:, 1]).any():
        raise ValueError("a pair is two different coordinates in 0..%d, got %r" % (d - 1, table.tolist()))
    return np.ascontiguousarray(table.astype(np.int32))


def histogram2d(history, pairs=None, bins=64, range=None, layout="rows"):
    """-> JointHistogram(counts uint64 [P][bins][bins], pairs int [P][2], edges float64 [D][bins + 1], outside, nan uint64 [P]):
    for every pair (a, b) of coordinates (None: all i < j) the `bins` x `bins` grid of the draws (row t, chain c), axis 0 along
    coordinate a and axis 1 along b as in numpy.histogram2d(x_a, x_b), each axis binned as ``histogram`` bins it.  A draw with a NaN in either coordinate is counted in `nan`; otherwise one
    with a value under lo or over hi in either coordinate in `outside`.  (a, b) and (b, a) are each other's transposes and a pair
    may repeat; more than 28 pairs go in several ``glabc_histogram2d`` launches.  range = (lo, hi) or [D][2]; range=None: each
    coordinate's exact minimum and maximum (NaNs aside), a constant coordinate widened by +-0.5, as ``histogram``.  With an
    explicit `range` the counts are additive over shards of chains (and slices of rows): a sharded job all-reduces them.
    ``hpd_levels`` turns a grid into the levels a contour plot draws."""
    _, _, d, _ = _check(history, layout, 0)
    table = _check_pairs(pairs, d)
    if isinstance(bins, bool) or bins != int(bins) or not 1 <= bins <= MAX_JOINT_BINS:
        raise ValueError("bins must be an integer in 1..%d, got %r" % (MAX_JOINT_BINS, bins))
    bins = int(bins)
    lim = None if range is None else _check_range(range, d)
    h = _chain_major(history, layout)
    if lim is None:
        lim = _exact_range(h)
    lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
    n_rows, _, stride = h.shape
    cells = bins * bins
    out = np.zeros((table.shape[0], cells + 2), np.uint64)
    stream = torch.cuda.current_stream(h.device).cuda_stream
    with torch.cuda.device(h.device):
        for p0 in np.arange(0, table.shape[0], MAX_PAIRS):
            part = np.ascontiguousarray(table[p0:p0 + MAX_PAIRS])
            k = part.shape[0]
            counts = torch.zeros(k, cells + 2, dtype=torch.int64, device=h.device)
            _capi.check(_capi.lib().glabc_histogram2d(h.data_ptr(), n_rows, d, stride, stride, k, part.ctypes.data, bins, lo.ctypes.data,
                                                      hi.ctypes.data, counts.data_ptr(), C.c_void_p(stream)), "glabc_histogram2d")
            out[p0:p0 + k] = counts.cpu().numpy().view(np.uint64)
    edges = np.stack([np.linspace(lo[j], hi[j], bins + 1) for j in np.arange(d)])
    return JointHistogram(out[:, :cells].reshape(-1, bins, bins).copy(), table.astype(np.int64), edges, out[:, cells].copy(),
                          out[:, cells + 1].copy())


def _cross(h, chain0, n_chains, mean, cov):
    """glabc_cross_moments on chains [chain0, chain0 + n_chains) of the chain-major rows `h`"""
    n_rows, d, stride = h.shape
    stream = torch.cuda.current_stream(h.device).cuda_stream
    with torch.cuda.device(h.device):
        _capi.check(_capi.lib().glabc_cross_moments(h.data_ptr() + 4 * chain0, n_rows, d, n_chains, stride, mean.data_ptr(),
                                                    cov.data_ptr(), C.c_void_p(stream)), "glabc_cross_moments")


def cross_moments(history, layout="rows"):
    """-> (mean [D][C], cov [D (D + 1) / 2][C]): float64 device tensors straight from the kernel, per chain; cov is the biased
    (1/n) covariance of coordinates i <= j at row i * D - i (i - 1) / 2 + (j - i), its diagonal ``autocovariance``'s lag 0"""
    _, c, d, _ = _check(history, layout, 0)
    h = _chain_major(history, layout)
    mean = torch.empty(d, c, dtype=torch.float64, device=h.device)
    cov = torch.empty(d * (d + 1) // 2, c, dtype=torch.float64, device=h.device)
    _cross(h, 0, c, mean, cov)
    return mean, cov


def joint_terms(history, layout="rows"):
    """The additive sufficient statistics of the covariance of a shard of chains (float64 host arrays, see JointTerms): M, n and
    the sums over chains of mean [D], of mean mean^T [D][D] and of the per-chain biased covariance [D][D].  The chains go through
    the kernel in slabs, as in ``terms``"""
    n, c, d, _ = _check(history, layout, 0)
    h = _chain_major(history, layout)
    tri = d * (d + 1) // 2
    per_chain = 8 * (d + tri + d * d)                 # mean, cov and the outer products of the means, float64
    slab = min(_SLAB_BYTES, h.numel()) // per_chain // 64 * 64
    slab = min(c, max(slab, 64))
    mean = torch.empty(d, slab, dtype=torch.float64, device=h.device)
    cov = torch.empty(tri, slab, dtype=torch.float64, device=h.device)
    s_mean = torch.zeros(d, dtype=torch.float64, device=h.device)
    s_outer = torch.zeros(d, d, dtype=torch.float64, device=h.device)
    s_cov = torch.zeros(tri, dtype=torch.float64, device=h.device)
    for chain0 in np.arange(0, c, slab):
        k = min(slab, c - int(chain0))
        m, v = (mean, cov) if k == slab else (mean.view(-1)[:d * k].view(d, k), cov.view(-1)[:tri * k].view(tri, k))
        _cross(h, int(chain0), k, m, v)
        s_mean += m.sum(dim=1)
        s_outer += (m[:, None, :] * m[None, :, :]).sum(dim=2)
        s_cov += v.sum(dim=1)
    packed = s_cov.cpu().numpy()
    i, j = np.triu_indices(d)                          # row-major upper triangle: the packed order
    full = np.empty((d, d))
    full[i, j] = packed
    full[j, i] = packed
    return JointTerms(c, n, s_mean.cpu().numpy(), s_outer.cpu().numpy(), full)


# ---------------------------------------------------------------------------------- the joint posterior: shards and formulas
def combine_joint(list_of_terms):
    """JointTerms of the concatenated shards of chains: a plain sum (n must agree)"""
    parts = list(list_of_terms)
    if not parts:
        raise ValueError("combine_joint needs at least one JointTerms")
    first = parts[0]
    for t in parts[1:]:
        if t.n != first.n or np.shape(t.sum_cov) != np.shape(first.sum_cov):
            raise ValueError("shards differ in rows or coordinates: (%d, %r) and (%d, %r)"
                             % (first.n, np.shape(first.sum_cov), t.n, np.shape(t.sum_cov)))
    add = lambda field: sum(np.asarray(getattr(t, field), np.float64) for t in parts)          # noqa: E731
    return JointTerms(sum(int(t.M) for t in parts), first.n, add("sum_mean"), add("sum_mean_outer"), add("sum_cov"))


def covariance(x, layout="rows"):
    """-> float64 [D][D]: the covariance of all M n pooled draws of a history (or of its JointTerms) about the grand mean, with
    divisor M n - 1 -- what numpy.cov of the pooled draws estimates:
        (n sum_c cov_c + n sum_c (m_c - m)(m_c - m)^T) / (M n - 1),      sum_c (m_c - m)(m_c - m)^T = sum_mean_outer - sum_mean sum_mean^T / M
    symmetric by construction"""
    draws = x.M * x.n if isinstance(x, JointTerms) else np.prod(_check(x, layout, 0)[:2])
    if draws < 2:
        raise ValueError("a covariance needs two draws, got M n = %d" % draws)
    t = x if isinstance(x, JointTerms) else joint_terms(x, layout)
    m, n = float(t.M), float(t.n)
    s = np.asarray(t.sum_mean, np.float64)
    between = np.asarray(t.sum_mean_outer, np.float64) - np.outer(s, s) / m
    between = 0.5 * (between + between.T)
    with np.errstate(invalid="ignore", over="ignore"):
        return (n * np.asarray(t.sum_cov, np.float64) + n * between) / (m * n - 1.0)


def correlation(x, layout="rows"):
    """-> float64 [D][D]: ``covariance`` divided by the square roots of its diagonal; NaN where a variance is 0, no exception"""
    v = covariance(x, layout)
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = np.sqrt(np.diag(v))
        r = v / np.outer(sd, sd)
    r[(sd == 0.0)[:, None] | (sd == 0.0)[None, :]] = np.nan
    return r


# ---------------------------------------------------------------------------------- highest-density levels of a grid (host)
def _check_grids(counts):
    c = np.asarray(counts)
    if c.ndim < 2 or c.dtype.kind not in "ui" or (c.dtype.kind == "i" and (c < 0).any()):
        raise ValueError("counts are non-negative integers [..][bins][bins], got shape %r of %s" % (c.shape, c.dtype))
    c = c.astype(np.uint64)
    flat = c.reshape(-1, c.shape[-2] * c.shape[-1])
    if flat.shape[1] == 0 or not flat.any(axis=1).all():
        raise ValueError("an empty grid has no highest-density region")
    return c, flat


def hpd_levels(counts, probs=(0.5, 0.9, 0.95)):
    """Highest-posterior-density levels of a pair's grid [bins][bins] (or of a stack of grids [..][bins][bins]), on the host in
    integer arithmetic.  With N_in the sum of the grid and need = ceil(p N_in) (the product one float64 multiplication, so that
    0.8 of 20 draws is 16 of them; at most N_in), the level of probability p is the largest count value v with the sum of the
    counts g >= v at least need: the region {g >= v} is the smallest set of whole level sets that holds
    the fraction p of the binned draws.  -> (level uint64 [..][Q], mass uint64 [..][Q] = the sum over the region, n_bins_inside
    int64 [..][Q]).  level / (N bin area), bin area the product of the two axes' bin widths, is the density threshold a filled
    contour plot of the grid draws at p; equal bins make the region the same for counts and densities.  An empty grid raises"""
    import math
    q = np.atleast_1d(np.asarray(probs, np.float64))
    if q.ndim != 1 or q.size < 1 or not ((q > 0.0) & (q <= 1.0)).all():
        raise ValueError("probs are numbers in (0, 1], got %r" % (probs,))
    c, flat = _check_grids(counts)
    level = np.empty((flat.shape[0], q.size), np.uint64)
    mass = np.empty((flat.shape[0], q.size), np.uint64)
    inside = np.empty((flat.shape[0], q.size), np.int64)
    for g, grid in enumerate(flat):
        s = np.sort(grid)[::-1]
        cum = np.cumsum(s, dtype=np.uint64)
        total = int(cum[-1])
        for i, p in enumerate(q):
            need = min(int(math.ceil(float(p) * float(total))), total)
            v = s[int(np.searchsorted(cum, np.uint64(need), side="left"))]
            region = grid >= v
            level[g, i], mass[g, i], inside[g, i] = v, grid[region].sum(dtype=np.uint64), int(region.sum())
    lead = c.shape[:-2]
    return level.reshape(lead + (q.size,)), mass.reshape(lead + (q.size,)), inside.reshape(lead + (q.size,))


def hpd_mask(counts, prob):
    """-> bool, the shape of `counts`: counts >= the ``hpd_levels`` level of `prob`, the highest-density region of each grid"""
    if np.ndim(prob) != 0:
        raise ValueError("prob is one number in (0, 1], got %r" % (prob,))
    level = hpd_levels(counts, (prob,))[0]
    return np.asarray(counts).astype(np.uint64) >= level[..., 0][..., None, None]
