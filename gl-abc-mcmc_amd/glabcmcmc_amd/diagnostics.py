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

Out of scope: rank-normalised bulk / tail ESS, per-chain ESS (``autocovariance`` returns the per-chain numbers), and
accumulating lagged products inside the sampler kernels.
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
