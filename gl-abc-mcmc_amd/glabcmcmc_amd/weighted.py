"""weighted -- posterior summaries of weighted draws: an ``smc.Population``, the ``regression.Adjusted`` draws, a
``rejection.Rejection`` (unit weights) or any ``(theta (n, D), weights (n,) | None)`` pair.

What ``diagnostics.quantile`` / ``interval`` / ``order_statistics`` / ``histogram`` / ``histogram2d`` are to a chain history, for
draws that carry weights.  Nothing is resampled and nothing is sorted: a draw's float32 weight w is quantised to an integer
multiplicity (include/glabc.h),

    v = (double) w * scale          m = 0 if not w > 0,   2^32 - 1 if v >= 4294967295,   rint(v) (ties to even) otherwise

and every summary is that of the multiset in which draw i occurs m_i times.  ``glabc_weighted_key_counts`` /
``glabc_weighted_histogram`` / ``glabc_weighted_histogram2d`` (csrc/glabc_weighted.hip) are the counting kernels of
``diagnostics`` with a draw adding m_i where those add 1, so ``diagnostics.select`` walks their digit counts unchanged and the
grids go to ``diagnostics.hpd_levels`` / ``hpd_mask`` as they are.  The counts are sums of integers: the same bits in every launch
geometry and on both paths below, and additive over shards of draws.

``quantize`` picks the scale: by default the power of two that puts the largest weight into [2^31, 2^32) -- scaling by a power
of two moves no mantissa bit, so every weight of at least 2^-8 of the largest is represented exactly (m / scale == w) and a
smaller one to within half a unit, 2^-32 of the largest weight.  It refuses weights that the kernel's clamps would have to decide
about (NaN, infinite, negative, all zero, an explicit scale that clamps).  A sharded job passes one explicit ``scale`` on every
rank, as it passes one explicit ``range``.

``quantile`` is the inverted weighted empirical distribution function: the smallest draw whose cumulative multiplicity reaches
max(ceil(q M), 1), M = sum m_i, with q M formed in exact integer arithmetic (``fractions.Fraction``: M can exceed 2^53, where a
float64 product picks a wrong rank) -- order statistic max(ceil(q M), 1) - 1 of the multiset, what
``numpy.quantile(x, q, weights=m, method="inverted_cdf")`` returns.  No interpolation: there is no agreed linear rule for weighted
samples.  NaN where a coordinate holds a NaN of positive multiplicity; a draw of multiplicity 0 is skipped whatever it holds.

``path="auto"`` runs the kernels for CUDA tensors and the same integer arithmetic in plain torch for CPU tensors;
``path="generic"`` is the torch arithmetic wherever the tensors live, ``path="fused"`` insists on the kernels.  Both paths return
equal integers, so equal quantiles and grids.

Shards.  ``key_counts`` and, under an explicit ``range``, the histogram counts are additive over slices of draws once every shard
uses the same ``scale``: a sharded job all-reduces ``key_counts`` inside the ``count_fn`` it gives ``select``, and all-reduces the
counts of ``histogram`` / ``histogram2d``.  ``terms`` reduces a shard to the additive statistics of ``summary``'s mean, sd and
effective sample size, ``combine`` adds shards, ``moments`` evaluates them.

Posterior predictive checks of weighted draws are ``predictive.check_weighted``, on the same quantised weights.

Out of scope: weights on (T, C, D) chain histories, weighted R-hat / ESS of chains, an interpolating
weighted quantile, a kernel for the weighted mean and covariance (``regression.terms`` holds sum w, sum w theta and
sum w theta theta^T in specified bits), float64 weights in the kernels (they are cast to float32, as everywhere in the package).
"""
import ctypes as C
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np
import torch

from . import _capi
from . import diagnostics as D
from .regression import _dimension_major, _fused

MAX_MULTIPLICITY = (1 << 32) - 1          # the clamp of the quantised weight
MAX_DRAWS = 1 << 31                       # GLABC_MAX_WEIGHTED_DRAWS

# additive over shards of draws under one scale: n draws, M = sum m, sum m^2 (Python integers), sum m x and sum m x^2 (float64 [D])
Terms = namedtuple("Terms", "scale n M sum_m2 sum_mx sum_mxx")
select = D.select                          # the radix selection over digit counts, unchanged: ranks run in 0 .. M - 1


# ---------------------------------------------------------------------------------- arguments
def _draws(draws):
    """-> (theta (n, D) tensor, weights (n,) tensor or None) of a Population, an Adjusted, a Rejection or a (theta, weights) pair"""
    if hasattr(draws, "theta"):
        theta, weights = draws.theta, getattr(draws, "weights", None)
    elif isinstance(draws, (tuple, list)) and len(draws) == 2:
        theta, weights = draws
    else:
        raise ValueError("draws is an smc.Population, a regression.Adjusted, a rejection.Rejection or a (theta, weights) pair, got %r"
                         % (type(draws),))
    theta = torch.as_tensor(theta)
    if theta.dim() != 2 or not 1 <= theta.shape[1] <= _capi.MAX_DIM:
        raise ValueError("theta is (n, D) with D in 1..%d, got shape %r" % (_capi.MAX_DIM, tuple(theta.shape)))
    if theta.shape[0] > MAX_DRAWS:
        raise ValueError("at most 2^31 draws, got %d" % theta.shape[0])
    if weights is not None:
        weights = torch.as_tensor(weights).reshape(-1)
        if weights.shape[0] != theta.shape[0]:
            raise ValueError("weights holds one number per draw (%d), got %d" % (theta.shape[0], weights.shape[0]))
    return theta, weights


def _weights32(theta, weights):
    """float32, contiguous, where theta lives; None: unit weights"""
    if weights is None:
        return torch.ones(theta.shape[0], dtype=torch.float32, device=theta.device)
    return weights.detach().to(device=theta.device, dtype=torch.float32).contiguous()


def _scale(w, scale):
    """The scale the float32 weights `w` are quantised with, after the checks that keep the kernel's clamps from ever deciding a
    result"""
    if w.numel() == 0:
        raise ValueError("no draws")
    lo, hi = float(w.min()), float(w.max())                          # a NaN propagates into both
    if math.isnan(lo) or math.isnan(hi) or math.isinf(hi) or lo < 0.0:
        raise ValueError("weights must be finite and >= 0, got a minimum of %r and a maximum of %r" % (lo, hi))
    if not hi > 0.0:
        raise ValueError("no draw carries weight")
    if scale is None:
        return 2.0 ** (32 - math.frexp(hi)[1])                       # 2^(31 - floor(log2 max w)): the largest lands in [2^31, 2^32)
    if isinstance(scale, bool) or not isinstance(scale, (int, float, np.floating, np.integer)):
        raise ValueError("scale is a positive finite number, got %r" % (scale,))
    scale = float(scale)
    if not (math.isfinite(scale) and scale > 0.0):
        raise ValueError("scale is a positive finite number, got %r" % (scale,))
    if hi * scale >= float(MAX_MULTIPLICITY):
        raise ValueError("scale %r clamps the largest weight %r at 2^32 - 1" % (scale, hi))
    return scale


def _multiplicity(w, scale):
    """the rule of include/glabc.h on float32 weights -> int64"""
    v = w.double() * torch.tensor([scale], dtype=torch.float64, device=w.device)          # one rounded product
    m = torch.round(v).clamp(max=float(MAX_MULTIPLICITY))                                 # ties to even
    return torch.where(w > 0, m, torch.zeros_like(m)).to(torch.int64)


def quantize(weights, scale=None):
    """-> (m int64 tensor (n,), scale): the integer multiplicities of float32 `weights` (module docstring) and the scale that gave
    them.  scale=None: 2^(31 - floor(log2 max w)).  ValueError on a NaN, infinite or negative weight, on all-zero weights and on
    an explicit scale that would clamp the largest weight."""
    w = torch.as_tensor(weights).detach().reshape(-1).to(torch.float32)
    scale = _scale(w, scale)
    return _multiplicity(w, scale), scale


class _Prepared:
    """the draws of one call: what the kernels read in place (x, stride), the float32 weights, the scale and the path"""

    def __init__(self, draws, scale, path):
        theta, weights = _draws(draws)
        self.n, self.d = theta.shape
        self.w = _weights32(theta, weights)
        self.scale = _scale(self.w, scale)
        self.fused = _fused(path, theta, self.w)
        self.dev = theta.device
        self._m = None
        if self.fused:
            self.x, self.stride = _dimension_major(theta.detach())
        else:
            self.theta = theta.detach().to(torch.float32)

    @property
    def m(self):
        if self._m is None:
            self._m = _multiplicity(self.w, self.scale)
        return self._m

    def call(self, name, *args):
        with torch.cuda.device(self.dev):
            stream = torch.cuda.current_stream(self.dev).cuda_stream
            _capi.check(getattr(_capi.lib(), name)(self.x.data_ptr(), self.stride, self.d, self.w.data_ptr(), self.n, self.scale, *args,
                                                   C.c_void_p(stream)), name)


# ---------------------------------------------------------------------------------- the generic path: integer sums in torch
def _keys(x):
    """the order-preserving key of float32 values (include/glabc.h) -> int64 in 0 .. 2^32 - 1"""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = torch.where(x == 0, torch.zeros_like(u), u)
    k = torch.where(u >> 31 == 1, ~u & 0xFFFFFFFF, u | 0x80000000)
    return torch.where(torch.isnan(x), torch.full_like(k, D.UNUSED_PREFIX), k)


def _sum_slots(slot, m, n_slots):
    """sum of m over the draws of each slot (slot < 0: none) -> uint64 NumPy [n_slots]; int64 adds, exact"""
    keep = (slot >= 0) & (m > 0)
    out = torch.zeros(n_slots, dtype=torch.int64, device=m.device)
    out.index_add_(0, slot[keep], m[keep])
    return out.cpu().numpy().view(np.uint64)


def _axis_bins(x, bins, lo, hi):
    """glabc_histogram's bin of float32 values on [lo, hi] -> int64; -1 outside, -2 NaN (plus `below`, for the marginal slots)"""
    v = x.double()
    scale = np.float64(bins) / (np.float64(hi) - np.float64(lo))
    u = (v - float(lo)) * float(scale)                               # two rounded operations
    nan, below, above = torch.isnan(v), v < float(lo), v > float(hi)
    b = torch.floor(torch.where(nan | below | above, torch.zeros_like(u), u)).to(torch.int64).clamp(max=bins - 1)
    b = torch.where(v == float(hi), torch.full_like(b, bins - 1), b)
    b = torch.where(below | above, torch.full_like(b, -1), b)
    return torch.where(nan, torch.full_like(b, -2), b), below


# ---------------------------------------------------------------------------------- digit counts
def _key_counts(p, level, table):
    """-> uint64 [D][P][2^digit_bits] of the prepared draws, at most MAX_PREFIXES columns of `table` per launch"""
    prefix_bits, digit_bits = D.KEY_LEVELS[level]
    bins = 1 << digit_bits
    out = np.zeros((p.d, table.shape[1], bins), np.uint64)
    if p.fused:
        for p0 in range(0, table.shape[1], D.MAX_PREFIXES):
            part = np.ascontiguousarray(table[:, p0:p0 + D.MAX_PREFIXES])
            k = part.shape[1]
            counts = torch.zeros(p.d, k, bins, dtype=torch.int64, device=p.dev)
            p.call("glabc_weighted_key_counts", int(level), k, part.ctypes.data, counts.data_ptr())
            out[:, p0:p0 + k] = counts.cpu().numpy().view(np.uint64)
        return out
    for j in range(p.d):
        key = _keys(p.theta[:, j])
        digit = (key >> (32 - prefix_bits - digit_bits)) & (bins - 1)
        for s, prefix in enumerate(table[j]):
            if level == 0:
                out[j, s] = _sum_slots(digit, p.m, bins)
            elif int(prefix) != D.UNUSED_PREFIX:
                out[j, s] = _sum_slots(torch.where(key >> (32 - prefix_bits) == int(prefix), digit, torch.full_like(digit, -1)), p.m, bins)
    return out


def key_counts(draws, level, prefixes=None, scale=None, path="auto"):
    """-> uint64 [D][P][2^digit_bits]: ``diagnostics.key_counts`` with every draw counted m_i times.  Additive over shards of
    draws that share `scale`: what a sharded job all-reduces inside the count_fn of ``select``"""
    p = _Prepared(draws, scale, path)
    return _key_counts(p, int(level), D._check_prefixes(level, prefixes, p.d))


def _counter(p):
    return lambda level, table: _key_counts(p, level, np.zeros((p.d, 1), np.uint32) if table is None else table)


# ---------------------------------------------------------------------------------- order statistics and quantiles
def order_statistics(draws, ranks, scale=None, path="auto"):
    """-> float32 [R][D]: element ranks[r] of each coordinate's multiset in ascending order (NaNs last); ranks in 0 .. M - 1"""
    return select(_counter(_Prepared(draws, scale, path)), ranks=D._check_ranks(ranks))


def _rank(q, total):
    """order statistic max(ceil(q M), 1) - 1, the product in exact integer arithmetic"""
    return max(math.ceil(Fraction(float(q)) * int(total)), 1) - 1


def _quantile(count_fn, q):
    x, _, n_nan = D._walk(count_fn, lambda total, n_nan: [[_rank(v, t) for t in total] for v in q])
    out = x.astype(np.float64)
    out[:, n_nan > 0] = np.nan
    return out


def quantile(draws, q, scale=None, path="auto"):
    """-> float64 [Q][D]: the inverted weighted empirical distribution function at q (module docstring)"""
    q = D._check_q(q)
    return _quantile(_counter(_Prepared(draws, scale, path)), q)


def interval(draws, prob=0.95, scale=None, path="auto"):
    """-> (lower [D], upper [D]): the equal-tailed credible interval, the quantiles at (1 - prob) / 2 and (1 + prob) / 2"""
    if not 0.0 < prob < 1.0:
        raise ValueError("prob must be in (0, 1), got %r" % (prob,))
    lower, upper = quantile(draws, ((1.0 - prob) / 2.0, (1.0 + prob) / 2.0), scale, path)
    return lower, upper


# ---------------------------------------------------------------------------------- histograms
def _exact_range(p):
    """-> float64 [D][2]: each coordinate's exact minimum and maximum over the draws of positive multiplicity (NaNs aside), by the
    selection; a constant coordinate widened by +-0.5 -- ``diagnostics.histogram``'s default range"""
    def first_and_last(total, n_nan):
        if (total == n_nan).any():
            raise ValueError("a coordinate holds nothing but NaN: no range to bin")
        return np.stack([np.zeros_like(total), total - n_nan - 1])
    ends, _, _ = D._walk(_counter(p), first_and_last)
    lim = np.ascontiguousarray(ends.astype(np.float64).T)
    if not np.isfinite(lim).all():
        raise ValueError("the draws' range %r is not finite: pass range=" % (lim.tolist(),))
    lim[lim[:, 0] == lim[:, 1]] += (-0.5, 0.5)
    return lim


def _bins(bins, most):
    if isinstance(bins, bool) or bins != int(bins) or not 1 <= bins <= most:
        raise ValueError("bins must be an integer in 1..%d, got %r" % (most, bins))
    return int(bins)


def _limits(p, range):
    lim = _exact_range(p) if range is None else D._check_range(range, p.d)
    return np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])


def histogram(draws, bins=64, range=None, scale=None, path="auto"):
    """-> ``diagnostics.Histogram``(counts uint64 [D][bins], edges, below, above, nan): ``diagnostics.histogram`` with every draw
    counted m_i times.  range=None: the exact minimum and maximum over the draws of positive multiplicity.  With an explicit
    `range` and `scale` the counts are additive over shards of draws"""
    bins = _bins(bins, D.MAX_BINS)
    p = _Prepared(draws, scale, path)
    lo, hi = _limits(p, range)
    if p.fused:
        counts = torch.zeros(p.d, bins + 3, dtype=torch.int64, device=p.dev)
        p.call("glabc_weighted_histogram", bins, lo.ctypes.data, hi.ctypes.data, counts.data_ptr())
        counts = counts.cpu().numpy().view(np.uint64)
    else:
        counts = np.zeros((p.d, bins + 3), np.uint64)
        for j in np.arange(p.d):                                     # `range` is the argument here
            b, below = _axis_bins(p.theta[:, j], bins, lo[j], hi[j])
            slot = torch.where(b == -2, torch.full_like(b, bins + 2), torch.where(b == -1, torch.where(below, bins, bins + 1), b))
            counts[j] = _sum_slots(slot, p.m, bins + 3)
    edges = np.stack([np.linspace(lo[j], hi[j], bins + 1) for j in np.arange(p.d)])
    return D.Histogram(counts[:, :bins].copy(), edges, counts[:, bins].copy(), counts[:, bins + 1].copy(), counts[:, bins + 2].copy())


def histogram2d(draws, pairs=None, bins=64, range=None, scale=None, path="auto"):
    """-> ``diagnostics.JointHistogram``(counts uint64 [P][bins][bins], pairs, edges, outside, nan): ``diagnostics.histogram2d``
    with every draw counted m_i times.  The grids go to ``diagnostics.hpd_levels`` / ``hpd_mask`` as they are: the levels a contour
    plot of the weighted posterior draws"""
    bins = _bins(bins, D.MAX_JOINT_BINS)
    p = _Prepared(draws, scale, path)
    table = D._check_pairs(pairs, p.d)
    lo, hi = _limits(p, range)
    cells = bins * bins
    out = np.zeros((table.shape[0], cells + 2), np.uint64)
    if p.fused:
        for p0 in np.arange(0, table.shape[0], D.MAX_PAIRS):
            part = np.ascontiguousarray(table[p0:p0 + D.MAX_PAIRS])
            k = part.shape[0]
            counts = torch.zeros(k, cells + 2, dtype=torch.int64, device=p.dev)
            p.call("glabc_weighted_histogram2d", k, part.ctypes.data, bins, lo.ctypes.data, hi.ctypes.data, counts.data_ptr())
            out[p0:p0 + k] = counts.cpu().numpy().view(np.uint64)
    else:
        axis = {j: _axis_bins(p.theta[:, j], bins, lo[j], hi[j])[0] for j in sorted(set(table.reshape(-1).tolist()))}
        for i, (a, b) in enumerate(table.tolist()):
            least = torch.minimum(axis[a], axis[b])
            slot = torch.where(least >= 0, axis[a] * bins + axis[b], torch.where(least == -2, cells + 1, cells))
            out[i] = _sum_slots(slot, p.m, cells + 2)
    edges = np.stack([np.linspace(lo[j], hi[j], bins + 1) for j in np.arange(p.d)])
    return D.JointHistogram(out[:, :cells].reshape(-1, bins, bins).copy(), table.astype(np.int64), edges, out[:, cells].copy(),
                            out[:, cells + 1].copy())


# ---------------------------------------------------------------------------------- moments and the summary
def _int_sum(t):
    return int(t.sum().item())


def _terms(theta, m, scale):
    hi, lo = m >> 16, m & 0xFFFF                                     # m^2 = 2^32 hi^2 + 2^17 hi lo + lo^2: no int64 sum overflows
    sum_m2 = (_int_sum(hi * hi) << 32) + (_int_sum(hi * lo) << 17) + _int_sum(lo * lo)
    keep = m > 0                                                     # a draw of multiplicity 0 is skipped, whatever it holds
    x, md = theta[keep].double(), m[keep].double()[:, None]
    return Terms(scale, int(theta.shape[0]), _int_sum(m), sum_m2, (md * x).sum(dim=0).cpu().numpy(), (md * x * x).sum(dim=0).cpu().numpy())


def terms(draws, scale):
    """The additive statistics of a shard of draws under an explicit `scale` (every shard's) -> Terms(scale, n, M, sum_m2, sum_mx
    [D], sum_mxx [D]): M and sum m^2 are Python integers from int64 sums that cannot overflow; sum m x and sum m x^2 are torch
    float64 reductions where the draws live, their bits torch's and unspecified.  There is no kernel here"""
    if scale is None:
        raise ValueError("terms needs the explicit scale every shard uses")
    theta, weights = _draws(draws)
    w = _weights32(theta, weights)
    scale = _scale(w, scale)
    return _terms(theta.detach().to(torch.float32), _multiplicity(w, scale), scale)


def combine(list_of_terms):
    """Terms of the union of shards: integer sums, and float64 sums in list order"""
    parts = list(list_of_terms)
    if not parts or any(t.scale != parts[0].scale or np.shape(t.sum_mx) != np.shape(parts[0].sum_mx) for t in parts):
        raise ValueError("combine takes a non-empty list of Terms of one scale and dimension")
    add = lambda field: sum(np.asarray(getattr(t, field), np.float64) for t in parts)          # noqa: E731
    return Terms(parts[0].scale, sum(t.n for t in parts), sum(t.M for t in parts), sum(t.sum_m2 for t in parts), add("sum_mx"), add("sum_mxx"))


def moments(t):
    """-> (mean [D], sd [D], ess): sum m x / M, sqrt(sum m x^2 / M - mean^2) and Kish's effective sample size M^2 / sum m^2"""
    if t.M <= 0:
        raise ValueError("no draw carries weight")
    mean = np.asarray(t.sum_mx, np.float64) / float(t.M)
    with np.errstate(invalid="ignore"):
        sd = np.sqrt(np.maximum(np.asarray(t.sum_mxx, np.float64) / float(t.M) - mean * mean, 0.0))
    return mean, sd, float(Fraction(t.M * t.M, t.sum_m2))


def summary(draws, probs=(0.025, 0.5, 0.975), scale=None, path="auto"):
    """-> dict of mean [D], sd [D], quantiles [Q][D] (``quantile`` at `probs`), probs, M, scale and ess (Kish's M^2 / sum m_i^2).
    The quantiles are exact and the same on both paths; mean and sd are torch float64 reductions of m_i x_i / M, not a kernel:
    their bits are torch's and unspecified"""
    q = D._check_q(probs)
    p = _Prepared(draws, scale, path)
    t = _terms(_draws(draws)[0].detach().to(torch.float32), p.m, p.scale)
    mean, sd, ess = moments(t)
    return {"mean": mean, "sd": sd, "quantiles": _quantile(_counter(p), q), "probs": q, "M": t.M, "scale": p.scale, "ess": ess}
