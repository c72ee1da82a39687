"""predictive -- posterior predictive checks: does the fitted model reproduce the observed data?

The ``y`` a chain carries was accepted because it lay near ``y_obs``, so it is biased towards the data by construction and says
nothing about the fit.  A posterior predictive check simulates afresh, ``y_rep ~ p(y | theta)`` for every draw theta of a history,
and looks at three things: the distribution of ``y_rep`` per coordinate against ``y_obs``, the distribution of the fresh distances
``d(y_rep, y_obs)`` against epsilon, and the tail probabilities ``P(y_rep_j >= y_obs_j)`` -- the posterior predictive p-values.

Fused path.  ``glabc_predictive_counts`` (include/glabc.h, csrc/glabc_predictive.hip) reads the history once, in place, makes every
draw in registers and writes a few kilobytes of integers: K = y_dim + 1 histograms (the coordinates of ``y_rep``, then the distance)
by ``diagnostics.histogram``'s bin arithmetic, K rows of tail counts (below, equal, above, NaN) against K thresholds, and the exact
minimum and maximum of every statistic.  ``glabc_predictive_draws`` materialises ``y_rep`` and the distances instead (``simulate``).
A predictive draw is a pure function of (Model, theta, seed, 64-bit id) with ``id = (row0 + t) * n_chains_total + chain0 + c``, so
the tables are the same bits in every launch geometry and additive over shards of chains and slices of rows: a sharded job passes
``chain0`` / ``n_chains_total`` (and ``row0``), all-reduces the integer tables of ``terms`` and every rank reads ``summary`` of the
very draws the whole job would have made.  There is no CPU implementation of this path.

A ``CompiledModel`` takes the same path through a kernel of its own: ``CompiledModel.predictive_program()`` compiles
``predictive_kernel`` around the user's simulator (``glabc_rtc_compile_predictive``; the user's distance where the source announces
``GLABC_USER_DISCREPANCY``), checks it bit for bit against the composition of entry points that specifies a draw, and
``glabc_rtc_predictive_counts`` / ``glabc_rtc_predictive_draws`` launch it: ``path="fused"`` on any CUDA history, ``path="auto"``
when the history is a CUDA tensor.  So ``check(CompiledModel, cuda_history)`` under ``"auto"`` draws the same law from the Philox
streams, not from torch's generator as it did when this route was the generic one: it is a function of (Model, theta, seed, id),
and ``terms`` / ``combine`` with ``chain0``, ``n_chains_total`` and ``row0`` are exact for user Models too.  Under ``"auto"`` a source
that does not compile or a program that fails its self-check warns (``RuntimeWarning``) and runs the generic path; under
``"fused"`` it raises.

Generic path (``path="generic"``, and every Model the kernels do not take: callback Models, CPU tensors).
Plain torch: ``Model.generate_samples(theta, 1)`` in chunks of rows, ``Model.discrepancy`` where the Model has one (otherwise there
are y_dim statistics and the distance fields are ``None``), and the same bin arithmetic in float64 torch.  The noise comes from
torch's generator, seeded with ``seed`` inside ``torch.random.fork_rng`` (``seed=None``: the global generator as it stands); ids do
not apply.

``range=None`` takes two passes on the fused path -- extremes and tails, then the counts over the exact minimum and maximum, a
constant statistic widened by +-0.5 as ``diagnostics.histogram`` widens it -- and an explicit ``(K, 2)`` range one.

Weighted draws (``check_weighted``, ``terms_weighted``, ``combine_weighted``).  An ``smc.Population``, the ``regression.Adjusted``
draws, a ``rejection.Rejection`` or a ``(theta (n, D), weights (n,) | None)`` pair -- what ``weighted._draws`` takes -- is checked
without resampling: a draw's float32 weight is quantised to the integer multiplicity m_i of ``weighted.quantize`` (its refusals of
bad weights are that function's, word for word), and every table is that of the multiset in which draw i occurs m_i times, so a
count or a tail adds m_i where ``check`` adds 1, the extremes run over the draws with m_i > 0, and ``Check.n`` is M = sum m_i.  A
draw of multiplicity 0 is skipped whatever theta holds.  ``glabc_weighted_predictive_counts`` (csrc/glabc_weighted_predictive.hip;
``CompiledModel.weighted_predictive_program()`` and ``glabc_rtc_weighted_predictive_counts`` for a CompiledModel) is the fused
route: draw i has the id ``draw0 + i`` and is, bit for bit, the draw ``simulate(Model, theta, seed=seed, row0=draw0)`` makes for row
i -- which is the way to materialise ``y_rep`` for weighted draws; there is no weighted draws entry point.  A sharded job passes
one explicit ``range`` and one explicit ``scale`` on every rank and ``draw0``, the index of the shard's first draw in the whole set,
and ``combine_weighted`` adds the integer tables of the very draws the one-shot call counts.  ``bins`` is at most 512 on both routes
(GLABC_MAX_WEIGHTED_PREDICTIVE_BINS: the 64-bit counters of the kernel's table).  The generic route (callback Models, CPU tensors,
``path="generic"``) is ``_generic_stats`` on the (n, D) theta and integer sums of m in torch; its noise is torch's generator's, so
ids and ``draw0`` do not apply there and a sharded generic job does not reproduce the one-shot draws.

Out of scope: test quantities other than the coordinates and the distance, joint summaries of ``y_rep``, weights on (T, C, D)
chain histories, a materialising weighted entry point, interpolated p-values.
"""
import ctypes as C
import warnings
from collections import namedtuple
from fractions import Fraction

import numpy as np
import torch

from . import _capi, diagnostics, engine

PREDICTIVE_KEY = 0xA0761D6478BD642F          # include/glabc.h GLABC_PREDICTIVE_KEY
MAX_BINS = 1024                              # GLABC_MAX_PREDICTIVE_BINS
MAX_WEIGHTED_BINS = 512                      # GLABC_MAX_WEIGHTED_PREDICTIVE_BINS
GENERIC_CHUNK = 1 << 20                      # draws per generate_samples call of the generic path
KEY_NONE = (0xFFFFFFFF, 0)                   # what a pair of extremes holds before any value that is no NaN

# the raw integer tables, additive over shards: counts uint64 [K][bins + 3] (bins, below, above, NaN), tails uint64 [K][4] (below,
# equal, above, NaN against thresholds [K]), lim float64 [K][2]; has_distance: the last statistic is the distance
Terms = namedtuple("Terms", "n counts tails lim thresholds has_distance")
# Terms of weighted draws: n is M = sum m (a Python integer), counts and tails are sums of m; scale the quantisation's, n_draws the draws
WeightedTerms = namedtuple("WeightedTerms", "n counts tails lim thresholds has_distance scale n_draws")
Check = namedtuple("Check", "y_counts y_edges y_outside distance_counts distance_edges distance_outside tails p_upper within_epsilon n")


# ---------------------------------------------------------------------------------- arguments
def _count(name, value, least):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < least:
        raise ValueError("%s must be an integer >= %d, got %r" % (name, least, value))
    return int(value)


def _seed(seed):
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, (int, np.integer))):
        raise ValueError("seed must be an integer or None, got %r" % (seed,))
    return seed


def _bins(bins):
    if isinstance(bins, bool) or bins != int(bins) or not 1 <= bins <= MAX_BINS:
        raise ValueError("bins must be an integer in 1..%d, got %r" % (MAX_BINS, bins))
    return int(bins)


def _ids(c, chain0, n_chains_total, row0):
    """-> (id0, id_step) of a shard that holds chains chain0 .. chain0 + c - 1 of n_chains_total, rows from row0"""
    chain0, row0 = _count("chain0", chain0, 0), _count("row0", row0, 0)
    total = chain0 + c if n_chains_total is None else _count("n_chains_total", n_chains_total, 1)
    if chain0 + c > total:
        raise ValueError("chains %d..%d do not lie in n_chains_total = %d" % (chain0, chain0 + c - 1, total))
    return row0 * total + chain0, total


def _history(Model, history, layout):
    n, c, d, _ = diagnostics._check(history, layout, 0)
    if d != int(Model.theta_dim):
        raise ValueError("the history has %d coordinates, the Model's theta_dim is %d" % (d, int(Model.theta_dim)))
    return n, c, d


def _thresholds(Model, thresholds, k, has_distance):
    """-> float32 [K]; None: y_obs for the coordinates and Model.epsilon for the distance"""
    if thresholds is None:
        thr = [float(v) for v in torch.as_tensor(Model.y_obs).reshape(-1)]
        if has_distance:
            thr.append(float(Model.epsilon))
    else:
        thr = thresholds
    try:
        thr = np.array(np.broadcast_to(np.asarray(thr, np.float32), (k,)))
    except (TypeError, ValueError):
        raise ValueError("thresholds are K = %d numbers, got %r" % (k, thresholds)) from None
    if thr.shape != (k,) or np.isnan(thr).any():
        raise ValueError("thresholds are K = %d numbers, none a NaN, got %r" % (k, thresholds))
    return np.ascontiguousarray(thr)


def accepted(Model):
    """The glabc_model of `Model` if ``glabc_predictive_counts`` takes it, else None.  The entry point itself is asked, with no
    chains: a refused call launches nothing, so this needs no GPU"""
    if not callable(getattr(Model, "descriptor", None)):
        return None
    try:
        desc = Model.descriptor()
    except (NotImplementedError, ValueError):
        return None
    if not isinstance(desc, _capi.Model):
        return None
    rc = _capi.lib().glabc_predictive_draws(C.byref(desc), C.c_void_p(8), 1, desc.theta_dim, 0, 0, 0, 0, 0, C.c_void_p(8), 0, None, 0, None)
    return desc if rc == _capi.OK else None


class Fused(namedtuple("Fused", "desc program")):
    """What the fused path launches: the glabc_model, and the handle of the run-time compiled predictive program of a CompiledModel
    (None: the built-in entry points)"""

    def draws(self, *args):
        if self.program is None:
            _capi.check(_capi.lib().glabc_predictive_draws(C.byref(self.desc), *args), "glabc_predictive_draws")
        else:
            _capi.check(_capi.lib().glabc_rtc_predictive_draws(self.program, C.byref(self.desc), *args), "glabc_rtc_predictive_draws")

    def counts(self, *args):
        if self.program is None:
            _capi.check(_capi.lib().glabc_predictive_counts(C.byref(self.desc), *args), "glabc_predictive_counts")
        else:
            _capi.check(_capi.lib().glabc_rtc_predictive_counts(self.program, C.byref(self.desc), *args), "glabc_rtc_predictive_counts")


def _path(Model, history, path):
    """The one place that decides what a call runs -> the Fused of the fused path, or None for the generic one"""
    from .compiled import CompiledModel, SimulatorCompileError, SimulatorSelfCheckError
    if path not in ("auto", "fused", "generic"):
        raise ValueError('path is "auto", "fused" or "generic", got %r' % (path,))
    if path == "generic":
        return None
    on_gpu = isinstance(history, torch.Tensor) and history.is_cuda
    if isinstance(Model, CompiledModel):
        # the program needs a device to be loaded on: "auto" asks for it only where the history lives on one
        if path == "auto" and not (on_gpu and torch.cuda.is_available()):
            return None
        if path == "fused" and not on_gpu:
            raise ValueError('path="fused" on a CompiledModel needs a history on the GPU: its predictive program is launched in place')
        try:
            return Fused(Model.descriptor(), Model.predictive_program())
        except (SimulatorCompileError, SimulatorSelfCheckError) as exc:
            if path == "fused":
                raise
            warnings.warn("the predictive program of this CompiledModel is not available (%s): running the generic path"
                          % (str(exc).splitlines()[0],), RuntimeWarning, stacklevel=3)
            return None
    desc = accepted(Model)
    if path == "fused":
        if desc is None:
            raise ValueError('path="fused" needs a Model whose descriptor() glabc_predictive_counts accepts (|theta| + noise or '
                             "g-and-k) or a CompiledModel, got %r" % (type(Model).__name__,))
        return Fused(desc, None)
    return Fused(desc, None) if desc is not None and on_gpu else None


# ---------------------------------------------------------------------------------- the fused path
def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _fused_counts(fused, h, seed, id0, id_step, bins, lim, thr, want):
    """one glabc_predictive_counts / glabc_rtc_predictive_counts call on the chain-major rows `h` -> (counts [K][bins + 3], tails [K][4],
    extremes [K][2]) as NumPy arrays, None for what `want` leaves out"""
    n_rows, d, stride = h.shape
    k = fused.desc.y_dim + 1
    dev = h.device
    counts = torch.zeros(k, bins + 3, dtype=torch.int64, device=dev) if "counts" in want else None
    tails = torch.zeros(k, 4, dtype=torch.int64, device=dev) if "tails" in want else None
    extremes = torch.from_numpy(np.array([KEY_NONE] * k, np.uint32).view(np.int32)).to(dev) if "extremes" in want else None
    lo = hi = None
    if counts is not None:
        lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
    ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    with torch.cuda.device(dev):
        fused.counts(h.data_ptr(), n_rows, d, stride, stride, seed, id0, id_step, bins, None if lo is None else lo.ctypes.data,
                     None if hi is None else hi.ctypes.data, thr.ctypes.data if tails is not None else None, ptr(counts), ptr(tails),
                     ptr(extremes), _stream(dev))
    to_u64 = lambda t: None if t is None else t.cpu().numpy().view(np.uint64)          # noqa: E731
    return to_u64(counts), to_u64(tails), None if extremes is None else extremes.cpu().numpy().view(np.uint32)


def _exact_range(extremes):
    """-> float64 [K][2] from the keys of the minimum and maximum; a constant statistic widened by +-0.5, as diagnostics.histogram"""
    if (extremes[:, 0] == KEY_NONE[0]).any():
        raise ValueError("a statistic holds nothing but NaN: no range to bin, pass range=")
    lim = diagnostics.unkey(extremes).astype(np.float64)
    if not np.isfinite(lim).all():
        raise ValueError("the statistics' range %r is not finite: pass range=" % (lim.tolist(),))
    lim[lim[:, 0] == lim[:, 1]] += (-0.5, 0.5)
    return lim


# ---------------------------------------------------------------------------------- the generic path
def _generic_stats(Model, history, layout, seed):
    """-> (stats float32 [N][K] on the history's device, has_distance): y_rep of every draw, then its distance"""
    x = torch.as_tensor(history).detach().to(torch.float32)
    if layout == "chain_major":
        x = x.permute(0, 2, 1)
    theta = x.reshape(-1, x.shape[-1])
    has_distance = callable(getattr(Model, "discrepancy", None))
    devices = [theta.device] if theta.is_cuda else []
    out = []
    with torch.random.fork_rng(devices=devices, enabled=seed is not None):
        if seed is not None:
            torch.manual_seed(int(seed) & 0x7FFFFFFFFFFFFFFF)
        for first in range(0, theta.shape[0], GENERIC_CHUNK):
            part = theta[first:first + GENERIC_CHUNK]
            y = Model.generate_samples(part, 1).reshape(part.shape[0], -1).to(torch.float32)
            cols = [y]
            if has_distance:
                cols.append(Model.discrepancy(y).reshape(-1, 1).to(device=y.device, dtype=torch.float32))
            out.append(torch.cat(cols, dim=1))
    return torch.cat(out), has_distance


def _torch_slots(v, lo, hi, bins):
    """diagnostics.histogram's bin arithmetic on a float32 vector, float64 torch, every operation rounded once -> the slot of every
    value among the bins + 3, int64"""
    x = v.to(torch.float64)
    scale = float(np.float64(bins) / (np.float64(hi) - np.float64(lo)))
    nan, below, above, top = torch.isnan(x), x < lo, x > hi, x == hi
    inside = ~(nan | below | above | top)
    u = (torch.where(inside, x, torch.full_like(x, lo)) - lo) * scale
    slot = torch.clamp(torch.floor(u).to(torch.int64), max=bins - 1)
    slot = torch.where(top, torch.full_like(slot, bins - 1), slot)
    slot = torch.where(above, torch.full_like(slot, bins + 1), slot)
    slot = torch.where(below, torch.full_like(slot, bins), slot)
    return torch.where(nan, torch.full_like(slot, bins + 2), slot)


def _torch_counts(v, lo, hi, bins):
    """-> int64 [bins + 3]: the values of each slot"""
    return torch.bincount(_torch_slots(v, lo, hi, bins), minlength=bins + 3)


def _torch_tables(stats, bins, lim, thr):
    """-> (counts uint64 [K][bins + 3], tails uint64 [K][4]) of stats [N][K]"""
    k = stats.shape[1]
    counts, tails = np.zeros((k, bins + 3), np.uint64), np.zeros((k, 4), np.uint64)
    for j in range(k):
        v = stats[:, j]
        counts[j] = _torch_counts(v, float(lim[j, 0]), float(lim[j, 1]), bins).cpu().numpy().astype(np.uint64)
        t = torch.tensor(float(thr[j]), dtype=torch.float32, device=v.device)
        tails[j] = [int((v < t).sum()), int((v == t).sum()), int((v > t).sum()), int(torch.isnan(v).sum())]
    return counts, tails


def _torch_range(stats):
    lim = np.empty((stats.shape[1], 2))
    for j in range(stats.shape[1]):
        v = stats[:, j]
        v = v[~torch.isnan(v)]
        if v.numel() == 0:
            raise ValueError("a statistic holds nothing but NaN: no range to bin, pass range=")
        lim[j] = float(v.min()), float(v.max())
    if not np.isfinite(lim).all():
        raise ValueError("the statistics' range %r is not finite: pass range=" % (lim.tolist(),))
    lim[lim[:, 0] == lim[:, 1]] += (-0.5, 0.5)
    return lim


# ---------------------------------------------------------------------------------- the public surface
def simulate(Model, history, *, seed, layout="rows", chain0=0, n_chains_total=None, row0=0):
    """``glabc_predictive_draws`` (a CompiledModel: ``glabc_rtc_predictive_draws``) -> (y_rep, distance): float32 device tensors in the history's layout -- y_rep (T, C, y_dim) and
    distance (T, C) for a (T, C, D) history, (T, y_dim) and (T,) for (T, D), (T, y_dim, C) and (T, C) for layout="chain_major".
    Draw (t, c) has the id (row0 + t) * n_chains_total + chain0 + c and depends on (Model, theta, seed, id) only."""
    n, c, d = _history(Model, history, layout)
    _seed(seed)
    id0, id_step = _ids(c, chain0, n_chains_total, row0)
    fused = _path(Model, history, "fused")
    h = diagnostics._chain_major(history, layout)
    y = torch.empty(n, fused.desc.y_dim, c, dtype=torch.float32, device=h.device)
    dis = torch.empty(n, c, dtype=torch.float32, device=h.device)
    with torch.cuda.device(h.device):
        fused.draws(h.data_ptr(), n, d, c, c, engine.draw_seed(seed), id0, id_step, y.data_ptr(), c, dis.data_ptr(), c, _stream(h.device))
    if layout == "chain_major":
        return y, dis
    if len(tuple(history.shape)) == 2:
        return y[:, :, 0], dis[:, 0]
    return y.permute(0, 2, 1), dis


def _tables(Model, history, bins, range, thresholds, seed, layout, chain0, n_chains_total, row0, path):
    n, c, d = _history(Model, history, layout)
    bins = _bins(bins)
    _seed(seed)
    id0, id_step = _ids(c, chain0, n_chains_total, row0)
    fused = _path(Model, history, path)
    if fused is not None:
        k = fused.desc.y_dim + 1
        thr = _thresholds(Model, thresholds, k, True)
        lim = None if range is None else diagnostics._check_range(range, k)
        h = diagnostics._chain_major(history, layout)
        key = engine.draw_seed(seed)
        if lim is None:
            _, tails, extremes = _fused_counts(fused, h, key, id0, id_step, bins, None, thr, ("tails", "extremes"))
            lim = _exact_range(extremes)
            counts, _, _ = _fused_counts(fused, h, key, id0, id_step, bins, lim, thr, ("counts",))
        else:
            counts, tails, _ = _fused_counts(fused, h, key, id0, id_step, bins, lim, thr, ("counts", "tails"))
        return Terms(n * c, counts, tails, lim, thr, True)
    stats, has_distance = _generic_stats(Model, history, layout, seed)
    k = stats.shape[1]
    thr = _thresholds(Model, thresholds, k, has_distance)
    lim = _torch_range(stats) if range is None else diagnostics._check_range(range, k)
    counts, tails = _torch_tables(stats, bins, lim, thr)
    return Terms(n * c, counts, tails, lim, thr, has_distance)


def terms(Model, history, *, bins=64, range, thresholds=None, seed, layout="rows", chain0=0, n_chains_total=None, row0=0, path="auto"):
    """The raw integer tables of a shard of chains (see Terms) under an explicit `range` (K, 2): additive, so a sharded job whose
    ranks pass their ``chain0`` and the job's ``n_chains_total`` all-reduces ``counts`` and ``tails`` (or ``combine``s the gathered
    Terms) and counts the very draws of the whole job."""
    if range is None:
        raise ValueError("terms needs an explicit range (K, 2): shards must bin over the same edges")
    return _tables(Model, history, bins, range, thresholds, seed, layout, chain0, n_chains_total, row0, path)


def combine(list_of_terms):
    """Terms of the concatenated shards: a plain sum of the integer tables (ranges, bins and thresholds must agree)"""
    parts = list(list_of_terms)
    if not parts:
        raise ValueError("combine needs at least one Terms")
    first = parts[0]
    for t in parts[1:]:
        if (np.shape(t.counts) != np.shape(first.counts) or not np.array_equal(t.lim, first.lim) or
                not np.array_equal(t.thresholds, first.thresholds) or t.has_distance != first.has_distance):
            raise ValueError("shards differ in bins, range, thresholds or statistics")
    add = lambda field: sum(np.asarray(getattr(t, field)).astype(np.uint64) for t in parts)          # noqa: E731
    return Terms(sum(int(t.n) for t in parts), add("counts"), add("tails"), first.lim, first.thresholds, first.has_distance)


def summary(t):
    """Terms -> Check(y_counts uint64 (y_dim, bins), y_edges float64 (y_dim, bins + 1), y_outside uint64 (y_dim, 3) = below, above,
    NaN; distance_counts (bins,), distance_edges (bins + 1,), distance_outside (3,); tails uint64 (K, 4) = below, equal, above, NaN
    against the thresholds; p_upper float64 (y_dim,) = (above + equal) / (N - NaN), the posterior predictive p-values;
    within_epsilon = (below + equal) / (N - NaN) of the distance; n = N).  The distance fields are None without a distance."""
    counts, tails = np.asarray(t.counts).astype(np.uint64), np.asarray(t.tails).astype(np.uint64)
    k, bins = counts.shape[0], counts.shape[1] - 3
    yd = k - 1 if t.has_distance else k
    edges = np.stack([np.linspace(t.lim[j, 0], t.lim[j, 1], bins + 1) for j in np.arange(k)])
    # ratios of exact integers, rounded once: N (the M of weighted draws) may be past 2^53
    rest = [int(t.n) - int(tails[j, 3]) for j in range(k)]
    ratio = lambda num, den: float(Fraction(num, den)) if den else float("nan")          # noqa: E731
    p_upper = np.array([ratio(int(tails[j, 2]) + int(tails[j, 1]), rest[j]) for j in range(yd)], np.float64)
    within = ratio(int(tails[yd, 0]) + int(tails[yd, 1]), rest[yd]) if t.has_distance else None
    return Check(counts[:yd, :bins].copy(), edges[:yd], counts[:yd, bins:].copy(),
                 counts[yd, :bins].copy() if t.has_distance else None, edges[yd] if t.has_distance else None,
                 counts[yd, bins:].copy() if t.has_distance else None, tails, p_upper, within, int(t.n))


def check(Model, history, *, bins=64, range=None, thresholds=None, seed, layout="rows", chain0=0, n_chains_total=None, row0=0,
          path="auto"):
    """The posterior predictive check of a history -> Check (see ``summary``).  thresholds: K numbers, default ``y_obs`` for the
    coordinates and ``Model.epsilon`` for the distance.  range: (lo, hi) or (K, 2) -- one pass; None -- the exact minimum and
    maximum of every statistic, found in a pass of its own.  path: "auto" (the kernel for descriptor Models and CompiledModels
    and a history on the GPU, else generic), "fused", "generic"."""
    return summary(_tables(Model, history, bins, range, thresholds, seed, layout, chain0, n_chains_total, row0, path))


# ---------------------------------------------------------------------------------- weighted draws
class FusedWeighted(namedtuple("FusedWeighted", "desc program")):
    """What the fused path of the weighted checks launches: the glabc_model, and the handle of the run-time compiled weighted predictive
    program of a CompiledModel (None: the built-in entry point)"""

    def counts(self, *args):
        if self.program is None:
            _capi.check(_capi.lib().glabc_weighted_predictive_counts(C.byref(self.desc), *args), "glabc_weighted_predictive_counts")
        else:
            _capi.check(_capi.lib().glabc_rtc_weighted_predictive_counts(self.program, C.byref(self.desc), *args),
                        "glabc_rtc_weighted_predictive_counts")


def _path_weighted(Model, theta, path):
    """The one place that decides what a weighted call runs -> the FusedWeighted of the fused path, or None for the generic one"""
    from .compiled import CompiledModel, SimulatorCompileError, SimulatorSelfCheckError
    if path not in ("auto", "fused", "generic"):
        raise ValueError('path is "auto", "fused" or "generic", got %r' % (path,))
    if path == "generic":
        return None
    on_gpu = theta.is_cuda
    if isinstance(Model, CompiledModel):
        if path == "auto" and not (on_gpu and torch.cuda.is_available()):
            return None
        if path == "fused" and not on_gpu:
            raise ValueError('path="fused" on a CompiledModel needs draws on the GPU: its weighted predictive program is launched in place')
        try:
            return FusedWeighted(Model.descriptor(), Model.weighted_predictive_program())
        except (SimulatorCompileError, SimulatorSelfCheckError) as exc:
            if path == "fused":
                raise
            warnings.warn("the weighted predictive program of this CompiledModel is not available (%s): running the generic path"
                          % (str(exc).splitlines()[0],), RuntimeWarning, stacklevel=4)
            return None
    desc = accepted(Model)              # glabc_weighted_predictive_counts examines a Model as glabc_predictive_draws does
    if path == "fused":
        if desc is None:
            raise ValueError('path="fused" needs a Model whose descriptor() glabc_weighted_predictive_counts accepts (|theta| + noise or '
                             "g-and-k) or a CompiledModel, got %r" % (type(Model).__name__,))
        if not on_gpu:
            raise ValueError('path="fused" needs draws on the GPU')
        return FusedWeighted(desc, None)
    return FusedWeighted(desc, None) if desc is not None and on_gpu else None


def _bins_weighted(bins):
    if isinstance(bins, bool) or bins != int(bins) or not 1 <= bins <= MAX_WEIGHTED_BINS:
        raise ValueError("bins must be an integer in 1..%d, got %r" % (MAX_WEIGHTED_BINS, bins))
    return int(bins)


def _fused_weighted_counts(fused, x, stride, d, w, n, scale, seed, id0, bins, lim, thr, want):
    """one glabc_weighted_predictive_counts / glabc_rtc_weighted_predictive_counts call on the dimension-major draws `x` -> (counts
    [K][bins + 3], tails [K][4], extremes [K][2]) as NumPy arrays, None for what `want` leaves out"""
    k = fused.desc.y_dim + 1
    dev = x.device
    counts = torch.zeros(k, bins + 3, dtype=torch.int64, device=dev) if "counts" in want else None
    tails = torch.zeros(k, 4, dtype=torch.int64, device=dev) if "tails" in want else None
    extremes = torch.from_numpy(np.array([KEY_NONE] * k, np.uint32).view(np.int32)).to(dev) if "extremes" in want else None
    lo = hi = None
    if counts is not None:
        lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
    ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
    with torch.cuda.device(dev):
        fused.counts(x.data_ptr(), stride, d, w.data_ptr(), n, scale, seed, id0, bins, None if lo is None else lo.ctypes.data,
                     None if hi is None else hi.ctypes.data, thr.ctypes.data if tails is not None else None, ptr(counts), ptr(tails),
                     ptr(extremes), _stream(dev))
    to_u64 = lambda t: None if t is None else t.cpu().numpy().view(np.uint64)          # noqa: E731
    return to_u64(counts), to_u64(tails), None if extremes is None else extremes.cpu().numpy().view(np.uint32)


def _torch_weighted_tables(stats, m, bins, lim, thr):
    """``_torch_tables`` with a draw adding its multiplicity m (int64 [N]) where that adds 1, a draw of multiplicity 0 left out
    -> (counts uint64 [K][bins + 3], tails uint64 [K][4]); int64 sums, exact"""
    from .weighted import _sum_slots
    k = stats.shape[1]
    counts, tails = np.zeros((k, bins + 3), np.uint64), np.zeros((k, 4), np.uint64)
    for j in range(k):
        v = stats[:, j]
        counts[j] = _sum_slots(_torch_slots(v, float(lim[j, 0]), float(lim[j, 1]), bins), m, bins + 3)
        t = torch.tensor(float(thr[j]), dtype=torch.float32, device=v.device)
        s = torch.where(v < t, 0, torch.where(v == t, 1, torch.where(v > t, 2, 3)))
        tails[j] = _sum_slots(s, m, 4)
    return counts, tails


def _weighted_tables(Model, draws, bins, range, thresholds, seed, scale, draw0, path):
    from . import weighted
    from .regression import _dimension_major
    theta, weights = weighted._draws(draws)
    n, d = theta.shape
    if d != int(Model.theta_dim):
        raise ValueError("the draws have %d coordinates, the Model's theta_dim is %d" % (d, int(Model.theta_dim)))
    bins = _bins_weighted(bins)
    _seed(seed)
    draw0 = _count("draw0", draw0, 0)
    w = weighted._weights32(theta, weights)
    scale = weighted._scale(w, scale)
    fused = _path_weighted(Model, theta, path)
    if fused is not None:
        k = fused.desc.y_dim + 1
        thr = _thresholds(Model, thresholds, k, True)
        lim = None if range is None else diagnostics._check_range(range, k)
        x, stride = _dimension_major(theta.detach())
        key = engine.draw_seed(seed)
        call = lambda lim, want: _fused_weighted_counts(fused, x, stride, d, w, n, scale, key, draw0, bins, lim, thr, want)      # noqa: E731
        if lim is None:
            _, tails, extremes = call(None, ("tails", "extremes"))
            lim = _exact_range(extremes)
            counts, _, _ = call(lim, ("counts",))
        else:
            counts, tails, _ = call(lim, ("counts", "tails"))
        # M = sum m: every draw of positive multiplicity adds it to exactly one of a statistic's four tails
        return WeightedTerms(int(tails[0].sum(dtype=np.uint64)), counts, tails, lim, thr, True, scale, n)
    stats, has_distance = _generic_stats(Model, theta, "rows", seed)
    k = stats.shape[1]
    m = weighted._multiplicity(w, scale).to(stats.device)
    thr = _thresholds(Model, thresholds, k, has_distance)
    lim = _torch_range(stats[m > 0]) if range is None else diagnostics._check_range(range, k)
    counts, tails = _torch_weighted_tables(stats, m, bins, lim, thr)
    return WeightedTerms(weighted._int_sum(m), counts, tails, lim, thr, has_distance, scale, n)


def terms_weighted(Model, draws, *, bins=64, range, thresholds=None, seed, scale, draw0=0, path="auto"):
    """The raw integer tables of a shard of weighted draws (see WeightedTerms) under an explicit `range` (K, 2) and an explicit
    `scale`, both the same on every shard: additive, so a sharded job whose ranks pass ``draw0``, the index of their first draw in
    the whole set, ``combine_weighted``s the gathered terms and counts, on the fused path, the very draws of the one-shot call."""
    if range is None:
        raise ValueError("terms_weighted needs an explicit range (K, 2): shards must bin over the same edges")
    if scale is None:
        raise ValueError("terms_weighted needs the explicit scale every shard uses")
    return _weighted_tables(Model, draws, bins, range, thresholds, seed, scale, draw0, path)


def combine_weighted(list_of_terms):
    """WeightedTerms of the concatenated shards: a plain sum of the integer tables (scales, ranges, bins and thresholds must agree)"""
    parts = list(list_of_terms)
    if not parts:
        raise ValueError("combine_weighted needs at least one WeightedTerms")
    first = parts[0]
    for t in parts[1:]:
        if t.scale != first.scale:
            raise ValueError("shards differ in scale: %r and %r" % (first.scale, t.scale))
        if (np.shape(t.counts) != np.shape(first.counts) or not np.array_equal(t.lim, first.lim) or
                not np.array_equal(t.thresholds, first.thresholds) or t.has_distance != first.has_distance):
            raise ValueError("shards differ in bins, range, thresholds or statistics")
    add = lambda field: sum(np.asarray(getattr(t, field)).astype(np.uint64) for t in parts)          # noqa: E731
    return WeightedTerms(sum(int(t.n) for t in parts), add("counts"), add("tails"), first.lim, first.thresholds, first.has_distance,
                         first.scale, sum(int(t.n_draws) for t in parts))


def check_weighted(Model, draws, *, bins=64, range=None, thresholds=None, seed, scale=None, draw0=0, path="auto"):
    """The posterior predictive check of weighted draws -> Check (see ``summary``; n = M = sum m_i, p_upper and within_epsilon the
    weighted tail probabilities).  draws: an ``smc.Population``, a ``regression.Adjusted``, a ``rejection.Rejection`` or a
    ``(theta, weights | None)`` pair.  scale: None -- ``weighted.quantize``'s default.  range: (lo, hi) or (K, 2) -- one pass;
    None -- the exact minimum and maximum of every statistic over the draws of positive multiplicity, found in a pass of its own
    (the draws regenerate bit for bit).  draw0: the id of the first draw (fused path).  path: "auto" (the kernel for descriptor
    Models and CompiledModels and draws on the GPU, else generic), "fused", "generic"."""
    return summary(_weighted_tables(Model, draws, bins, range, thresholds, seed, scale, draw0, path))
