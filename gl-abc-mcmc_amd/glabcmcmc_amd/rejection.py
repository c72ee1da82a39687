"""rejection -- plain rejection ABC: where ``epsilon`` and the chains' starting states come from, and independent exact draws.

Draw theta from the prior, simulate, keep the draws whose discrepancy is small.  A quantile of the prior-predictive distances
is the usual tolerance (``calibrate_epsilon``), the k nearest draws start k chains (``initial_state``), and accepting a draw
with probability K_eps(distance) / K_eps(0) -- the Model's own kernel -- gives independent, exact draws from the posterior the
MCMC samplers target (``sample(kernel="model")``).

Fused path.  ``glabc_abc_draws`` (include/glabc.h, csrc/glabc_abc.hip) does draw -> simulate -> distance -> acceptance in
registers; a draw is a pure function of (Model, seed, 64-bit id), so nothing but 4 bytes (the distance) or 1 byte (the
acceptance) per draw is ever stored: one sweep over all ids in launches of at most 2^24 draws, ``torch.nonzero`` for the kept
ids in ascending order, and one ``glabc_abc_draws(ids=...)`` call that regenerates theta and y of the kept draws alone.  The
order statistic of the hard kernel is exact and sort-free: ``diagnostics.select`` over ``diagnostics.key_counts`` of the
distances viewed as a (1, n_draws, 1) history.  There is no CPU implementation of this path.

A ``CompiledModel`` runs the same path through ``glabc_rtc_abc_draws``: the kernel of ``glabc_abc_draws`` compiled around the user's
simulator (``CompiledModel.draws_program``, compiled and checked once per Model), where the source has no prior of its own and the
prior is a DiagGaussian or a Uniform.  ``path="auto"`` takes it where a GPU is present; a program that fails to compile or to check
makes ``"auto"`` warn and run the generic path.  Which entry point a call runs is decided in one place, ``_path``.

Generic path (``path="generic"``): plain torch for Models neither entry point takes -- a ``CompiledModel`` with a user prior, Gamma
priors, callback Models.  theta comes from ``prior.forward`` in chunks, ``ABCset.generate_samples(theta, 1)`` and
``ABCset.discrepancy`` give the distance, the acceptance uniform is ``torch.rand``; ids are draw positions.  It runs wherever
the Model's callbacks run, CPU tensors included.

Selection rules of ``kernel="hard"`` (both paths).  epsilon given: keep distance <= float32(epsilon).  ``n_accept=k``: epsilon
is the order statistic of rank k - 1 of all n_draws distances (NaNs last) and exactly k rows return: every distance < epsilon,
then the ties == epsilon in ascending id.  ``quantile=q``: rank floor(q (n_draws - 1)), every distance <= epsilon returns.  A
NaN distance is never kept; a wanted rank that falls on a NaN is a ValueError.  Rows are in ascending id.
"""
import ctypes as C
import math
import warnings
from collections import namedtuple

import numpy as np
import torch

from . import _capi, diagnostics, engine

MAX_LAUNCH = 1 << 24              # draws per glabc_abc_draws launch of a sweep
GENERIC_CHUNK = 1 << 20           # draws per chunk of the generic path
OUTPUTS = ("theta", "y", "distance", "accept")

Rejection = namedtuple("Rejection", "theta y distance ids epsilon n_draws")
Draws = namedtuple("Draws", "theta y distance accept")


# ---------------------------------------------------------------------------------- arguments
def _count(name, value, least):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < least:
        raise ValueError("%s must be an integer >= %d, got %r" % (name, least, value))
    return int(value)


def _epsilon(ABCset, epsilon, positive):
    eps = ABCset.epsilon if epsilon is None else epsilon
    try:
        eps = float(eps)
    except (TypeError, ValueError):
        raise ValueError("epsilon must be a number, got %r" % (epsilon,)) from None
    if not math.isfinite(eps) or eps < 0.0 or (positive and eps == 0.0):
        raise ValueError("epsilon must be finite and %s 0, got %r" % (">" if positive else ">=", eps))
    return eps


def _hard_rank(n_draws, epsilon, n_accept, quantile):
    """-> the rank of the order statistic that is epsilon (None: epsilon is given), checking the three arguments"""
    if (epsilon is not None) + (n_accept is not None) + (quantile is not None) != 1:
        raise ValueError('kernel="hard" takes exactly one of epsilon, n_accept and quantile, got epsilon=%r, n_accept=%r, quantile=%r'
                         % (epsilon, n_accept, quantile))
    if n_accept is not None:
        k = _count("n_accept", n_accept, 1)
        if k > n_draws:
            raise ValueError("n_accept must be at most n_draws = %d, got %r" % (n_draws, n_accept))
        return k - 1
    if quantile is not None:
        q = float(quantile) if isinstance(quantile, (int, float, np.floating, np.integer)) and not isinstance(quantile, bool) else math.nan
        if not 0.0 <= q <= 1.0:
            raise ValueError("quantile must be a number in [0, 1], got %r" % (quantile,))
        return int(math.floor(q * (n_draws - 1)))
    return None


def accepted(ABCset, epsilon=None):
    """The glabc_model of `ABCset` if ``glabc_abc_draws`` takes it, else None.  The entry point itself is asked, with no draws:
    a refused call launches nothing, so this needs no GPU"""
    if not callable(getattr(ABCset, "descriptor", None)):
        return None
    try:
        desc = ABCset.descriptor(epsilon)
    except (NotImplementedError, ValueError):
        return None
    if not isinstance(desc, _capi.Model):
        return None
    rc = _capi.lib().glabc_abc_draws(C.byref(desc), 0, 0, None, 0, 0, C.c_void_p(8), None, None, None, None)
    return desc if rc == _capi.OK else None


class _Entry:
    """The fused draws of one Model: its glabc_model and the entry points that take it -- glabc_abc_draws / glabc_smc_draws for the
    built-in simulators, glabc_rtc_abc_draws / glabc_rtc_smc_draws with the draws program of a CompiledModel.  ``abc`` and ``smc`` (and
    ``smc_full``: glabc_smc_draws_full / glabc_rtc_smc_draws_full) take
    the arguments of the C entry points after the Model (and the population), and raise on a status other than GLABC_OK."""

    def __init__(self, desc, program=None):
        self.desc, self.program = desc, program
        self.theta_dim, self.y_dim = desc.theta_dim, desc.y_dim

    def abc(self, *args):
        lib = _capi.lib()
        if self.program is None:
            _capi.check(lib.glabc_abc_draws(C.byref(self.desc), *args), "glabc_abc_draws")
        else:
            _capi.check(lib.glabc_rtc_abc_draws(self.program, C.byref(self.desc), *args), "glabc_rtc_abc_draws")

    def smc(self, kde_desc, *args):
        lib = _capi.lib()
        if self.program is None:
            _capi.check(lib.glabc_smc_draws(C.byref(self.desc), C.byref(kde_desc), *args), "glabc_smc_draws")
        else:
            _capi.check(lib.glabc_rtc_smc_draws(self.program, C.byref(self.desc), C.byref(kde_desc), *args), "glabc_rtc_smc_draws")

    def smc_full(self, kde_desc, chol, *args):
        """``smc`` under a full-covariance perturbation kernel: `chol` is the packed lower factor, a ctypes array of floats"""
        lib = _capi.lib()
        if self.program is None:
            _capi.check(lib.glabc_smc_draws_full(C.byref(self.desc), C.byref(kde_desc), chol, *args), "glabc_smc_draws_full")
        else:
            _capi.check(lib.glabc_rtc_smc_draws_full(self.program, C.byref(self.desc), C.byref(kde_desc), chol, *args),
                        "glabc_rtc_smc_draws_full")


def _path(ABCset, path, epsilon):
    """The one place that decides what a call runs -> the _Entry of the fused path, or None for the generic one.  "fused" raises where
    no entry point takes the Model; "auto" goes generic there, and, for a CompiledModel, also without a GPU and (with a warning) where
    the draws program fails to compile or to check."""
    if path not in ("auto", "fused", "generic"):
        raise ValueError('path is "auto", "fused" or "generic", got %r' % (path,))
    if path == "generic":
        return None
    desc = accepted(ABCset, epsilon)
    if desc is not None:
        return _Entry(desc)
    from .compiled import CompiledModel, SimulatorCompileError, SimulatorSelfCheckError
    reason = ABCset.draws_refusal() if isinstance(ABCset, CompiledModel) else None
    if isinstance(ABCset, CompiledModel) and reason is None and (path == "fused" or torch.cuda.is_available()):
        try:
            return _Entry(ABCset.descriptor(epsilon), ABCset.draws_program())
        except (SimulatorCompileError, SimulatorSelfCheckError) as exc:
            if path == "fused":
                raise
            warnings.warn("the run-time compiled draw kernels are unavailable, running the generic path instead (%s)" % (exc,),
                          RuntimeWarning, stacklevel=3)
            return None
    if path == "fused":
        raise ValueError('path="fused" needs a Model whose descriptor() glabc_abc_draws accepts (|theta| + noise or g-and-k with a '
                         'DiagGaussian or Uniform prior) or a CompiledModel with a draws program, got %r%s'
                         % (type(ABCset).__name__, "" if reason is None else " (%s)" % reason))
    return None


# ---------------------------------------------------------------------------------- the fused path
def _outputs(desc, n, dev, want):
    """-> the dimension-major buffers {name: tensor} of the wanted outputs of a draws entry point (`desc`: the _Entry of the Model), and
    ptr(name): the pointer the entry point takes for an output, None where it is not wanted or there is nothing to draw"""
    shapes = {"theta": (desc.theta_dim, n), "y": (desc.y_dim, n)}
    out = {name: torch.empty(shapes.get(name, (n,)), dtype=torch.uint8 if name == "accept" else torch.float32, device=dev) for name in want}
    return out, lambda name: out[name].data_ptr() if name in out and n else None


def _launch(desc, seed, row0, ids, n, dev, want):
    """glabc_abc_draws (`desc`: the _Entry of the Model) -> the dimension-major buffers {name: tensor} of the wanted outputs"""
    out, ptr = _outputs(desc, n, dev, want)
    if n:
        with torch.cuda.device(dev):
            desc.abc(seed, row0, None if ids is None else ids.data_ptr(), n, n, ptr("theta"), ptr("y"), ptr("distance"), ptr("accept"),
                     C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    return out


def _draw_arguments(outputs, n, row0, ids, want, seed, entry):
    """What draws() here and in smc checks of its arguments -> (n, row0, want as a tuple, ids as a tensor or None, entry()).  `entry`
    resolves and checks the Model (and the population), between the scalars and the ids, where its refusals have always come"""
    n = _count("n", n, 0)
    row0 = _count("row0", row0, 0)
    want = (want,) if isinstance(want, str) else tuple(want)
    if not want or any(w not in outputs for w in want):
        raise ValueError("want names one or more of %r, got %r" % (outputs, want))
    if seed is None or isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError("seed must be an integer, got %r" % (seed,))
    desc = entry()
    if ids is not None:
        if row0 != 0:
            raise ValueError("row0 must be 0 when ids are given, got %r" % (row0,))
        ids = torch.as_tensor(ids)
        if ids.dim() != 1 or ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool or ids.numel() != n:
            raise ValueError("ids are n = %d integers, got shape %r of %s" % (n, tuple(ids.shape), ids.dtype))
        if n and int(ids.min()) < 0:
            raise ValueError("ids must be >= 0, got %d" % int(ids.min()))
    return n, row0, want, ids, desc


def draws(ABCset, n, *, seed, row0=0, ids=None, want=OUTPUTS, epsilon=None, device=None):
    """``glabc_abc_draws`` (a ``CompiledModel``: ``glabc_rtc_abc_draws``) on device tensors -> Draws(theta (n, D), y (n, YD),
    distance (n,), accept (n,) uint8), None for what `want` leaves out; theta and y are views of the kernel's dimension-major buffers.  Draw r has id ``ids[r]`` (any integers
    in 0 .. 2^63 - 1, any order, repeats allowed; `n` must be their number) or ``row0 + r``; a draw depends on (Model, seed, id) only."""
    n, row0, want, ids, desc = _draw_arguments(OUTPUTS, n, row0, ids, want, seed,
                                               lambda: _fused_entry(ABCset, _epsilon(ABCset, epsilon, True), "glabc_abc_draws"))
    dev = engine.require_device(device)
    ids = ids if ids is None else ids.to(device=dev, dtype=torch.int64).contiguous()
    out = _launch(desc, engine.draw_seed(seed), row0, ids, n, dev, want)
    return Draws(out["theta"].t() if "theta" in out else None, out["y"].t() if "y" in out else None, out.get("distance"), out.get("accept"))


def _fused_entry(ABCset, epsilon, what):
    """the _Entry of draws(): _path's "fused", with the message of the entry point the caller names"""
    try:
        return _path(ABCset, "fused", epsilon)
    except ValueError as exc:
        raise ValueError("%s does not take this Model (%s): use sample(path=\"generic\") [%s]" % (what, type(ABCset).__name__, exc)) from None


def _sweep(desc, seed, n_draws, dev, name):
    """one output of every draw 0 .. n_draws - 1, in launches of at most MAX_LAUNCH draws"""
    full = torch.empty(n_draws, dtype=torch.uint8 if name == "accept" else torch.float32, device=dev)
    size = full.element_size()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        for row0 in range(0, n_draws, MAX_LAUNCH):
            k = min(MAX_LAUNCH, n_draws - row0)
            p = full.data_ptr() + size * row0
            desc.abc(seed, row0, None, k, k, None, None, p if name == "distance" else None, p if name == "accept" else None, stream)
    return full


def _select_rank(dis, rank):
    """the order statistic of rank `rank` of a device vector of distances (NaNs last), exactly and without a sort"""
    hist = dis.view(1, -1, 1)
    x = diagnostics.select(lambda level, prefixes: diagnostics.key_counts(hist, level, prefixes), ranks=[rank])
    return float(x[0, 0])


def _kept_ids(dis, eps, k):
    """ascending positions of the kept distances: <= eps, or (k given) every one < eps and the first ties == eps up to k rows"""
    if k is None:
        return torch.nonzero(dis <= eps).view(-1)
    less = torch.nonzero(dis < eps).view(-1)
    ties = torch.nonzero(dis == eps).view(-1)[:k - less.numel()]
    return torch.sort(torch.cat([less, ties])).values


def _nan_rank(rank, n_draws):
    raise ValueError("the distance of rank %d of %d draws is NaN: fewer than %d draws have a distance" % (rank, n_draws, rank + 1))


def _fused(desc, n_draws, kernel, eps, rank, k, seed, dev, regenerate=True):
    if kernel == "model":
        ids = torch.nonzero(_sweep(desc, seed, n_draws, dev, "accept")).view(-1)
    else:
        dis = _sweep(desc, seed, n_draws, dev, "distance")
        if rank is not None:
            eps = _select_rank(dis, rank)
            if math.isnan(eps):
                _nan_rank(rank, n_draws)
        else:
            eps = float(np.float32(eps))
        if not regenerate:
            return eps
        ids = _kept_ids(dis, eps, k)
        del dis
    out = _launch(desc, seed, 0, ids, ids.numel(), dev, ("theta", "y", "distance"))
    return Rejection(out["theta"].t(), out["y"].t(), out["distance"], ids, eps, n_draws)


# ---------------------------------------------------------------------------------- the generic path
def _generic(ABCset, prior, n_draws, kernel, eps, rank, k, regenerate=True):
    keep = None if rank is None else rank + 1                     # rows that can still be among the kept ones, ties aside
    th = y = dis = ids = None
    n_valid = 0
    for first in range(0, n_draws, GENERIC_CHUNK):
        n = min(GENERIC_CHUNK, n_draws - first)
        theta = prior.forward(n)[0].to(torch.float32).reshape(n, -1)
        ys = ABCset.generate_samples(theta, 1).reshape(n, -1)
        d = ABCset.discrepancy(ys).reshape(n).to(torch.float32)
        n_valid += int((~torch.isnan(d)).sum())
        if kernel == "model":
            log_k = lambda x: ABCset.calculate_log_kernel_dis(x, eps).reshape(-1)          # noqa: E731
            p = torch.exp(log_k(d) - log_k(torch.zeros(1, dtype=d.dtype, device=d.device)))
            mask = torch.rand(n, device=d.device) < p.to(d.device)
        elif keep is None:
            mask = d <= float(np.float32(eps))
        else:
            mask = ~torch.isnan(d)
        i = torch.nonzero(mask).view(-1)
        rows = (theta[i], ys[i], d[i], i + first)
        th, y, dis, ids = rows if th is None else tuple(torch.cat(pair) for pair in zip((th, y, dis, ids), rows))
        if keep is not None and dis.numel() > keep:               # the running best: nothing above the keep-th smallest so far can stay
            i = torch.nonzero(dis <= torch.kthvalue(dis, keep).values).view(-1)
            th, y, dis, ids = th[i], y[i], dis[i], ids[i]
    if keep is not None:
        if rank >= n_valid:
            _nan_rank(rank, n_draws)
        eps = float(torch.kthvalue(dis, keep).values)
        pos = _kept_ids(dis, eps, k)                               # positions in the kept rows, which are in ascending id
        th, y, dis, ids = th[pos], y[pos], dis[pos], ids[pos]
    elif kernel == "hard":
        eps = float(np.float32(eps))
    if not regenerate:
        return eps
    return Rejection(th, y, dis, ids, eps, n_draws)


# ---------------------------------------------------------------------------------- the public surface
def _run(ABCset, n_draws, kernel, epsilon, n_accept, quantile, seed, device, path, prior, regenerate=True):
    n_draws = _count("n_draws", n_draws, 1)
    if kernel == "model":
        if n_accept is not None or quantile is not None:
            raise ValueError('kernel="model" accepts with the Model\'s own kernel at epsilon: n_accept=%r / quantile=%r belong to kernel="hard"'
                             % (n_accept, quantile))
        eps, rank = _epsilon(ABCset, epsilon, True), None
    elif kernel == "hard":
        rank = _hard_rank(n_draws, epsilon, n_accept, quantile)
        eps = _epsilon(ABCset, epsilon, False) if rank is None else None
    else:
        raise ValueError('kernel is "model" or "hard", got %r' % (kernel,))
    k = None if n_accept is None else int(n_accept)
    desc = _path(ABCset, path, eps if kernel == "model" else None)
    if desc is None:
        if prior is None or not callable(getattr(prior, "forward", None)):
            raise ValueError('path="generic" needs prior=, a distribution object with forward(n), got %r' % (prior,))
        return _generic(ABCset, prior, n_draws, kernel, eps, rank, k, regenerate)
    dev = engine.require_device(device)
    return _fused(desc, n_draws, kernel, eps, rank, k, engine.draw_seed(seed), dev, regenerate)


def sample(ABCset, n_draws, *, kernel="model", epsilon=None, n_accept=None, quantile=None, seed=None, device=None, path="auto",
           prior=None):
    """Rejection ABC over draws 0 .. n_draws - 1 -> Rejection(theta (m, D), y (m, YD), distance (m,), ids (m,) int64, epsilon,
    n_draws), rows in ascending id.  kernel="model": the draws accepted with probability K_eps(distance) / K_eps(0) at
    ``ABCset.epsilon`` (or `epsilon`): independent exact draws from the samplers' target.  kernel="hard": the draws with
    distance <= epsilon, epsilon given or the order statistic that ``n_accept`` / ``quantile`` names (module docstring).
    path: "auto" (fused where ``glabc_abc_draws`` takes the Model or a ``CompiledModel`` has a draws program and a GPU, else
    generic), "fused", "generic" (needs ``prior=``)."""
    return _run(ABCset, n_draws, kernel, epsilon, n_accept, quantile, seed, device, path, prior)


def calibrate_epsilon(ABCset, n_draws, quantile, **kw):
    """The epsilon that ``sample(kernel="hard", quantile=quantile)`` would use, as a float; nothing is regenerated"""
    if quantile is None:
        raise ValueError("calibrate_epsilon needs a quantile in [0, 1], got None")
    unknown = set(kw) - {"seed", "device", "path", "prior"}
    if unknown:
        raise ValueError("calibrate_epsilon takes seed, device, path and prior, got %r" % (sorted(unknown),))
    return _run(ABCset, n_draws, "hard", None, None, quantile, kw.get("seed"), kw.get("device"), kw.get("path", "auto"), kw.get("prior"),
                regenerate=False)


def initial_state(ABCset, n_chains, *, n_draws=None, kernel="hard", seed=None, **kw):
    """-> (Initial_theta (C, D), Initial_y (C, YD)), float32 CPU tensors every sampler and MCMCRunner.run_* takes as they are.
    kernel="hard": the n_chains nearest of n_draws (default 64 n_chains) draws.  kernel="model": the first n_chains by id of the
    draws the Model's kernel accepted -- exact draws from the target; fewer accepted than n_chains raises."""
    n_chains = _count("n_chains", n_chains, 1)
    n_draws = 64 * n_chains if n_draws is None else _count("n_draws", n_draws, 1)
    if n_draws < n_chains:
        raise ValueError("n_draws must be at least n_chains = %d, got %r" % (n_chains, n_draws))
    if kernel == "hard":
        r = sample(ABCset, n_draws, kernel="hard", n_accept=n_chains, seed=seed, **kw)
    elif kernel == "model":
        r = sample(ABCset, n_draws, kernel="model", seed=seed, **kw)
        if r.ids.numel() < n_chains:
            raise RuntimeError("only %d of %d draws were accepted at epsilon = %g, %d chains need more: raise n_draws"
                               % (r.ids.numel(), n_draws, r.epsilon, n_chains))
    else:
        raise ValueError('kernel is "model" or "hard", got %r' % (kernel,))
    to_host = lambda t: t[:n_chains].detach().to(device="cpu", dtype=torch.float32).contiguous()          # noqa: E731
    return to_host(r.theta), to_host(r.y)
