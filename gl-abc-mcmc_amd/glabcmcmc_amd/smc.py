"""smc -- ABC-SMC (population Monte Carlo): weighted particles that walk a ladder of tolerances down to the samplers' target.

Rejection from the prior (``rejection``) pays 1 / acceptance rate simulations per kept draw, and the rate collapses when the
prior is wide or epsilon small.  ABC-SMC proposes from the previous generation instead: pick an ancestor by weight, perturb it
with a Gaussian kernel (a weighted KDE of the population, ``glabc_kde_fit``; ``perturbation="full"``: below), keep the proposal if its distance is within this
generation's tolerance, and weigh it by prior density / proposal density (Beaumont et al. 2009).

Generations.  Generation 0 is ``rejection.sample(kernel="hard", n_accept=N)`` over ceil(N / quantile) prior draws, uniform
weights.  Generation t >= 1 has the tolerance max(epsilon_stop, the order statistic of rank floor(quantile (N - 1)) of the
previous distances), or the next entry of the ladder ``epsilons`` (its entries are the tolerances of generations 1, 2, ...; the
last one is epsilon_stop).  The generation that reaches epsilon_stop is the last hard one.  With ``kernel="model"`` one more
generation follows: it proposes from the last hard population and accepts with probability K_eps(distance) / K_eps(0) at
``ABCset.epsilon`` -- the Model's own kernel --, so its weighted particles target exactly the posterior the MCMC samplers target.

Fused path.  ``glabc_smc_draws`` (include/glabc.h, csrc/glabc_smc.hip) does ancestor -> perturbation -> prior density ->
simulation -> distance -> acceptance in registers; a draw is a pure function of (Model, population, key, 64-bit id).  A
generation sweeps ids 0, 1, 2, ... in launches that ask for the distance alone (4 bytes per draw; the acceptance byte alone in
the soft generation), sized from the acceptance rate seen so far; ``torch.nonzero`` finds the kept ids, the sweep stops once N
are kept, and the FIRST N BY ID are the generation: the result depends on (Model, N, settings, seed), never on how the sweep was
cut.  One ``glabc_smc_draws(ids=...)`` call regenerates theta, y, distance and log-prior of the kept draws.  A proposal of prior
density 0 has the distance +inf and is never kept.  Generation t runs under the key (seed + t * 0x632BE59BD9B4E019) mod 2^64.
There is no CPU implementation of this path.  A ``CompiledModel`` runs it through ``glabc_rtc_smc_draws``, the same kernel compiled
around the user's simulator (``rejection._path`` decides, as for ``rejection.sample``).

Generic path (``path="generic"``): plain torch on the Model's callbacks and on ``prior`` (``forward`` and ``log_prob``), for a
``CompiledModel`` with a user prior, Gamma priors and callback Models, CPU tensors included.  Ancestors come from ``torch.multinomial``, the
perturbation from ``torch.randn`` (torch's global generator), the mixture density is a chunked float64 ``logsumexp``; ids are
draw positions.  Ladder, selection and weights are the code the fused path runs.

Full-covariance perturbation (``perturbation="full"``, opt-in; Filippi et al. 2013, Beaumont et al. 2009 in its multivariate form).
theta = x_j + L z with L L^T a multiple of the weighted population covariance, instead of a product of marginals: on posteriors
with strongly correlated parameters the diagonal kernel puts most proposals off the ridge.  The factor is computed in float64 on the
host and rounded to float32; ``glabc_smc_draws_full`` draws with it from the SAME ancestor and the SAME normals as the diagonal
kernel.  The proposal density is evaluated by whitening (``_FullKernel``) with the existing mixture kernel; the generic path does
both in plain torch (``_FullMixture``).  Per-ancestor covariances are not implemented.

Weights: log w = log prior(theta) - log q(theta), q the proposal mixture, normalised in float64.  ess = 1 / sum w^2.
"""
import ctypes as C
import math
from collections import namedtuple

import numpy as np
import torch

from . import engine, rejection
from .kernel_density import KernelDensity

SEED_STEP = 0x632BE59BD9B4E019    # generation t draws under the key (seed + t * SEED_STEP) mod 2^64
MIN_LAUNCH = 1 << 14              # draws per launch of a sweep, at least (at most rejection.MAX_LAUNCH)
HEADROOM = 1.25                   # a launch is sized for the particles still missing / the rate seen, times this
LOGQ_ELEMENTS = 1 << 24           # points x centres per chunk of the generic path's mixture density
OUTPUTS = ("theta", "y", "distance", "log_prior", "accept")

Population = namedtuple("Population", "theta y distance weights epsilon ess generations")
Draws = namedtuple("Draws", "theta y distance log_prior accept")


# ---------------------------------------------------------------------------------- glabc_smc_draws
def _launch(desc, kde, seed, row0, ids, n, dev, want, chol=None):
    """glabc_smc_draws (`desc`: the rejection._Entry of the Model; `chol`, a packed factor of ``pack_cholesky``: glabc_smc_draws_full)
    -> the dimension-major buffers {name: tensor} of the wanted outputs"""
    out, ptr = rejection._outputs(desc, n, dev, want)
    if n:
        with torch.cuda.device(dev):
            args = (seed, row0, None if ids is None else ids.data_ptr(), n, n, ptr("theta"), ptr("y"), ptr("distance"), ptr("log_prior"),
                    ptr("accept"), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
            if chol is None:
                desc.smc(kde.descriptor(), *args)
            else:
                desc.smc_full(kde.descriptor(), chol, *args)
    return out


def pack_cholesky(L, dim):
    """a lower Cholesky factor (dim, dim) -> the ctypes array of dim (dim + 1) / 2 float32 the ``_full`` entry points take, packed
    row-major: entry d (d + 1) / 2 + e is L[d][e], e <= d.  The factor is finite, zero above its diagonal and positive on it."""
    try:
        m = np.array(torch.as_tensor(L).detach().cpu().numpy(), dtype=np.float32)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError("cholesky is a (%d, %d) lower triangular matrix, got %r" % (dim, dim, L)) from None
    if m.shape != (dim, dim) or not np.isfinite(m).all() or np.triu(m, 1).any() or not (np.diagonal(m) > 0).all():
        raise ValueError("cholesky is a finite (%d, %d) lower triangular matrix with a positive diagonal, got %r" % (dim, dim, L))
    return (C.c_float * (dim * (dim + 1) // 2))(*[float(m[d, e]) for d in range(dim) for e in range(d + 1)])


def draws(ABCset, population, n, *, seed, row0=0, ids=None, want=OUTPUTS, epsilon=None, device=None, cholesky=None):
    """``glabc_smc_draws`` (a ``CompiledModel``: ``glabc_rtc_smc_draws``) on device tensors -> Draws(theta (n, D), y (n, YD),
    distance (n,), log_prior (n,), accept (n,) uint8), None for what `want` leaves out; theta and y are views of the kernel's dimension-major buffers.  `population` is a fitted
    ``KernelDensity`` of theta_dim features.  Draw r has id ``ids[r]`` (any integers in 0 .. 2^63 - 1, any order, repeats allowed;
    `n` must be their number) or ``row0 + r``; a draw depends on (Model, population, seed, id) only.  The distance of a proposal
    of prior density 0 is +inf.  ``cholesky=L`` (a (D, D) lower factor): ``glabc_smc_draws_full``, the perturbation L z instead of
    the population's bandwidth times z, from the same ancestor and the same normals."""
    def entry():
        desc = rejection._fused_entry(ABCset, rejection._epsilon(ABCset, epsilon, True), "glabc_smc_draws")
        if not isinstance(population, KernelDensity) or not population._fitted:
            raise ValueError("population must be a fitted KernelDensity, got %r" % (population,))
        if population.dim != desc.theta_dim:
            raise ValueError("population has %d features, the Model %d parameters" % (population.dim, desc.theta_dim))
        return desc

    n, row0, want, ids, desc = rejection._draw_arguments(OUTPUTS, n, row0, ids, want, seed, entry)
    dev = engine.require_device(device)
    if population.device != dev:
        raise ValueError("population lives on %s, the draws on %s" % (population.device, dev))
    ids = ids if ids is None else ids.to(device=dev, dtype=torch.int64).contiguous()
    chol = None if cholesky is None else pack_cholesky(cholesky, desc.theta_dim)
    out = _launch(desc, population, engine.draw_seed(seed), row0, ids, n, dev, want, chol)
    return Draws(out["theta"].t() if "theta" in out else None, out["y"].t() if "y" in out else None, out.get("distance"),
                 out.get("log_prior"), out.get("accept"))


# ---------------------------------------------------------------------------------- arguments
def _number(name, value, low_open, high=None):
    """a finite float > low_open (and <= high)"""
    ok = isinstance(value, (int, float, np.floating, np.integer)) and not isinstance(value, bool)
    v = float(value) if ok else math.nan
    if not (math.isfinite(v) and v > low_open and (high is None or v <= high)):
        raise ValueError("%s must be a number in (%g, %s], got %r" % (name, low_open, "inf)" if high is None else "%g" % high, value))
    return v


def _ladder(epsilons):
    try:
        lad = [float(e) for e in epsilons]
    except (TypeError, ValueError):
        raise ValueError("epsilons must be a sequence of numbers, got %r" % (epsilons,)) from None
    if not lad or any(not math.isfinite(e) or e <= 0.0 for e in lad):
        raise ValueError("epsilons must be positive finite numbers, at least one, got %r" % (epsilons,))
    if any(b >= a for a, b in zip(lad, lad[1:])):
        raise ValueError("epsilons must be strictly decreasing, got %r" % (lad,))
    return [float(np.float32(e)) for e in lad]


def _bandwidth(bandwidth, dim):
    """-> a rule's name, or the fixed bandwidth as a list of `dim` floats"""
    if isinstance(bandwidth, str):
        if bandwidth not in ("silverman", "scott", "beaumont"):
            raise ValueError('bandwidth is "silverman", "scott", "beaumont", a float or a tensor, got %r' % (bandwidth,))
        return bandwidth
    try:
        bw = torch.as_tensor(bandwidth, dtype=torch.float32).detach().cpu().reshape(-1)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError('bandwidth is "silverman", "scott", "beaumont", a float or a tensor, got %r' % (bandwidth,)) from None
    if bw.numel() not in (1, dim) or not bool((torch.isfinite(bw) & (bw > 0)).all()):
        raise ValueError("a fixed bandwidth is 1 or %d positive finite numbers, got %r" % (dim, bandwidth))
    return [float(v) for v in bw.expand(dim)]


def _covariance(bandwidth, dim):
    """perturbation="full" -> a rule's name, or the fixed covariance as a float64 (D, D) array (`dim` None: any D)"""
    message = 'with perturbation="full", bandwidth is "silverman", "scott", "beaumont" or a symmetric positive-definite (D, D) matrix, got %r'
    if isinstance(bandwidth, str):
        if bandwidth not in ("silverman", "scott", "beaumont"):
            raise ValueError(message % (bandwidth,))
        return bandwidth
    try:
        cov = np.array(torch.as_tensor(bandwidth).detach().cpu().numpy(), dtype=np.float64)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(message % (bandwidth,)) from None
    if cov.ndim != 2 or cov.shape[0] != cov.shape[1] or (dim is not None and cov.shape[0] != dim) or not np.isfinite(cov).all():
        raise ValueError(message % (bandwidth,))
    if not np.allclose(cov, cov.T, rtol=1e-6, atol=0.0) or np.linalg.eigvalsh(0.5 * (cov + cov.T)).min() <= 0.0:
        raise ValueError(message % (bandwidth,))
    return 0.5 * (cov + cov.T)


def _factor(cov):
    """the float32 lower Cholesky factor (D, D) the kernels draw with, of a float64 covariance: factored in float64 on the host,
    then rounded.  A covariance that is not positive definite, or not finite, is a degenerate population"""
    smallest = math.nan
    try:
        if not np.isfinite(cov).all():
            raise np.linalg.LinAlgError("not finite")
        smallest = float(np.linalg.eigvalsh(cov).min())
        L = np.linalg.cholesky(cov).astype(np.float32)
        if not (np.isfinite(L).all() and (np.diagonal(L) > 0).all()):
            raise np.linalg.LinAlgError("the float32 factor has no positive diagonal")
    except np.linalg.LinAlgError:
        raise RuntimeError("the population is degenerate: its weighted covariance is not positive definite (smallest eigenvalue %r; "
                           "too few distinct particles, or a coordinate in which every particle has the same value?)" % (smallest,)) from None
    return L


def full_factor(theta, weights, bandwidth):
    """The factor of perturbation="full" -> L float32 (D, D) lower, numpy.  A rule's name: the weighted covariance of the particles
    in float64, with the unbiased correction 1 / (1 - sum w^2) of the diagonal rule, times rule_factor(rule)^2 -- "beaumont": twice
    the covariance, the kernel of Beaumont et al. 2009 / Filippi et al. 2013, whose marginal scales are the diagonal path's
    bandwidths.  A matrix: that covariance."""
    if not isinstance(bandwidth, str):
        return _factor(np.asarray(bandwidth, np.float64))
    x, w = theta.double(), weights.double().to(theta.device)
    mean = (w.unsqueeze(1) * x).sum(dim=0)
    xc = x - mean
    cov = (xc.t() * w) @ xc / max(1.0 - float((w * w).sum()), 1e-10)
    return _factor(rule_factor(bandwidth, theta.shape[0], theta.shape[1]) ** 2 * cov.cpu().numpy())


def _marginal_scales(L):
    """sqrt(diag(L L^T)) of the float32 factor, as floats: what `generations` reports as the bandwidth of a full run"""
    L = np.asarray(L, np.float64)
    return [float(v) for v in np.sqrt((L * L).sum(axis=1))]


def rule_factor(rule, n, dim):
    """the factor h of bandwidth = h * weighted std: Silverman's and Scott's rules as KernelDensity has them, and sqrt(2) --
    a kernel of twice the weighted variance -- of Beaumont et al. 2009"""
    if rule == "silverman":
        return (n * (dim + 2) / 4.) ** (-1. / (dim + 4))
    if rule == "scott":
        return n ** (-1. / (dim + 4))
    return math.sqrt(2.0)


def _generation_key(seed0, t):
    return (seed0 + t * SEED_STEP) & 0xFFFFFFFFFFFFFFFF


def _launch_size(need, rate, start, max_draws):
    """draws of the next launch: the particles still missing over the rate seen, with headroom, inside the limits"""
    k = int(math.ceil(HEADROOM * need / max(rate, 1e-12)))
    return max(0, min(max(k, MIN_LAUNCH), rejection.MAX_LAUNCH, max_draws - start))


def _ladder_text(gens):
    return ", ".join("%.6g" % g["epsilon"] for g in gens)


def _check_bandwidth(bw):
    bad = [j for j, v in enumerate(bw) if not (math.isfinite(v) and v > 0.0)]
    if bad:
        raise RuntimeError("the population is degenerate: the bandwidth of coordinate %d is %r (every particle has the same value there?)"
                           % (bad[0], bw[bad[0]]))


def _normalise(log_w):
    """float64 weights summing to 1 of float64 log-weights, and the effective sample size 1 / sum w^2"""
    w = torch.softmax(log_w, dim=0)
    return w, float(1.0 / (w * w).sum())


# ---------------------------------------------------------------------------------- one generation, fused
class _Rule(KernelDensity):
    """KernelDensity whose rule factor is this module's (the two rules of the class and Beaumont's)"""

    chol = None                   # the diagonal kernel: glabc_smc_draws

    def _rule_factor(self, n):
        return rule_factor(self.bandwidth, n, self.dim)


class _FullKernel:
    """The fused path's proposal under perturbation="full": q(theta) = sum_j w_j N(theta; x_j, L L^T), L the float32 factor the
    kernel draws with -- so q is the law that is sampled.  Drawing: the particles as a glabc_kde (its bandwidth holds the marginal
    scales and is not read) and the packed factor, for glabc_smc_draws_full.  Density: by whitening, u = L^-1 (theta - m) and
    c_j = L^-1 (x_j - m) in float64, m the weighted mean, cast to float32; glabc_kde_log_prob on a KernelDensity of the c_j with
    unit bandwidth, minus sum_d log L_dd in float64.  Without the centring on m the float32 casts lose the digits the differences
    u - c_j need when the population sits far from the origin."""

    def __init__(self, theta, weights, L, dev):
        self.L = L
        self.dim = theta.shape[1]
        self.chol = pack_cholesky(L, self.dim)
        self.scales = _marginal_scales(L)
        w32 = weights.to(torch.float32)
        self.kde = KernelDensity(torch.tensor(self.scales, dtype=torch.float32), device=dev).fit(theta, w32)
        self.L64 = torch.from_numpy(np.asarray(L, np.float64)).to(dev)
        self.mean = (weights.double().to(dev).unsqueeze(1) * theta.double()).sum(dim=0)
        self.white = KernelDensity(1.0, device=dev).fit(self._whiten(theta).t(), w32)
        self.log_det = float(np.log(np.diagonal(np.asarray(L, np.float64))).sum())

    def _whiten(self, rows):
        """rows (n, D) -> L^-1 (rows - m), dimension-major (D, n) float32"""
        u = torch.linalg.solve_triangular(self.L64, (rows.double() - self.mean).t(), upper=False)
        return u.to(torch.float32).contiguous()

    def descriptor(self):
        return self.kde.descriptor()

    def log_prob_soa(self, theta_soa):
        """theta dimension-major (D, n) on the device -> log q (n,) float64"""
        return self.white.log_prob_soa(self._whiten(theta_soa.t())).double() - self.log_det


class _Fused:
    def __init__(self, desc, dev, seed, full=False):
        self.desc, self.dev, self.full = desc, dev, full
        self.seed0 = engine.draw_seed(seed)

    def first(self, n_draws, N):
        r = rejection._fused(self.desc, n_draws, "hard", None, N - 1, N, _generation_key(self.seed0, 0), self.dev)
        return r.theta, r.y, r.distance, r.epsilon

    def rank(self, dis, rank):
        return rejection._select_rank(dis, rank)

    def fit(self, theta, weights, bandwidth):
        if self.full:
            kernel = _FullKernel(theta, weights, full_factor(theta, weights, bandwidth), self.dev)
            return kernel, kernel.scales
        kde = _Rule(bandwidth, device=self.dev).fit(theta, weights.to(torch.float32))
        bw = kde._consts[:kde.dim]
        _check_bandwidth(bw)
        return kde, bw

    def generation(self, t, kde, N, eps, rate, max_draws):
        """the first N draws by id that are kept (eps None: by the Model's kernel) -> theta, y, distance, log w, n_draws"""
        name = "accept" if eps is None else "distance"
        key = _generation_key(self.seed0, t)
        kept, n_kept, start = [], 0, 0
        while n_kept < N:
            k = _launch_size(N - n_kept, rate, start, max_draws)
            if k == 0:
                raise RuntimeError("generation %d kept %d of the %d particles in max_draws = %d draws (acceptance rate %.3g)"
                                   % (t, n_kept, N, max_draws, n_kept / max(start, 1)))
            buf = _launch(self.desc, kde, key, start, None, k, self.dev, (name,), kde.chol)[name]
            ids = torch.nonzero(buf if eps is None else buf <= eps).view(-1) + start
            kept.append(ids)
            n_kept += ids.numel()
            start += k
            rate = max(n_kept, 1) / start
        ids = torch.cat(kept)[:N]
        out = _launch(self.desc, kde, key, 0, ids, N, self.dev, ("theta", "y", "distance", "log_prior"), kde.chol)
        log_q = kde.log_prob_soa(out["theta"])
        log_w = out["log_prior"].double() - log_q.double()
        return out["theta"].t(), out["y"].t(), out["distance"], log_w, int(ids[-1]) + 1


# ---------------------------------------------------------------------------------- one generation, plain torch
class _Mixture:
    """the proposal of the generic path: centres x (S, D), weights (S,) float64, bandwidth (D,)"""

    def __init__(self, x, weights, bw):
        self.x, self.w, self.bw = x, weights, torch.tensor(bw, dtype=torch.float32, device=x.device)

    def sample(self, n):
        j = torch.multinomial(self.w, n, replacement=True)
        return self.x[j] + torch.randn(n, self.x.shape[1], device=self.x.device) * self.bw

    def log_prob(self, theta):
        x, bw = self.x.double(), self.bw.double()
        const = torch.log(self.w) - torch.log(bw).sum() - 0.5 * x.shape[1] * math.log(2.0 * math.pi)
        out = []
        step = max(1, LOGQ_ELEMENTS // x.shape[0])
        for first in range(0, theta.shape[0], step):
            e = (theta[first:first + step].double().unsqueeze(1) - x.unsqueeze(0)) / bw
            out.append(torch.logsumexp(const - 0.5 * (e * e).sum(dim=2), dim=1))
        return torch.cat(out) if out else torch.empty(0, dtype=torch.float64, device=theta.device)


class _FullMixture:
    """the same under perturbation="full": centres x (S, D), weights (S,) float64, the float32 factor L (D, D); plain torch, any device"""

    def __init__(self, x, weights, L):
        self.x, self.w = x, weights
        self.L = torch.from_numpy(np.asarray(L, np.float32)).to(x.device)

    def sample(self, n):
        j = torch.multinomial(self.w, n, replacement=True)
        return self.x[j] + torch.randn(n, self.x.shape[1], device=self.x.device) @ self.L.t()

    def log_prob(self, theta):
        """the Mahalanobis mixture density in float64, chunked: the whitened differences L^-1 (theta - x_j)"""
        L = self.L.double()
        white = lambda rows: torch.linalg.solve_triangular(L, rows.double().t(), upper=False).t()          # noqa: E731
        c = white(self.x)
        const = torch.log(self.w) - torch.log(torch.diagonal(L)).sum() - 0.5 * c.shape[1] * math.log(2.0 * math.pi)
        out = []
        step = max(1, LOGQ_ELEMENTS // c.shape[0])
        for first in range(0, theta.shape[0], step):
            e = white(theta[first:first + step]).unsqueeze(1) - c.unsqueeze(0)
            out.append(torch.logsumexp(const - 0.5 * (e * e).sum(dim=2), dim=1))
        return torch.cat(out) if out else torch.empty(0, dtype=torch.float64, device=theta.device)


class _Generic:
    def __init__(self, ABCset, prior, model_eps, full=False):
        self.ABCset, self.prior, self.model_eps, self.full = ABCset, prior, model_eps, full

    def first(self, n_draws, N):
        r = rejection._generic(self.ABCset, self.prior, n_draws, "hard", None, N - 1, N)
        return r.theta, r.y, r.distance, r.epsilon

    def rank(self, dis, rank):
        return float(torch.kthvalue(dis, rank + 1).values)

    def fit(self, theta, weights, bandwidth):
        if self.full:
            L = full_factor(theta, weights, bandwidth)
            return _FullMixture(theta, weights.to(theta.device), L), _marginal_scales(L)
        if isinstance(bandwidth, str):                            # the rule factor times the weighted std (unbiased, as glabc_kde_fit)
            x = theta.double()
            mean = (weights.unsqueeze(1) * x).sum(dim=0)
            var = (weights.unsqueeze(1) * (x - mean) ** 2).sum(dim=0) / max(1.0 - float((weights * weights).sum()), 1e-10)
            bw = [float(v) for v in rule_factor(bandwidth, theta.shape[0], theta.shape[1]) * var.sqrt()]
        else:
            bw = list(bandwidth)
        _check_bandwidth(bw)
        return _Mixture(theta, weights.to(theta.device), bw), bw

    def generation(self, t, mix, N, eps, rate, max_draws):
        A = self.ABCset
        rows, n_kept, start, last = [], 0, 0, -1
        while n_kept < N:
            k = min(_launch_size(N - n_kept, rate, start, max_draws), rejection.GENERIC_CHUNK)
            if k == 0:
                raise RuntimeError("generation %d kept %d of the %d particles in max_draws = %d draws (acceptance rate %.3g)"
                                   % (t, n_kept, N, max_draws, n_kept / max(start, 1)))
            theta = mix.sample(k)
            lp = self.prior.log_prob(theta).reshape(k).to(torch.float32)
            y = A.generate_samples(theta, 1).reshape(k, -1)
            d = A.discrepancy(y).reshape(k).to(torch.float32)
            d = torch.where(lp == -math.inf, torch.full_like(d, math.inf), d)
            if eps is None:
                log_k = lambda x: A.calculate_log_kernel_dis(x, self.model_eps).reshape(-1)          # noqa: E731
                p = torch.exp(log_k(d) - log_k(torch.zeros(1, dtype=d.dtype, device=d.device)))
                mask = torch.rand(k, device=d.device) < p.to(d.device)
            else:
                mask = d <= eps
            i = torch.nonzero(mask).view(-1)[:N - n_kept]
            if i.numel():
                rows.append((theta[i], y[i], d[i], lp[i]))
                last = start + int(i[-1])
            n_kept += i.numel()
            start += k
            rate = max(n_kept, 1) / start
        theta, y, d, lp = (torch.cat(c) for c in zip(*rows))
        return theta, y, d, lp.double() - mix.log_prob(theta), last + 1


# ---------------------------------------------------------------------------------- the generations
def sample(ABCset, n_particles, *, kernel="model", epsilon=None, epsilons=None, quantile=0.5, bandwidth="silverman", max_generations=30,
           max_draws=1 << 30, seed=None, device=None, path="auto", prior=None, perturbation="diagonal"):
    """ABC-SMC -> Population(theta (N, D), y (N, YD), distance (N,), weights (N,) float64 summing to 1, epsilon, ess, generations).
    kernel="model": hard generations down to `epsilon` (default 3 ``ABCset.epsilon``), then one accepted by the Model's own kernel
    at ``ABCset.epsilon``; kernel="hard": hard generations down to `epsilon`, or along the ladder `epsilons` (module docstring).
    bandwidth: "silverman" (default) / "scott": the rule's factor times the weighted std; "beaumont": sqrt(2) times it; a float or
    a tensor: fixed.  `generations` holds one dict per generation: epsilon, kernel, n_draws, rate, ess, bandwidth.
    perturbation="full": the multivariate normal kernel theta = x_j + L z instead of the product of marginals (module docstring);
    bandwidth is then a rule's name -- L L^T = rule_factor^2 times the weighted covariance, "beaumont": twice it -- or a fixed
    symmetric positive-definite (D, D) covariance, and a generation's dict also holds `cholesky` (L as a nested list), its
    `bandwidth` the marginal scales sqrt(diag(L L^T)).
    max_draws bounds the draws of one generation.  path: as in ``rejection.sample`` ("generic" needs ``prior=`` with forward and
    log_prob)."""
    N = rejection._count("n_particles", n_particles, 2)
    max_generations = rejection._count("max_generations", max_generations, 1)
    max_draws = rejection._count("max_draws", max_draws, 1)
    q = _number("quantile", quantile, 0.0, 1.0)
    if kernel not in ("model", "hard"):
        raise ValueError('kernel is "model" or "hard", got %r' % (kernel,))
    if epsilon is not None and epsilons is not None:
        raise ValueError("give epsilon or the ladder epsilons, not both: got epsilon=%r, epsilons=%r" % (epsilon, epsilons))
    ladder = None if epsilons is None else _ladder(epsilons)
    model_eps = rejection._epsilon(ABCset, None, True) if kernel == "model" else None
    if ladder is not None:
        eps_stop = ladder[-1]
    elif epsilon is not None:
        eps_stop = float(np.float32(_number("epsilon", epsilon, 0.0)))
    elif kernel == "model":
        eps_stop = float(np.float32(3.0 * model_eps))
    else:
        raise ValueError('kernel="hard" needs epsilon or the ladder epsilons')
    if perturbation not in ("diagonal", "full"):
        raise ValueError('perturbation is "diagonal" or "full", got %r' % (perturbation,))
    full = perturbation == "full"
    dim = getattr(ABCset, "theta_dim", None)
    desc = rejection._path(ABCset, path, model_eps)
    if full:
        bandwidth = _covariance(bandwidth, int(dim) if dim is not None else (desc.theta_dim if desc is not None else None))
    else:
        bandwidth = _bandwidth(bandwidth, int(dim) if dim is not None else (desc.theta_dim if desc is not None else 1))
    if desc is None:
        if prior is None or not callable(getattr(prior, "forward", None)) or not callable(getattr(prior, "log_prob", None)):
            raise ValueError('path="generic" needs prior=, a distribution object with forward(n) and log_prob(theta), got %r' % (prior,))
        run = _Generic(ABCset, prior, model_eps, full)
    else:
        run = _Fused(desc, engine.require_device(device), seed, full)

    n0 = int(math.ceil(N / q))
    theta, y, dis, eps = run.first(n0, N)
    weights = torch.full((N,), 1.0 / N, dtype=torch.float64, device=theta.device)
    ess, rate = float(N), N / n0
    gens = [dict(epsilon=eps, kernel="hard", n_draws=n0, rate=rate, ess=ess, bandwidth=None)]

    def advance(t, eps_t):
        if t > max_generations:
            raise RuntimeError("max_generations = %d reached above epsilon = %g; the ladder so far: %s" % (max_generations, eps_stop, _ladder_text(gens)))
        proposal, bw = run.fit(theta, weights, bandwidth)
        th, yy, d, log_w, n_draws = run.generation(t, proposal, N, eps_t, gens[-1]["rate"], max_draws)
        w, e = _normalise(log_w)
        gens.append(dict(epsilon=model_eps if eps_t is None else eps_t, kernel="model" if eps_t is None else "hard", n_draws=n_draws,
                         rate=N / n_draws, ess=e, bandwidth=bw))
        if full:
            gens[-1]["cholesky"] = [[float(v) for v in row] for row in proposal.L]
        return th, yy, d, w, e

    t = 0
    while eps > eps_stop:
        t += 1
        if ladder is not None:
            eps_t = ladder[t - 1]
        else:
            eps_t = max(eps_stop, float(np.float32(run.rank(dis, int(math.floor(q * (N - 1)))))))
        if not eps_t < eps:
            raise RuntimeError("the tolerance of generation %d, %g, does not decrease before epsilon = %g; the ladder so far: %s"
                               % (t, eps_t, eps_stop, _ladder_text(gens)))
        theta, y, dis, weights, ess = advance(t, eps_t)
        eps = eps_t
    if kernel == "model":
        theta, y, dis, weights, ess = advance(t + 1, None)
        eps = model_eps
    return Population(theta, y, dis, weights, eps, ess, gens)
