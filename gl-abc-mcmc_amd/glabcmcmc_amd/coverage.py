"""coverage -- is epsilon small enough?  Coverage checks of an ABC posterior on pseudo-observed data.

The test of Prangle et al. (2014; ``abctools::cov.pi``, ``abc::cv4abc``; simulation-based calibration, Talts et al. 2018): take R test
pairs (theta*, y*) with y* simulated from theta*, run ABC against each y* as if it were the observation, and record where theta*_j
ranks in the resulting posterior sample.  If the ABC posterior is the right one the ranks are uniform and the central alpha-intervals
contain theta* a share alpha of the time; a tolerance that is too loose gives an over-dispersed posterior, the ranks pile up in the
middle and the intervals cover too often.

Fused path.  ``glabc_coverage_counts`` (include/glabc.h, csrc/glabc_coverage.hip) never stores the reference table: table draw i is
``rejection.draws``' draw of id ``row0 + i`` under `seed`, bit for bit, regenerated in registers, and each test keeps 2 + D integers:
``mass = sum m``, ``mass2 = sum m^2`` and ``below_j = sum m [theta_ij < theta*_j]`` with the integer pair multiplicity m -- 1 where
the distance ``d(y_i, y*) <= width`` under ``kernel="hard"``, ``rint(65536 K(d) / K(0))`` at the test's width under ``kernel="model"``
(the Model's acceptance probability as an importance weight, quantised to 2^-16: no uniforms, no Monte-Carlo noise).  The sums are
exact and order-free, so the result is the same bits in every launch geometry and additive over shards of table draws and over slices
of tests (``terms`` / ``combine``).  Sweeps longer than ``rejection.MAX_LAUNCH`` draws are cut as ``rejection._sweep`` cuts them.
There is no CPU implementation of this path.

``quantile=q`` (hard kernel only) gives every test its own tolerance, its floor(q (n_draws - 1))-th smallest distance -- ``rejection``'s
rank rule -- found exactly and without storing a distance: 31 counting-only sweeps (``below = mass2 = NULL``) bisect the
order-preserving integer key of a non-negative float32 for all tests at once, then one full sweep follows.  Each sweep regenerates the
table: 32 sweeps in all.

Test pairs.  ``tests=None`` draws them from the prior predictive with ``rejection.draws(Model, n_tests, seed=test_seed)``,
``test_seed = seed ^ COVERAGE_TEST_KEY`` by default: an independent stream of the table's.  ``tests=(theta_star, y_star)`` or a
``rejection.Rejection`` (its kept theta and y) gives the local test of Prangle et al., pseudo-observations near ``y_obs``.  Such a
sample MUST come from another seed than the table's: otherwise every test meets itself in the table at distance 0.

Generic path (``path="generic"``; under ``"auto"`` a ``CompiledModel``, a callback Model, a Gamma prior, CPU test tensors).  Table chunks
of ``rejection.GENERIC_CHUNK`` draws come from ``rejection.draws`` where it takes the Model, else from ``prior.forward`` and
``Model.generate_samples`` (``prior=``), or from ``table=callable(row0, n) -> (theta (n, D), y (n, YD))``; the pair arithmetic is torch
int64 under the same multiplicity rule, one test at a time, so no R x n matrix ever exists.  The distance is
``distance=callable(y (n, YD), y_star (YD,)) -> (n,)``, by default the float32 Euclidean norm.  No bit-for-bit promise is made between
the generic and the fused distances; given equal distances the integers are equal.

Out of scope: a run-time compiled kernel for ``CompiledModel`` (it runs the generic path), point-estimate prediction error, id lists.
"""
import ctypes as C
import math
from collections import namedtuple
from fractions import Fraction

import numpy as np
import torch

from . import _capi, engine, rejection

COVERAGE_TEST_KEY = _capi.COVERAGE_TEST_KEY      # include/glabc.h GLABC_COVERAGE_TEST_KEY
MAX_TESTS = 1 << 20                              # GLABC_MAX_COVERAGE_TESTS
UNIT = {"hard": 1, "model": 65536}               # the multiplicity of a full-weight pair
KEY_INF = 0x7F800000                             # the integer key of +inf: a non-negative float32's bits order as the floats do
KEY_BITS = 31

# the raw integer sums, additive over shards of table draws and concatenated over slices of tests: int64 CPU tensors mass [R],
# mass2 [R], below [R][D]; widths float32 [R]; table draws row0 .. row0 + n_draws - 1; test0: the slice's first test in the whole set
Terms = namedtuple("Terms", "mass mass2 below widths n_draws row0 kernel test0")
Levels = namedtuple("Levels", "levels per_coordinate pooled n_tests")
Chi2 = namedtuple("Chi2", "value dof per_coordinate")


# ---------------------------------------------------------------------------------- the result
def _ints(t):
    """an integer tensor as a numpy array that cannot overflow in the products below: int64 where 64 bits hold 2 * 2^20 * value"""
    a = t.detach().cpu().numpy().astype(np.int64)
    return a if a.size == 0 or int(a.max()) < (1 << 40) else a.astype(object)


class Coverage:
    """The sums of a coverage check and what is read from them.  ``mass``, ``mass2`` (R,) and ``below`` (R, D) are int64 CPU
    tensors, ``widths`` (R,) float32; ``unit`` is 1 under the hard kernel and 65536 under the Model's, so a full-weight draw counts
    as one.  Tests with ``mass == 0`` (``empty``) are left out of every ratio and counted in ``n_empty``."""

    def __init__(self, mass, mass2, below, widths, n_draws, kernel):
        self.mass, self.mass2, self.below, self.widths = mass, mass2, below, widths
        self.n_draws, self.kernel, self.unit = int(n_draws), kernel, UNIT[kernel]

    @property
    def empty(self):
        return self.mass == 0

    @property
    def n_empty(self):
        return int(self.empty.sum())

    @property
    def ess(self):
        """Kish's effective sample size mass^2 / mass2 per test in units of draws (float64, NaN for an empty test); under the hard
        kernel the kept count"""
        m = self.mass.to(torch.float64)
        return torch.where(self.empty, torch.full_like(m, math.nan), m * m / self.mass2.to(torch.float64).clamp(min=1.0))

    @property
    def pit(self):
        """(below + unit / 2) / (mass + unit), (R, D) float64: the rank of theta*_j in the weighted posterior sample, NaN for an
        empty test"""
        num = 2.0 * self.below.to(torch.float64) + self.unit
        den = 2.0 * (self.mass.to(torch.float64) + self.unit)
        return torch.where(self.empty[:, None], torch.full_like(num, math.nan), num / den[:, None])

    def _live(self):
        keep = (~self.empty).numpy()
        return _ints(self.mass)[keep], _ints(self.below)[keep]

    def rank_histogram(self, bins=10):
        """-> int64 (D, bins): the non-empty tests' pit per coordinate in `bins` equal bins of [0, 1), bin floor(pit bins) decided
        in exact integer arithmetic"""
        bins = rejection._count("bins", bins, 1)
        mass, below = self._live()
        d = self.below.shape[1]
        out = np.zeros((d, bins), np.int64)
        if mass.size:
            slot = ((2 * below + self.unit) * bins) // (2 * (mass + self.unit))[:, None]          # pit < 1: below <= mass
            for j in range(d):
                out[j] = np.bincount(slot[:, j].astype(np.int64), minlength=bins)
        return torch.from_numpy(out)

    def coverage(self, levels=(0.5, 0.9, 0.95)):
        """The share of non-empty tests whose theta*_j lies in the central `level` interval, |pit - 1/2| <= level / 2 -- which is
        |2 below - mass| <= level (mass + unit), decided in exact integer arithmetic with `level` read as the nearest fraction of
        denominator <= 10^6 -> Levels(levels, per_coordinate (L, D), pooled (L,), n_tests)"""
        levels = tuple(float(v) for v in (levels if isinstance(levels, (tuple, list)) else (levels,)))
        if not levels or any(not 0.0 < v <= 1.0 for v in levels):
            raise ValueError("levels are numbers in (0, 1], got %r" % (levels,))
        mass, below = self._live()
        d = self.below.shape[1]
        per = np.full((len(levels), d), math.nan)
        for i, v in enumerate(levels):
            f = Fraction(v).limit_denominator(10 ** 6)
            if mass.size:
                inside = abs(2 * below - mass[:, None]) * f.denominator <= f.numerator * (mass + self.unit)[:, None]
                per[i] = inside.astype(np.float64).mean(axis=0)
        return Levels(levels, torch.from_numpy(per), torch.from_numpy(per.mean(axis=1)), int(mass.size))

    def chi2(self, bins=10):
        """Pearson's statistic of the rank histogram pooled over the coordinates against the uniform law -> Chi2(value, dof = bins -
        1, per_coordinate (D,)); NaN where every test is empty"""
        h = self.rank_histogram(bins).to(torch.float64)

        def stat(counts):
            e = float(counts.sum()) / bins
            return float(((counts - e) ** 2).sum() / e) if e > 0 else math.nan
        return Chi2(stat(h.sum(dim=0)), bins - 1, torch.tensor([stat(row) for row in h], dtype=torch.float64))

    def __repr__(self):
        return "Coverage(kernel=%r, n_tests=%d, n_empty=%d, n_draws=%d)" % (self.kernel, self.mass.numel(), self.n_empty, self.n_draws)


# ---------------------------------------------------------------------------------- arguments
def _kernel(kernel):
    if kernel not in UNIT:
        raise ValueError('kernel is "model" or "hard", got %r' % (kernel,))
    return kernel


def _seeds(seed, test_seed):
    for name, s in (("seed", seed), ("test_seed", test_seed)):
        if s is not None and (isinstance(s, bool) or not isinstance(s, (int, np.integer))):
            raise ValueError("%s must be an integer or None, got %r" % (name, s))
    seed = engine.draw_seed(seed)
    return seed, (seed ^ COVERAGE_TEST_KEY) if test_seed is None else engine.draw_seed(test_seed)


def _widths(Model, epsilon, n_tests, kernel):
    """-> float32 CPU tensor [n_tests]: one width for all tests or one each; the default is the samplers' target, Model.epsilon.
    +inf is a width (the posterior is then the prior); the Model's kernel needs widths > 0"""
    eps = Model.epsilon if epsilon is None else epsilon
    try:
        w = torch.as_tensor(eps).detach().to(device="cpu", dtype=torch.float32).reshape(-1)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError("epsilon is a number or %d numbers, got %r" % (n_tests, epsilon)) from None
    if w.numel() == 1:
        w = w.expand(n_tests)
    if w.numel() != n_tests:
        raise ValueError("epsilon is a number or n_tests = %d numbers, got %d" % (n_tests, w.numel()))
    if bool(torch.isnan(w).any()) or bool((w < 0).any()) or (kernel == "model" and bool((w == 0).any())):
        raise ValueError("epsilon must be %s 0 and no NaN, got %r" % (">" if kernel == "model" else ">=", epsilon))
    return w.contiguous().clone()


def _rank(n_draws, kernel, epsilon, quantile):
    if quantile is None:
        return None
    if kernel != "hard":
        raise ValueError('quantile=%r belongs to kernel="hard": the Model\'s kernel weighs every draw at epsilon' % (quantile,))
    if epsilon is not None:
        raise ValueError("give epsilon or quantile, not both: got epsilon=%r, quantile=%r" % (epsilon, quantile))
    return rejection._hard_rank(n_draws, None, None, quantile)


def _test_rows(tests, theta_dim, y_dim, n_tests):
    """tests=(theta_star, y_star) or a rejection.Rejection -> float32 (R, D), (R, YD)"""
    th, y = (tests.theta, tests.y) if isinstance(tests, rejection.Rejection) else tests if isinstance(tests, (tuple, list)) and len(tests) == 2 \
        else (None, None)
    if th is None or y is None:
        raise ValueError("tests is None, (theta_star, y_star) or a rejection.Rejection, got %r" % (type(tests).__name__,))
    th, y = torch.as_tensor(th).detach().to(torch.float32), torch.as_tensor(y).detach().to(torch.float32)
    if th.dim() != 2 or y.dim() != 2 or th.shape != (n_tests, theta_dim) or y.shape != (n_tests, y_dim):
        raise ValueError("tests are theta_star (%d, %d) and y_star (%d, %d), got %r and %r"
                         % (n_tests, theta_dim, n_tests, y_dim, tuple(th.shape), tuple(y.shape)))
    return th, y


# ---------------------------------------------------------------------------------- the exact per-test order statistic
def bisect_widths(count, n_tests, rank, device="cpu"):
    """The per-test tolerance of ``quantile=``: the smallest float32 width w >= 0 with ``count(w)[r] >= rank + 1``, where
    ``count(widths float32 [R]) -> integer tensor [R]`` counts the table's distances <= widths[r] (a NaN distance is never counted).
    That is the distance of rank `rank` among the test's distances in ascending order, NaNs last, ties included: KEY_BITS calls of
    `count`, each for all tests at once, set the bits of the width's integer key from the top.  A rank that falls on a NaN raises."""
    need = rank + 1
    key = torch.zeros(n_tests, dtype=torch.int32, device=device)
    for b in range(KEY_BITS - 1, -1, -1):
        trial = key | (1 << b)
        w = (trial - 1).clamp(max=KEY_INF).view(torch.float32)          # past +inf the keys are NaNs: count as +inf counts
        key = torch.where(count(w).to(key.device) < need, trial, key)
    if n_tests and int(key.max()) > KEY_INF:
        raise ValueError("the distance of rank %d is NaN for %d of %d tests: fewer than %d draws have a distance"
                         % (rank, int((key > KEY_INF).sum()), n_tests, need))
    return key.view(torch.float32)


# ---------------------------------------------------------------------------------- the fused path
class _Fused:
    """glabc_coverage_counts over table draws row0 .. row0 + n_draws - 1 against R tests held dimension-major on the device"""

    def __init__(self, entry, theta_star, y_star, seed, row0, n_draws, dev):
        self.desc, self.seed, self.row0, self.n_draws, self.dev = entry.desc, seed, row0, n_draws, dev
        self.r, self.d = theta_star.shape
        self.theta_star = theta_star.to(dev).t().contiguous()              # [D][R]
        self.y_star = y_star.to(dev).t().contiguous()                      # [YD][R]

    def sweep(self, widths, kernel, full):
        """-> (mass, mass2, below) int64 device tensors (full) or mass alone (a counting-only sweep: below = mass2 = NULL)"""
        widths = widths.to(device=self.dev, dtype=torch.float32).contiguous()
        mass = torch.zeros(self.r, dtype=torch.int64, device=self.dev)
        mass2 = torch.zeros(self.r, dtype=torch.int64, device=self.dev) if full else None
        below = torch.zeros(self.r, self.d, dtype=torch.int64, device=self.dev) if full else None
        lib = _capi.lib()
        with torch.cuda.device(self.dev):
            stream = C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream)
            for first in range(0, self.n_draws, rejection.MAX_LAUNCH):
                k = min(rejection.MAX_LAUNCH, self.n_draws - first)
                _capi.check(lib.glabc_coverage_counts(C.byref(self.desc), self.seed, self.row0 + first, k, self.theta_star.data_ptr(),
                                                      self.y_star.data_ptr(), widths.data_ptr(), self.r, self.r, 0 if kernel == "hard" else 1,
                                                      mass.data_ptr(), mass2.data_ptr() if full else None,
                                                      below.data_ptr() if full else None, stream), "glabc_coverage_counts")
        return (mass, mass2, below) if full else mass


# ---------------------------------------------------------------------------------- the generic path
def euclidean(y, y_star):
    """the default distance of the generic path: the float32 Euclidean norm of y (n, YD) - y_star (YD,)"""
    diff = y - y_star
    return torch.sqrt((diff * diff).sum(dim=1))


def multiplicity(d, width, kernel):
    """The integer pair multiplicity of distances d (n,) float32 at one width, include/glabc.h's rule in torch -> int64 (n,)"""
    d = d.to(torch.float32)
    width = torch.as_tensor(width, dtype=torch.float32, device=d.device)
    if kernel == "hard":
        return (d <= width).to(torch.int64)
    e = (d - 0.0) / width
    p = torch.exp(-(0.5 * (e * e)))
    return torch.where(p == p, torch.round(p * 65536.0), torch.zeros_like(p)).to(torch.int64)


class _Generic:
    """The same sums in torch int64 from table chunks of rejection.GENERIC_CHUNK draws, one test at a time"""

    def __init__(self, source, distance, theta_star, y_star, row0, n_draws):
        self.source, self.distance, self.row0, self.n_draws = source, distance, row0, n_draws
        self.theta_star, self.y_star = theta_star, y_star
        self.r, self.d = theta_star.shape

    def sweep(self, widths, kernel, full):
        dev = self.theta_star.device
        widths = widths.to(device=dev, dtype=torch.float32)
        mass = torch.zeros(self.r, dtype=torch.int64, device=dev)
        mass2, below = torch.zeros_like(mass), torch.zeros(self.r, self.d, dtype=torch.int64, device=dev)
        for first in range(0, self.n_draws, rejection.GENERIC_CHUNK):
            n = min(rejection.GENERIC_CHUNK, self.n_draws - first)
            theta, y = self.source(self.row0 + first, n)
            theta, y = theta.to(device=dev, dtype=torch.float32).reshape(n, -1), y.to(device=dev, dtype=torch.float32).reshape(n, -1)
            for r in range(self.r):
                m = multiplicity(self.distance(y, self.y_star[r]).reshape(n), widths[r], kernel)
                mass[r] += m.sum()
                if full:
                    mass2[r] += (m * m).sum()
                    below[r] += (m[:, None] * (theta < self.theta_star[r]).to(torch.int64)).sum(dim=0)
        return (mass, mass2, below) if full else mass


def _table_source(Model, entry, seed, prior, table):
    """callable(row0, n) -> (theta, y) of the generic path's table draws"""
    if table is not None:
        if not callable(table):
            raise ValueError("table is a callable(row0, n) -> (theta (n, D), y (n, YD)), got %r" % (table,))
        return table
    if entry is not None:                                               # rejection.draws takes the Model: the Philox table
        def philox(row0, n):
            d = rejection.draws(Model, n, seed=seed, row0=row0, want=("theta", "y"))
            return d.theta, d.y
        return philox
    if prior is None or not callable(getattr(prior, "forward", None)):
        raise ValueError('path="generic" on a Model rejection.draws does not take needs prior=, a distribution object with forward(n), '
                         "or table=, got prior=%r" % (prior,))

    def torch_draws(row0, n):
        theta = prior.forward(n)[0].to(torch.float32).reshape(n, -1)
        return theta, Model.generate_samples(theta, 1).reshape(n, -1)
    return torch_draws


# ---------------------------------------------------------------------------------- the public surface
def _engine(Model, n_tests, n_draws, kernel, tests, seed, test_seed, row0, device, path, prior, table, distance):
    """What a call runs -> (_Fused or _Generic, seed): the one place that decides the path, after rejection._path"""
    theta_dim, y_dim = int(Model.theta_dim), int(Model.y_dim)
    seed, test_seed = _seeds(seed, test_seed)
    if table is not None or distance is not None:
        if path == "fused":
            raise ValueError('table= and distance= belong to path="generic"')
        path = "generic"
    entry = rejection._path(Model, "auto" if path == "generic" else path, None)
    builtin = entry is not None and entry.program is None               # glabc_coverage_counts takes what glabc_abc_draws takes
    if path == "fused" and not builtin:
        raise ValueError('path="fused" needs a Model glabc_abc_draws accepts: there is no run-time compiled coverage kernel, a '
                         "CompiledModel runs path=\"generic\" (got %r)" % (type(Model).__name__,))
    rows = None if tests is None else _test_rows(tests, theta_dim, y_dim, n_tests)
    on_cpu = rows is not None and rows[0].device.type == "cpu" and rows[1].device.type == "cpu"
    fused = builtin and path != "generic" and not (path == "auto" and on_cpu)
    if fused:
        dev = engine.require_device(device)
        if rows is None:
            t = rejection.draws(Model, n_tests, seed=test_seed, want=("theta", "y"), device=dev)
            rows = (t.theta, t.y)
        return _Fused(entry, rows[0], rows[1], seed, row0, n_draws, dev), seed
    source = _table_source(Model, entry, seed, prior, table)
    if rows is None:
        if table is not None:
            raise ValueError("table= needs tests=(theta_star, y_star): the test pairs must come from another stream than the table")
        if entry is not None:
            t = rejection.draws(Model, n_tests, seed=test_seed, want=("theta", "y"), device=device)
            rows = (t.theta, t.y)
        else:
            rows = source(0, n_tests)
            rows = (rows[0].to(torch.float32).reshape(n_tests, -1), rows[1].to(torch.float32).reshape(n_tests, -1))
    return _Generic(source, euclidean if distance is None else distance, rows[0], rows[1], row0, n_draws), seed


def terms(Model, n_tests, n_draws, *, kernel="model", epsilon=None, quantile=None, tests=None, seed=None, test_seed=None, row0=0,
          test0=0, device=None, path="auto", prior=None, table=None, distance=None):
    """The integer sums of ``check`` for table draws row0 .. row0 + n_draws - 1 and the given tests -> Terms.  A sharded job gives
    every rank one `seed`, one set of test pairs (or one `test_seed`) and explicit widths; ranks that share the tests and split the
    table pass their `row0` / `n_draws`, ranks that split the tests pass their slice and `test0`, its first test's index; ``combine``
    adds the former and concatenates the latter.  ``quantile=`` depends on the whole table, so it is for a call that holds it all."""
    n_tests, n_draws = rejection._count("n_tests", n_tests, 1), rejection._count("n_draws", n_draws, 1)
    row0, test0 = rejection._count("row0", row0, 0), rejection._count("test0", test0, 0)
    if n_tests > MAX_TESTS:
        raise ValueError("n_tests is at most %d per call (slice the tests and combine), got %d" % (MAX_TESTS, n_tests))
    kernel = _kernel(kernel)
    if path not in ("auto", "fused", "generic"):
        raise ValueError('path is "auto", "fused" or "generic", got %r' % (path,))
    rank = _rank(n_draws, kernel, epsilon, quantile)
    widths = None if rank is not None else _widths(Model, epsilon, n_tests, kernel)
    run, _ = _engine(Model, n_tests, n_draws, kernel, tests, seed, test_seed, row0, device, path, prior, table, distance)
    if rank is not None:
        dev = run.dev if isinstance(run, _Fused) else run.theta_star.device
        widths = bisect_widths(lambda w: run.sweep(w, "hard", False), n_tests, rank, dev)
    mass, mass2, below = (t.cpu() for t in run.sweep(widths, kernel, True))
    return Terms(mass, mass2, below, widths.detach().to(device="cpu", dtype=torch.float32), n_draws, row0, kernel, test0)


def combine(parts):
    """Terms of shards -> Coverage of the whole job, exactly: parts with the same `test0` hold the same tests against different table
    draws and add (their widths must agree); the groups are slices of tests and are concatenated in ascending `test0`"""
    parts = list(parts)
    if not parts or any(not isinstance(p, Terms) for p in parts):
        raise ValueError("combine takes a non-empty list of Terms")
    if len({p.kernel for p in parts}) != 1:
        raise ValueError("the parts were counted under different kernels: %r" % sorted({p.kernel for p in parts}))
    groups = {}
    for p in parts:
        g = groups.get(p.test0)
        if g is None:
            groups[p.test0] = [p.mass.clone(), p.mass2.clone(), p.below.clone(), p.widths, p.n_draws]
            continue
        if g[0].shape != p.mass.shape or not torch.equal(g[3].view(torch.int32), p.widths.view(torch.int32)):
            raise ValueError("parts with test0 = %d hold different tests or widths" % p.test0)
        g[0] += p.mass
        g[1] += p.mass2
        g[2] += p.below
        g[4] += p.n_draws
    order = [groups[k] for k in sorted(groups)]
    if len({g[4] for g in order}) != 1:
        raise ValueError("the slices of tests met different numbers of table draws: %r" % [g[4] for g in order])
    return Coverage(torch.cat([g[0] for g in order]), torch.cat([g[1] for g in order]), torch.cat([g[2] for g in order]),
                    torch.cat([g[3] for g in order]), order[0][4], parts[0].kernel)


def check(Model, n_tests, n_draws, *, kernel="model", epsilon=None, quantile=None, tests=None, seed=None, test_seed=None, row0=0,
          device=None, path="auto", prior=None, table=None, distance=None):
    """The coverage check of `Model`'s ABC posterior at `epsilon` on `n_tests` test pairs against a table of `n_draws` prior draws
    -> Coverage (module docstring).  kernel: "model" (the Model's kernel at epsilon as an importance weight) or "hard" (distance <=
    epsilon); epsilon: one width or n_tests of them, default ``Model.epsilon``; quantile (hard only): every test's own tolerance, its
    floor(q (n_draws - 1))-th smallest distance; tests: None (prior-predictive pairs under `test_seed`), (theta_star, y_star) or a
    ``rejection.Rejection`` drawn under ANOTHER seed than `seed`; path: "auto", "fused", "generic" (``prior=`` / ``table=`` /
    ``distance=`` are the generic path's)."""
    return combine([terms(Model, n_tests, n_draws, kernel=kernel, epsilon=epsilon, quantile=quantile, tests=tests, seed=seed,
                          test_seed=test_seed, row0=row0, device=device, path=path, prior=prior, table=table, distance=distance)])
