"""The part of the C ABI a user of the drop-in Python surface calls directly, at every dimension it is compiled for:
rowwise_kernel<OP, D> (glabc_dist_log_prob, glabc_model_prior_log_prob, glabc_model_discrepancy, glabc_model_log_kernel),
simulate_kernel (glabc_model_simulate, both with the noise supplied and drawn from Philox) and init_weights_kernel
(glabc_init_weights), each against a float64 NumPy restatement of the formula it evaluates (distribution.py:81-86,
123-137, 176-181; Mixture.py:19-45; GLMCMC.py:52-55).  The restatements share no code with oracle/ or csrc/.

CPU: the checker (oracle/) against float64.  GPU: the kernel against the checker bit for bit (NaN compared as NaN), and
against float64 within the same bound; the refusals; the Python surface's CUDA path against its CPU-tensor path.

Bounds.  With u = 2^-24 (half a float32 ulp, the relative error of one rounding):
  log-densities and the log-kernel: |got - exact| <= 16 u S, S = the sum of the magnitudes of the terms that are added,
      |c0| + sum |log_scale_j| + sum e_j^2 / 2 for the Gaussian, |c0| + |log eps| + e^2 / 2 for the kernel, and for the
      Gamma sum (|(a - 1) log x| + x + |gammaln| + |log scale|).  The longest path is the log-kernel at y_dim = 8: the
      difference (1 rounding, relative to a term), its square (2 + 1), three levels of torch.sum's add tree over 8 terms (3),
      the square root (halves what came before, + 1), the division (1), its square (doubles, + 1), the product with 0.5
      (exact), two more additions (2): (((1 * 2 + 1) + 3) / 2 + 1 + 1) * 2 + 1 + 2 = 15.  The Gaussian at d = 8 has the
      division, the square, + log_scale, three levels of adds and the subtraction from c0: 2 + 1 + 1 + 1 + 3 + 1 = 9.
  discrepancy: 16 u times the value (difference, square, add tree, root: (1 * 2 + 1 + 3) / 2 + 1 = 4).
  simulate: 4 u (|theta| + |loc| + |scale eps|): a product and two additions.
  init_weights: the sum of the three terms' bounds (prior, kernel, proposal).
Measured worst case in units of u S, d = 1 .. 8: the checker on the CPU (x86-64) 4.58 for dist_log_prob / the prior, 2.23
for the discrepancy, 5.86 for the log-kernel, 1.77 for init_weights; the kernels on the MI355X the same figures (they equal
the checker bit for bit in every case of this file).

Every output buffer starts as a canary and is one element longer than the entry point may write.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from glabcmcmc_amd import _capi as A
from helpers import CANARY_BITS, assert_untouched, assert_written, bits, canary_f32, dev, host

ERR_NULL, ERR_DIM, ERR_KIND, ERR_ARG = -1, -2, -3, -4          # glabc_status, include/glabc.h
U = 2.0 ** -24
FACTOR = 16
DIMS = range(1, 9)
N = 1000
EPSILONS = (1e-4, 0.05, 0.3, 2.0)
F32 = np.float32


def f32(x):
    return np.asarray(x, F32)


def same_bits(a, b):
    """bit patterns equal, any NaN equal to any NaN"""
    a, b = f32(a), f32(b)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def assert_same_bits(got, want, what):
    ok = same_bits(got, want)
    assert ok.all(), "%s: first mismatch at row %d: %r != %r" % (what, np.argwhere(~ok)[0][0], f32(got)[~ok][0], f32(want)[~ok][0])


def units(got, ref, scale, what):
    """largest |got - ref| / (u scale) over the rows with a finite reference; the others must agree exactly"""
    got, ref, scale = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(scale, np.float64)
    fin = np.isfinite(ref)
    odd = ~fin
    same = (got[odd] == ref[odd]) | (np.isnan(got[odd]) & np.isnan(ref[odd]))
    assert same.all(), "%s: non-finite rows differ: %r != %r" % (what, got[odd][~same][:4], ref[odd][~same][:4])
    assert fin.any() and np.isfinite(got[fin]).all(), what
    err = np.abs(got[fin] - ref[fin])
    zero = scale[fin] == 0
    assert (err[zero] == 0).all(), what
    return float(np.max(err[~zero] / (U * scale[fin][~zero]))) if (~zero).any() else 0.0


WORST = {}


def hold(got, ref, scale, what, factor=FACTOR):
    w = units(got, ref, scale, what)
    key = what.split(" ")[0]
    WORST[key] = max(WORST.get(key, 0.0), w)
    assert w <= factor, "%s: %.2f units of 2^-24 S (allowed %d)" % (what, w, factor)
    return w


# ---------------------------------------------------------------------------------- descriptors
def gauss_desc(loc, log_scale):
    loc, log_scale = f32(loc), f32(log_scale)
    g = A.Dist()
    g.kind, g.dim = A.DIST_DIAG_GAUSS, len(loc)
    scale = np.exp(log_scale)                                     # float32 exp: "as the caller's exp returned it"
    for j in range(len(loc)):
        g.p0[j], g.p1[j], g.p2[j] = float(loc[j]), float(log_scale[j]), float(scale[j])
    g.c0 = float(F32(-0.5 * len(loc) * math.log(2 * math.pi)))
    return g


def uniform_desc(low, high):
    low, high = f32(low), f32(high)
    g = A.Dist()
    g.kind, g.dim = A.DIST_UNIFORM, len(low)
    for j in range(len(low)):
        g.p0[j], g.p1[j], g.p2[j] = float(low[j]), float(high[j]), float(high[j] - low[j])
    g.c0 = float(F32(-math.log(float(np.prod((high - low).astype(np.float64))))))
    return g


def gamma_desc(shape, rate):
    shape, rate = f32(shape), f32(rate)
    g = A.Dist()
    g.kind, g.dim = A.DIST_GAMMA, len(shape)
    for j in range(len(shape)):
        g.p0[j], g.p1[j] = float(shape[j]), float(rate[j])
        g.p2[j] = float(F32(1) / rate[j])
        g.p3[j] = float(F32(math.lgamma(float(shape[j]))))
    return g


def params(g):
    d = g.dim
    return tuple(np.array(list(p)[:d], np.float64) for p in (g.p0, g.p1, g.p2, g.p3))


def model_desc(theta_dim, y_dim, prior, eps, sim=A.SIM_ABS_GAUSS, noise_dim=None):
    m = A.Model()
    m.sim_kind, m.theta_dim, m.y_dim, m.gk_c = sim, theta_dim, y_dim, 0.8
    m.prior = prior
    nd = y_dim if noise_dim is None else noise_dim
    m.noise = gauss_desc(0.03 * np.arange(1, nd + 1) - 0.1, np.log(0.1 + 0.07 * np.arange(nd)))
    for j in range(y_dim):
        m.y_obs[j] = float(F32(1.5 - 0.37 * j + 0.05 * j * j))    # differs in every coordinate, some negative
    kls = F32(np.log(F32(eps)))
    m.kern_log_scale, m.kern_scale = float(kls), float(np.exp(kls))
    m.kern_c0 = float(F32(-0.5 * math.log(2 * math.pi)))
    m.epsilon = float(F32(eps))
    return m


# ---------------------------------------------------------------------------------- float64 restatements
def gauss_ref(g, z):
    loc, log_scale, scale, _ = params(g)
    with np.errstate(invalid="ignore", over="ignore"):
        e = (z.astype(np.float64) - loc) / scale
        half = 0.5 * e * e
        return float(F32(g.c0)) - (log_scale + half).sum(1), abs(g.c0) + np.abs(log_scale).sum() + half.sum(1)


def uniform_ref(g, z):
    low, high, _, _ = params(g)
    with np.errstate(invalid="ignore"):
        out = ((z < low) | (z > high)).any(1)                     # distribution.py:81-86; NaN is not out of range
    return np.where(out, -np.inf, float(F32(g.c0))), np.full(len(z), abs(g.c0))


def gamma_ref(g, z):
    """log(scipy.stats.gamma.pdf) restated, -inf where the pdf is 0 (include/glabc.h), summed over the coordinates"""
    shape, _, scale, gl = params(g)
    with np.errstate(all="ignore"):
        x = z.astype(np.float64) / scale
        xl = np.where(shape == 1.0, 0.0, (shape - 1.0) * np.log(x))
        pdf = np.exp(xl - x - gl) / scale
        lp = np.where(x >= 0, np.where(pdf > 0, np.log(pdf), -np.inf), -np.inf)
        mag = np.abs(xl) + np.abs(x) + np.abs(gl) + np.abs(np.log(scale))
        return lp.sum(1), np.where(np.isfinite(mag), mag, 0.0).sum(1)


def dist_ref(g, z):
    return {A.DIST_DIAG_GAUSS: gauss_ref, A.DIST_UNIFORM: uniform_ref, A.DIST_GAMMA: gamma_ref}[g.kind](g, z)


def discrepancy_ref(m, y):
    y_obs = np.array(list(m.y_obs)[:m.y_dim], np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt(((y.astype(np.float64) - y_obs) ** 2).sum(1))


def log_kernel_ref(m, y):
    with np.errstate(invalid="ignore", over="ignore"):
        half = 0.5 * (discrepancy_ref(m, y) / float(F32(m.kern_scale))) ** 2
        return float(F32(m.kern_c0)) - (float(F32(m.kern_log_scale)) + half), abs(m.kern_c0) + abs(m.kern_log_scale) + half


# ---------------------------------------------------------------------------------- inputs
def next_after(x, to):
    return np.nextafter(f32(x), F32(to))


@functools.lru_cache(maxsize=None)
def dist_cases(d):
    """[(name, descriptor, rows float32 [n][d])]: every parameter set and edge row of the module docstring"""
    rng = np.random.default_rng([11, d])
    out = []
    loc = rng.uniform(-2, 2, d)
    sets = {"general": (loc, np.log(2.0 ** rng.uniform(-3, 2, d))), "unit": (loc, np.zeros(d))}
    last, first = np.zeros(d), np.zeros(d)
    last[d - 1], first[0] = math.log(0.75), math.log(1.5)
    sets["unit_but_last"], sets["unit_but_first"] = (loc, last), (loc, first)
    for name, (lo, ls) in sets.items():
        g = gauss_desc(lo, ls)
        p0, _, p2, _ = params(g)
        z = f32(p0 + p2 * rng.uniform(-6, 6, (N, d)))
        edge = np.tile(f32(p0), (3 * d + 1, 1))                  # row 0: the point equal to loc
        for j in range(d):
            edge[1 + j, j], edge[1 + d + j, j], edge[1 + 2 * d + j, j] = np.inf, -np.inf, np.nan
        out.append(("gauss_" + name, g, np.concatenate([z, edge])))
    low = f32(rng.uniform(-3, 0, d))
    high = f32(low + rng.uniform(0.5, 4, d))
    g = uniform_desc(low, high)
    inside = f32(low + (high - low) * rng.uniform(0.01, 0.99, (N, d)))
    inside = np.minimum(np.maximum(inside, low), high)
    rows = [inside, low[None], high[None]]
    for j in range(d):
        for v in (next_after(low[j], -np.inf), next_after(high[j], np.inf), np.nan, low[j], high[j]):
            r = inside[j].copy()
            r[j] = v
            rows.append(r[None])
    r = inside[d].copy()
    r[d - 1] = high[d - 1] + F32(0.5)                              # outside in the last coordinate only
    rows.append(r[None])
    r = inside[d + 1].copy()
    r[0] = np.nan                                                  # NaN hides nothing: the last coordinate is still outside
    if d > 1:
        r[d - 1] = low[d - 1] - F32(0.5)
    rows.append(r[None])
    out.append(("uniform", g, np.concatenate(rows)))
    shape = np.where(np.arange(d) % 2 == 0, 0.6, 2.5) + 0.1 * np.arange(d)          # both sides of 1
    if d >= 3:
        shape[2] = 1.0                                             # xlogy(0, x) = 0
    g = gamma_desc(shape, rng.uniform(0.5, 3, d))
    _, _, scale, _ = params(g)
    inside = f32(scale * rng.gamma(np.asarray(shape), size=(N, d)) + 1e-3)
    rows = [inside]
    for j in range(d):
        for v in (0.0, -0.25, 900.0 * scale[j], 2000.0 * scale[j], np.nan):        # exp(-745.2) is the last non-zero double
            r = inside[j].copy()
            r[j] = v
            rows.append(r[None])
    out.append(("gamma", g, np.concatenate(rows)))
    for _, _, z in out:
        z.setflags(write=False)
    return out


def prior_cases(d):
    """the three kinds as a Model's prior"""
    return [c for c in dist_cases(d) if c[0] in ("gauss_general", "gauss_unit_but_last", "uniform", "gamma")]


@functools.lru_cache(maxsize=None)
def y_rows(y_dim):
    rng = np.random.default_rng([12, y_dim])
    m = model_desc(1, y_dim, gauss_desc([0], [0]), 0.3)
    y_obs = f32(list(m.y_obs)[:y_dim])
    y = f32(y_obs + rng.standard_normal((N, y_dim)) * 2.0 ** rng.uniform(-12, 3, (N, 1)))
    edge = np.tile(y_obs, (2 * y_dim + 2, 1))                     # row 0: y == y_obs
    for j in range(y_dim):
        edge[1 + j, j], edge[1 + y_dim + j, j] = np.inf, np.nan
    edge[-1, 0] = -np.inf
    y = np.concatenate([y, edge])
    y.setflags(write=False)
    return y


FAR = 1e20          # finite, but its square is not a float32: both the kernel and the checker say +inf / -inf (as torch's float32 does)


# ---------------------------------------------------------------------------------- running the checker and the kernels
class Oracle:
    def __init__(self, lib):
        self.lib = lib

    def rows(self, fn, desc, z, n=None):
        n = len(z) if n is None else n
        z = np.ascontiguousarray(z, F32)
        out = canary_f32(len(z) + 1)
        assert getattr(self.lib, "oracle_" + fn)(C.byref(desc), z.ctypes.data, n, out.ctypes.data) == 0, fn
        if n == 0:
            assert_untouched(out)
            return None
        assert_written(out[:n])
        assert_untouched(out[n:])
        return out[:n]

    def simulate(self, m, theta, eps):
        n = len(theta)
        y = canary_f32(n * m.y_dim + 1)
        theta, eps = np.ascontiguousarray(theta, F32), np.ascontiguousarray(eps, F32)
        assert self.lib.oracle_model_simulate(C.byref(m), theta.ctypes.data, eps.ctypes.data, n, y.ctypes.data) == 0
        assert_written(y[:-1])
        assert_untouched(y[-1:])
        return y[:-1].reshape(n, m.y_dim)


class Hip:
    def __init__(self, lib):
        self.lib = lib

    def rows(self, fn, desc, z, n=None, rc=0):
        n = len(z) if n is None else n
        out = dev(canary_f32(len(z) + 1))
        got = getattr(self.lib, "glabc_" + fn)(C.byref(desc), dev(np.array(z, F32)).data_ptr(), n, out.data_ptr(), None)
        assert got == rc, "%s returned %d, expected %d" % (fn, got, rc)
        out = host(out)
        if rc != 0 or n == 0:
            assert_untouched(out)
            return None
        assert_written(out[:n])
        assert_untouched(out[n:])
        return out[:n]

    def simulate(self, m, theta, eps, seed=0, row0=0):
        n = len(theta)
        y = dev(canary_f32(n * m.y_dim + 1))
        e = None if eps is None else dev(np.array(eps, F32))
        assert self.lib.glabc_model_simulate(C.byref(m), dev(np.array(theta, F32)).data_ptr(), None if e is None else e.data_ptr(), n,
                                             seed, row0, y.data_ptr(), None) == 0
        y = host(y)
        assert_written(y[:-1])
        assert_untouched(y[-1:])
        return y[:-1].reshape(n, m.y_dim)


class user_simulator:
    """the checker accepts GLABC_SIM_USER descriptors once any simulator is registered; the row-wise callbacks never call it"""
    PROTO = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_void_p)

    def __init__(self, lib):
        self.lib, self.fn = lib, self.PROTO(lambda theta, eps, y: None)
        lib.oracle_set_user_simulator.restype = None
        lib.oracle_set_user_simulator.argtypes = [C.c_void_p]

    def __enter__(self):
        self.lib.oracle_set_user_simulator(C.cast(self.fn, C.c_void_p))

    def __exit__(self, *exc):
        self.lib.oracle_set_user_simulator(None)


def check_dist(run, d, checker=None):
    for name, g, z in dist_cases(d):
        ref, s = dist_ref(g, z)
        assert np.isfinite(ref[:N]).mean() > 0.9 and (~np.isfinite(ref[N:])).any(), name
        got = run.rows("dist_log_prob", g, z)
        if checker is not None:
            assert_same_bits(got, checker.rows("dist_log_prob", g, z), "dist_log_prob %s d=%d" % (name, d))
        hold(got, ref, s, "dist_log_prob %s d=%d" % (name, d))
        assert run.rows("dist_log_prob", g, z, n=0) is None         # GLABC_OK, nothing written


def check_prior(run, d, checker=None):
    for name, g, z in prior_cases(d):
        m = model_desc(d, d, g, 0.3)
        ref, s = dist_ref(g, z)
        got = run.rows("model_prior_log_prob", m, z)
        if checker is not None:
            assert_same_bits(got, checker.rows("model_prior_log_prob", m, z), "prior %s d=%d" % (name, d))
        hold(got, ref, s, "model_prior_log_prob %s d=%d" % (name, d))


def check_kernel_rows(run, m, what, checker=None):
    y = y_rows(m.y_dim)
    dis_ref = discrepancy_ref(m, y)
    lk_ref, lk_s = log_kernel_ref(m, y)
    assert dis_ref[N] == 0 and np.isinf(dis_ref[N + 1]) and np.isnan(dis_ref[N + 1 + m.y_dim])
    assert np.isfinite(lk_ref[:N]).all() and lk_ref[N + 1] == -np.inf
    dis = run.rows("model_discrepancy", m, y)
    lk = run.rows("model_log_kernel", m, y)
    far = np.full((2, m.y_dim), FAR, F32)
    far[1] = -far[1]
    dis_far, lk_far = run.rows("model_discrepancy", m, far), run.rows("model_log_kernel", m, far)
    assert (dis_far == np.inf).all() and (lk_far == -np.inf).all(), what
    if checker is not None:
        assert_same_bits(dis, checker.rows("model_discrepancy", m, y), "discrepancy " + what)
        assert_same_bits(lk, checker.rows("model_log_kernel", m, y), "log_kernel " + what)
    hold(dis, dis_ref, dis_ref, "model_discrepancy " + what)
    hold(lk, lk_ref, lk_s, "model_log_kernel " + what)
    assert dis[N] == 0 and lk[N] == F32(F32(m.kern_c0) - F32(m.kern_log_scale))          # y == y_obs


def check_model_rows(run, d, checker=None):
    for eps in EPSILONS:
        m = model_desc(d, d, gauss_desc(np.zeros(d), np.zeros(d)), eps)
        check_kernel_rows(run, m, "eps=%g d=%d" % (eps, d), checker)


def check_user_dims(run, d, checker=None):
    """theta_dim = d, y_dim = 9 - d: a swap of the two reads the wrong number of columns"""
    yd = 9 - d
    for name, g, z in prior_cases(d):
        m = model_desc(d, yd, g, 0.05, sim=A.SIM_USER, noise_dim=1 + d % 3)
        ref, s = dist_ref(g, z)
        got = run.rows("model_prior_log_prob", m, z)
        if checker is not None:
            assert_same_bits(got, checker.rows("model_prior_log_prob", m, z), "user prior %s (%d, %d)" % (name, d, yd))
        hold(got, ref, s, "model_prior_log_prob user %s (%d, %d)" % (name, d, yd))
    for eps in (0.05, 2.0):
        m = model_desc(d, yd, gauss_desc(np.zeros(d), np.zeros(d)), eps, sim=A.SIM_USER, noise_dim=1 + d % 3)
        check_kernel_rows(run, m, "user eps=%g (%d, %d)" % (eps, d, yd), checker)


# ---------------------------------------------------------------------------------- simulate
def sim_inputs(d):
    rng = np.random.default_rng([13, d])
    theta = f32(rng.standard_normal((N, d)) * 2)
    theta[::7] = -np.abs(theta[::7])
    theta[3, :] = -0.0
    theta[4, 0] = 0.0
    return theta, f32(rng.standard_normal((N, d)))


def gk_model(eps=0.3):
    from glabcmcmc_amd.examples.GK import GK_set
    return GK_set(eps).descriptor()


def gk_inputs():
    rng = np.random.default_rng(14)
    theta = f32(np.stack([rng.uniform(0, 10, N), rng.uniform(0.1, 5, N), rng.uniform(-3, 3, N), rng.uniform(0, 1, N)], 1))
    return theta, f32(rng.standard_normal((N, 8)))


def check_simulate(run, d, checker=None):
    m = model_desc(d, d, gauss_desc(np.zeros(d), np.zeros(d)), 0.3)
    theta, eps = sim_inputs(d)
    y = run.simulate(m, theta, eps)
    loc, _, scale, _ = params(m.noise)
    noise = scale * eps.astype(np.float64)
    ref = np.abs(theta.astype(np.float64)) + (loc + noise)
    s = np.abs(theta.astype(np.float64)) + np.abs(loc) + np.abs(noise)
    if checker is not None:
        assert_same_bits(y, checker.simulate(m, theta, eps), "simulate d=%d" % d)
    hold(y.ravel(), ref.ravel(), s.ravel(), "model_simulate d=%d" % d, factor=4)
    assert (y[3] == f32(loc) + f32(scale) * eps[3]).all()        # theta = -0: |-0| = +0 adds nothing


def philox_normals(oracle, seed, row0, n, count):
    """eps[n][count] of glabc_model_simulate(eps = NULL): Philox(seed; row0 + r, 0, b), word pairs (0, 1) and (2, 3) of block b
    -> normals 4b .. 4b + 3 (include/glabc.h)"""
    blocks = 2
    words = np.empty((n, blocks, 4), np.uint32)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32)
    for r in range(n):
        gid = row0 + r
        for b in range(blocks):
            ctr = np.array([gid & 0xFFFFFFFF, gid >> 32, 0, b], np.uint32)
            oracle.oracle_philox4x32_10(ctr.ctypes.data, key.ctypes.data, words[r, b].ctypes.data)
    a = np.ascontiguousarray(words[:, :, 0::2].reshape(-1))       # (r, b, pair): words 0 and 2
    b_ = np.ascontiguousarray(words[:, :, 1::2].reshape(-1))
    z0, z1 = np.empty(a.size, F32), np.empty(a.size, F32)
    oracle.oracle_normal_pair_v(a.ctypes.data, b_.ctypes.data, a.size, z0.ctypes.data, z1.ctypes.data)
    eps = np.stack([z0, z1], 1).reshape(n, blocks * 4)            # (r, b, pair, which) -> 4b + 2 pair + which
    return np.ascontiguousarray(eps[:, :count])


PHILOX_N = 257
ROW0S = (0, 2 ** 32 - 100)
SEEDS = (0x0000000512345678, 0x9ABCDEF012345678)               # equal low words


# ---------------------------------------------------------------------------------- init_weights
KINDS = ("gauss", "uniform", "gamma")
CHAINS, STRIDE = 130, 192
FLAG_CANARY = CANARY_BITS


def iw_dist(kind, d, which):
    rng = np.random.default_rng([15, d, which, KINDS.index(kind)])
    if kind == "gauss":
        return gauss_desc(rng.uniform(0.2, 1.0, d), np.log(rng.uniform(0.5, 2.0, d)))
    if kind == "uniform":
        return uniform_desc(rng.uniform(-0.5, 0.0, d), rng.uniform(2.5, 4.0, d))
    return gamma_desc(rng.uniform(0.7, 3.0, d), rng.uniform(0.5, 2.0, d))


class IwState:
    """chain-major state with NaN / canary padding; run(fn) hands a glabc_chains over host or device arrays to fn"""

    def __init__(self, d, yd, seed):
        rng = np.random.default_rng([16, d, yd, seed])
        self.theta = np.full((d, STRIDE), np.nan, F32)
        self.y = np.full((yd, STRIDE), np.nan, F32)
        self.theta[:, :CHAINS] = f32(rng.uniform(0.05, 2.4, (d, CHAINS)))
        self.theta[:, 5] = -0.3                                    # outside the Gamma's and the uniform's support
        m = model_desc(d, yd, gauss_desc(np.zeros(d), np.zeros(d)), 0.3)
        self.y[:, :CHAINS] = f32(np.array(list(m.y_obs)[:yd])[:, None] + 0.2 * rng.standard_normal((yd, CHAINS)))
        self.log_w = canary_f32(STRIDE)
        self.flags = np.full(STRIDE, FLAG_CANARY, np.uint32)
        self.flags[:CHAINS] = rng.choice(np.array([0, 1, 2, 4, 8, 14, 15], np.uint32), CHAINS)
        self.flags0 = self.flags.copy()

    def chains(self, ptr, n=CHAINS, stride=STRIDE):
        return A.Chains(n, 0, stride, ptr(self.theta), ptr(self.y), ptr(self.log_w), ptr(self.flags), None, None, None, None,
                        None)


def iw_reference(m, imp, st):
    theta, y = st.theta[:, :CHAINS].T, st.y[:, :CHAINS].T
    p, ps = dist_ref(m.prior, theta)
    k, ks = log_kernel_ref(m, y)
    q, qs = dist_ref(imp, theta)
    with np.errstate(invalid="ignore"):
        return (p + k) - q, ps + ks + qs


def iw_check_outputs(st, log_w, flags, what):
    assert_written(log_w[:CHAINS])
    assert_untouched(log_w[CHAINS:])
    assert (flags[CHAINS:] == FLAG_CANARY).all(), what + ": flags of the padding columns"
    assert (flags[:CHAINS] == (st.flags0[:CHAINS] | A.FLAG_LOCAL)).all(), what + ": flags"


def oracle_init_weights(oracle, m, imp, st):
    cs = st.chains(lambda a: a.ctypes.data)
    theta0, y0 = st.theta.copy(), st.y.copy()
    assert oracle.oracle_init_weights(C.byref(m), C.byref(imp), C.byref(cs)) == 0
    assert np.array_equal(bits(st.theta), bits(theta0)) and np.array_equal(bits(st.y), bits(y0))
    return st.log_w, st.flags


def hip_init_weights(hip, m, imp, st, rc=0, **kw):
    arrays = {id(a): dev(a) for a in (st.theta, st.y, st.log_w)}
    arrays[id(st.flags)] = dev(st.flags.view(np.int32))
    cs = st.chains(lambda a: arrays[id(a)].data_ptr(), **kw)
    got = hip.glabc_init_weights(C.byref(m), None if imp is None else C.byref(imp), C.byref(cs), None)
    assert got == rc, "glabc_init_weights returned %d, expected %d" % (got, rc)
    log_w, flags = host(arrays[id(st.log_w)]), host(arrays[id(st.flags)]).view(np.uint32)
    assert np.array_equal(bits(host(arrays[id(st.theta)])), bits(st.theta))
    if rc != 0:
        assert_untouched(log_w)
        assert (flags == st.flags0).all()
    return log_w, flags


def check_init_weights(d, run, checker=None):
    finite = 0
    for pk in KINDS:
        for ik in KINDS:
            what = "init_weights d=%d prior=%s importance=%s" % (d, pk, ik)
            m = model_desc(d, d, iw_dist(pk, d, 0), 0.3)
            imp = iw_dist(ik, d, 1)
            st = IwState(d, d, 0)
            ref, s = iw_reference(m, imp, st)
            log_w, flags = run(m, imp, st)
            iw_check_outputs(st, log_w, flags, what)
            if checker is not None:
                st2 = IwState(d, d, 0)
                want, _ = checker(m, imp, st2)
                assert_same_bits(log_w[:CHAINS], want[:CHAINS], what)
            hold(log_w[:CHAINS], ref, s, what)
            finite += int(np.isfinite(ref).sum())
    assert finite > 9 * CHAINS * 0.9


# ================================================================================== CPU: the checker against float64
@pytest.fixture(scope="module")
def chk(oracle):
    return Oracle(oracle)


@pytest.mark.parametrize("d", DIMS)
def test_checker_dist_log_prob(chk, d):
    check_dist(chk, d)
    print("checker dist_log_prob d=%d: %.2f units" % (d, WORST["dist_log_prob"]))


@pytest.mark.parametrize("d", DIMS)
def test_checker_model_prior(chk, d):
    check_prior(chk, d)


@pytest.mark.parametrize("d", DIMS)
def test_checker_discrepancy_and_log_kernel(chk, d):
    check_model_rows(chk, d)
    print("checker d=%d: discrepancy %.2f, log_kernel %.2f units" % (d, WORST["model_discrepancy"], WORST["model_log_kernel"]))


@pytest.mark.parametrize("d", DIMS)
def test_checker_user_model_dims(oracle, chk, d):
    with user_simulator(oracle):
        check_user_dims(chk, d)


@pytest.mark.parametrize("d", DIMS)
def test_checker_simulate(chk, d):
    check_simulate(chk, d)


@pytest.mark.parametrize("d", DIMS)
def test_checker_init_weights(oracle, d):
    check_init_weights(d, functools.partial(oracle_init_weights, oracle))
    print("checker init_weights d=%d: %.2f units" % (d, WORST["init_weights"]))


def test_philox_normals_layout(oracle):
    """the host construction of the eps = NULL draws: finite standard normals, a different row per counter and per seed half"""
    a = philox_normals(oracle, SEEDS[0], ROW0S[1], PHILOX_N, 8)
    assert a.shape == (PHILOX_N, 8) and np.isfinite(a).all() and 0.8 < a.std() < 1.2 and abs(a.mean()) < 0.1
    assert len(np.unique(a)) == a.size
    b = philox_normals(oracle, SEEDS[1], ROW0S[1], PHILOX_N, 8)
    c = philox_normals(oracle, SEEDS[0], ROW0S[0], PHILOX_N, 8)
    assert not np.isin(a, b).any() and not np.isin(a, c).any()
    # rows 100 .. of the second launch have crossed 2^32: the low counter word restarts at 0, the high one is 1
    assert not np.isin(a[100:], c[:157]).any()


# ================================================================================== GPU
@pytest.fixture(scope="module")
def gpu(hip):
    return Hip(hip)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_dist_log_prob(gpu, chk, d):
    check_dist(gpu, d, chk)
    print("kernel dist_log_prob d=%d: %.2f units" % (d, WORST["dist_log_prob"]))


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_model_prior_log_prob(gpu, chk, d):
    check_prior(gpu, d, chk)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_model_discrepancy_and_log_kernel(gpu, chk, d):
    check_model_rows(gpu, d, chk)
    print("kernel d=%d: discrepancy %.2f, log_kernel %.2f units" % (d, WORST["model_discrepancy"], WORST["model_log_kernel"]))


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_user_model_dims(gpu, oracle, chk, d):
    with user_simulator(oracle):
        check_user_dims(gpu, d, chk)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_model_simulate(gpu, chk, d):
    check_simulate(gpu, d, chk)


@pytest.mark.gpu
def test_model_simulate_gk(gpu, chk):
    """g-and-k (theta_dim 4, y_dim 8): the kernel restates the checker's float32 steps -- bit for bit; sorted ascending"""
    m = gk_model()
    theta, eps = gk_inputs()
    y = gpu.simulate(m, theta, eps)
    assert_same_bits(y, chk.simulate(m, theta, eps), "simulate g-and-k")
    assert (np.diff(y, axis=1) >= 0).all() and np.isfinite(y).all()


@pytest.mark.gpu
@pytest.mark.parametrize("d", list(DIMS) + ["gk"])
def test_model_simulate_philox(gpu, oracle, d):
    """eps = NULL: the draws are Philox(seed; row0 + r, 0, b) -- also where row0 + r crosses 2^32 inside the launch"""
    if d == "gk":
        m, theta, yd = gk_model(), gk_inputs()[0][:PHILOX_N], 8
    else:
        m, theta, yd = model_desc(d, d, gauss_desc(np.zeros(d), np.zeros(d)), 0.3), sim_inputs(d)[0][:PHILOX_N], d
    seen = []
    for seed in SEEDS:
        for row0 in ROW0S:
            drawn = gpu.simulate(m, theta, None, seed=seed, row0=row0)
            given = gpu.simulate(m, theta, philox_normals(oracle, seed, row0, PHILOX_N, yd))
            assert_same_bits(drawn, given, "simulate eps=NULL d=%s seed=%#x row0=%d" % (d, seed, row0))
            seen.append(drawn)
    for i in range(len(seen)):
        for j in range(i):
            assert not np.array_equal(seen[i], seen[j]), "two (seed, row0) pairs gave the same output"
    # the same global row from two launches: row0 + r is what counts
    shifted = gpu.simulate(m, theta[:50], None, seed=SEEDS[0], row0=ROW0S[1] + 100)
    again = gpu.simulate(m, np.concatenate([theta[:100], theta[:50]]), None, seed=SEEDS[0], row0=ROW0S[1])[100:]
    assert_same_bits(shifted, again, "simulate eps=NULL: rows 2^32 .. of two launches")


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_init_weights(hip, oracle, d):
    check_init_weights(d, functools.partial(hip_init_weights, hip), functools.partial(oracle_init_weights, oracle))
    print("kernel init_weights d=%d: %.2f units" % (d, WORST["init_weights"]))


@pytest.mark.gpu
def test_init_weights_gk(hip, oracle):
    """the g-and-k shape (4, 8): every importance kind, its Uniform prior"""
    for ik in KINDS:
        m, imp = gk_model(), iw_dist(ik, 4, 1)
        st, st2 = IwState(4, 8, 1), IwState(4, 8, 1)
        ref, s = iw_reference(m, imp, st)
        log_w, flags = hip_init_weights(hip, m, imp, st)
        iw_check_outputs(st, log_w, flags, "g-and-k " + ik)
        assert_same_bits(log_w[:CHAINS], oracle_init_weights(oracle, m, imp, st2)[0][:CHAINS], "init_weights g-and-k " + ik)
        hold(log_w[:CHAINS], ref, s, "init_weights g-and-k " + ik)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_init_weights_refusals(hip, d):
    """what the dispatch does not accept: a Model without a built-in simulator, y_dim != theta_dim, a proposal of another
    dimension or an unknown kind, a Gamma with shape <= 0, a stride shorter than the chains -- nothing is written"""
    good, imp = model_desc(d, d, iw_dist("gauss", d, 0), 0.3), iw_dist("gauss", d, 1)
    other = d + 1 if d < 8 else 7
    cases = [(ERR_KIND, model_desc(d, d, iw_dist("gauss", d, 0), 0.3, sim=A.SIM_USER), imp, {}),
             (ERR_DIM, model_desc(d, other, iw_dist("gauss", d, 0), 0.3), imp, {}),
             (ERR_DIM, good, iw_dist("uniform", other, 1), {}),
             (ERR_DIM, model_desc(d, d, iw_dist("gamma", other, 0), 0.3), imp, {}),
             (ERR_NULL, good, None, {}),
             (ERR_ARG, good, imp, dict(n=CHAINS, stride=CHAINS - 1)),
             (ERR_ARG, good, imp, dict(n=-1))]
    bad = iw_dist("gauss", d, 1)
    bad.kind = 3
    cases.append((ERR_KIND, good, bad, {}))
    bad = iw_dist("gamma", d, 1)
    bad.p0[d - 1] = 0.0
    cases.append((ERR_ARG, good, bad, {}))
    bad = model_desc(d, d, iw_dist("uniform", d, 0), 0.3)
    bad.prior.p1[d - 1] = float("inf")
    cases.append((ERR_ARG, bad, imp, {}))
    bad = model_desc(d, d, iw_dist("gauss", d, 0), 0.3)
    bad.noise.kind = A.DIST_UNIFORM
    cases.append((ERR_KIND, bad, imp, {}))
    for rc, m, q, kw in cases:
        hip_init_weights(hip, m, q, IwState(d, m.y_dim if 1 <= m.y_dim <= 8 else d, 2), rc=rc, **kw)
    st = IwState(d, d, 2)
    log_w, flags = hip_init_weights(hip, good, imp, st, n=0)
    assert_untouched(log_w)
    assert (flags == st.flags0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_rowwise_refusals(gpu, d):
    z = np.zeros((4, 8), F32)
    for make in (lambda: gauss_desc(np.zeros(d), np.zeros(d)), lambda: uniform_desc(np.zeros(d), np.ones(d)),
                 lambda: gamma_desc(np.ones(d) * 2, np.ones(d))):
        for dim in (0, 9, -1):
            g = make()
            g.dim = dim
            gpu.rows("dist_log_prob", g, z, rc=ERR_DIM)
        for field, value in (("p0", float("nan")), ("p1", float("inf")), ("p2", float("-inf"))):
            g = make()
            getattr(g, field)[d - 1] = value
            gpu.rows("dist_log_prob", g, z, rc=ERR_ARG)
            m = model_desc(d, d, g, 0.3)
            gpu.rows("model_prior_log_prob", m, z, rc=ERR_ARG)
        g = make()
        assert gpu.rows("dist_log_prob", g, z, n=0) is None       # GLABC_OK, nothing written
        gpu.rows("dist_log_prob", g, z, n=-1, rc=ERR_ARG)
    for shape in (0.0, -1.0):
        g = gamma_desc(np.ones(d) * 2, np.ones(d))
        g.p0[d - 1] = shape
        gpu.rows("dist_log_prob", g, z, rc=ERR_ARG)
        gpu.rows("model_prior_log_prob", model_desc(d, d, g, 0.3), z, rc=ERR_ARG)
    g = gauss_desc(np.zeros(d), np.zeros(d))
    g.p2[0] = 0.0                                                  # a scale of 0
    gpu.rows("dist_log_prob", g, z, rc=ERR_ARG)
    g = gauss_desc(np.zeros(d), np.zeros(d))
    g.kind = 3
    gpu.rows("dist_log_prob", g, z, rc=ERR_KIND)
    ok = gauss_desc(np.zeros(d), np.zeros(d))
    for fn in ("model_prior_log_prob", "model_discrepancy", "model_log_kernel"):
        for td, yd in ((0, d), (9, d), (d, 0), (d, 9)):
            m = model_desc(d, d, ok, 0.3)
            m.theta_dim, m.y_dim = td, yd
            gpu.rows(fn, m, z, rc=ERR_DIM)
        m = model_desc(d, d, ok, 0.3)
        m.kern_scale = 0.0
        gpu.rows(fn, m, z, rc=ERR_ARG)
        m = model_desc(d, d, ok, 0.3)
        m.y_obs[d - 1] = float("nan")
        gpu.rows(fn, m, z, rc=ERR_ARG)
        m = model_desc(d, d, ok, 0.3)
        m.sim_kind = 3
        gpu.rows(fn, m, z, rc=ERR_KIND)
        m = model_desc(d, d, ok, 0.3)
        assert gpu.rows(fn, m, z, n=0) is None


# ---------------------------------------------------------------------------------- the Python surface
class PriorModel:
    """AbsGaussModel with the prior, noise and y_obs of model_desc"""

    def __new__(cls, d, prior, eps):
        from helpers import AbsGaussModel
        from glabcmcmc_amd import distribution

        class _Model(AbsGaussModel):
            def _prior(self):
                return prior

            def _likelihood(self):
                n = model_desc(d, d, gauss_desc([0], [0]), eps).noise
                return distribution.DiagGaussian(d, torch.tensor(list(n.p0)[:d]), torch.tensor(list(n.p1)[:d]))

        return _Model(eps, list(model_desc(d, d, gauss_desc([0], [0]), eps).y_obs)[:d])


def surface_objects(d):
    from glabcmcmc_amd import distribution
    out = {}
    for name, g, z in dist_cases(d):
        p0, p1, _, _ = (torch.tensor(list(p)[:d], dtype=torch.float32) for p in (g.p0, g.p1, g.p2, g.p3))
        if g.kind == A.DIST_DIAG_GAUSS:
            out[name] = (distribution.DiagGaussian(d, p0, p1), g, z)
        elif g.kind == A.DIST_UNIFORM:
            out[name] = (distribution.Uniform(d, p0, p1), g, z)
        else:
            out[name] = (distribution.Gamma(p0, p1), g, z)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_python_surface(hip, d):
    """CUDA tensors run the kernels, CPU tensors the reference's torch / SciPy formulas: the two paths of one object agree"""
    for name, (obj, g, z) in surface_objects(d).items():
        _, s = dist_ref(g, z)
        zt = torch.from_numpy(np.array(z))
        cpu = obj.log_prob(zt).numpy()
        what = "%s.log_prob d=%d" % (name, d)
        if name == "gamma" and d > 3:                              # glabc_gamma_log_prob (float64) is compiled for 1 .. 3 coordinates
            with pytest.raises(ValueError):
                obj.log_prob(zt.cuda())
        else:
            hold(host(obj.log_prob(zt.cuda())), cpu, s, what)
        if name in ("gauss_general", "gauss_unit_but_last", "uniform", "gamma"):
            model = PriorModel(d, obj, 0.3)
            got = host(model.prior_log_prob(zt.cuda()))
            assert got.dtype == np.float32 and got.shape == (len(z),)
            hold(got, cpu, s, "prior_log_prob " + what)
    y = np.array(y_rows(d))
    for eps in EPSILONS:
        model = PriorModel(d, surface_objects(d)["gauss_unit"][0], eps)
        desc = model.descriptor()
        yt = torch.from_numpy(y)
        hold(host(model.discrepancy(yt.cuda())), model.discrepancy(yt).numpy(), discrepancy_ref(desc, y),
             "discrepancy surface eps=%g d=%d" % (eps, d))
        hold(host(model.calculate_log_kernel(yt.cuda())), model.calculate_log_kernel(yt).numpy(), log_kernel_ref(desc, y)[1],
             "calculate_log_kernel surface eps=%g d=%d" % (eps, d))
    model = PriorModel(d, surface_objects(d)["gauss_unit"][0], 0.3)
    theta, eps_n = sim_inputs(d)
    tt, et = torch.from_numpy(theta), torch.from_numpy(eps_n)
    cpu = model.simulate_from_noise(tt, et).numpy()
    loc, _, scale, _ = params(model.descriptor().noise)
    s = np.abs(theta.astype(np.float64)) + np.abs(loc) + np.abs(scale * eps_n.astype(np.float64))
    hold(host(model.simulate_from_noise(tt.cuda(), et.cuda())).ravel(), cpu.ravel(), s.ravel(), "simulate surface d=%d" % d,
         factor=8)                                                 # two float32 results, each within 4
