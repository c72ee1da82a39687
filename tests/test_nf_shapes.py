"""The RealNVP kernels of glabc_nf.hip and glabc_nf_train.hip at every launch shape and edge row.

What is held to what
  * oracle_nf_sample / oracle_nf_log_prob / oracle_nf_inverse (the CPU checker, float32 in the kernel's operation order) are
    held to a plain NumPy float64 restatement of RealNVP (f64_sample, f64_inverse below) whose exact inputs are the float32
    numbers the kernel receives: the packed blob and the descriptor's base_loc / base_log_scale / base_scale / base_c0 as stored.
  * the kernels are held to the checker bit for bit at every branch of the host launch code (nf_geometry restates it), and
    one GPU test holds them to float64 directly, so a change made identically in kernel and checker is caught as well.
  * glabc_nf_grad keeps the project's rule (loss 2e-6 relative, every tensor 2e-4 of the checker tensor's largest entry);
    glabc_adam_step is bit-equal to oracle_adam_step.

Tolerance.  F64_ATOL is four times the checker's largest absolute error against float64 over its cases (make_flow with 1, 2, 3,
8 and 32 couplings on F64_ROWS rows, and the reference's own initialisation), over z, log_q, log_prob, inverse z_out and trace,
measured on the CPU; test_checker_matches_float64 re-measures it.  Once the kernel is bit-equal the checker's error is the
kernel's error; the factor covers other seeds.

ReLU of a NaN.  The kernels (and the checker) take max(a, 0) with fmaxf, which returns 0 for a NaN pre-activation where
torch.relu returns NaN ("Non-finite rows in the flow kernels"): a row with a non-finite coordinate keeps its
neighbours' bits untouched, its log_q is never a finite number, but single outputs of that row can be finite or infinite where
a NaN-propagating evaluation has NaN.  The tests assert exactly that: the classes (finite / +inf / -inf / NaN) of the
row's outputs equal those of the float64 restatement written with fmax, and differ from the one written with NumPy's
NaN-propagating maximum only where the latter has NaN.
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from glabcmcmc_amd import _capi as A
from glabcmcmc_amd.flows import RealNVP
from helpers import assert_untouched, assert_written, bits, canary_f32, canary_left, dev, host
from test_nf import host_descriptor, make_flow
from test_nf_train import (assert_close, autograd_gradient, hip_gradient, oracle_gradient, sections,
                           trained_looking_flow)

H = 128
NC_FLOATS = A.NF_COUPLING_FLOATS
ERR_NULL, ERR_ARG = -1, -4               # glabc_status, include/glabc.h
TAIL = 67                                # canary elements behind every output

# 4 x the checker's largest absolute error against the float64 restatement over these cases: measured 5.4e-6 on the CPU (x86-64;
# 32 couplings, log_prob).  Per quantity: z 3.0e-6, log_q 3.6e-6, log_prob 5.4e-6, inverse z_out 2.1e-6, trace 1.9e-6; with one
# coupling 3.3e-7, 8.6e-7, 1.6e-6, 2.5e-7, 0.
F64_MEASURED = 5.4e-6
F64_ATOL = 4 * F64_MEASURED
F64_COUPLINGS = (1, 2, 3, 8, 32)
F64_ROWS = 4096


# ---------------------------------------------------------------------------------------------------------------- float64
def f64_blocks(f, blob):
    b = np.asarray(blob, np.float32).reshape(-1, NC_FLOATS).astype(np.float64)
    out = []
    for blk in b:
        v4 = blk[H * H + 2 * H:H * H + 6 * H].reshape(H, 4)
        out.append(dict(W2T=blk[:H * H].reshape(H, H), W1=blk[H * H:H * H + H], b1=blk[H * H + H:H * H + 2 * H], b2=v4[:, 0],
                        W3=v4[:, 1:3], b3=blk[H * H + 6 * H:H * H + 6 * H + 2]))
    base = dict(loc=np.array(list(f.base_loc), np.float64), ls=np.array(list(f.base_log_scale), np.float64),
                sc=np.array(list(f.base_scale), np.float64), c0=float(f.base_c0))
    return out, base


def f64_conditioner(blk, t, relu):
    h1 = relu(np.multiply.outer(t, blk["W1"]) + blk["b1"], 0.0)
    h2 = relu(h1 @ blk["W2T"] + blk["b2"], 0.0)
    p = h2 @ blk["W3"] + blk["b3"]
    return p[:, 0], p[:, 1]


def f64_sample(f, blob, eps, relu=np.maximum):
    """eps [2][n] -> z [2][n], log_q [n] (nf.NormalizingFlow.sample: base draw, then coupling + swap, coupling by coupling)"""
    blocks, b = f64_blocks(f, blob)
    with np.errstate(all="ignore"):
        e = np.asarray(eps, np.float64)
        z0, z1 = b["loc"][0] + b["sc"][0] * e[0], b["loc"][1] + b["sc"][1] * e[1]
        lq = b["c0"] - ((b["ls"][0] + 0.5 * e[0] ** 2) + (b["ls"][1] + 0.5 * e[1] ** 2))
        for blk in blocks:
            shift, log_s = f64_conditioner(blk, z0, relu)
            z0, z1 = z1 * np.exp(log_s) + shift, z0
            lq = lq - log_s
    return np.stack([z0, z1]), lq


def f64_inverse(f, blob, x, relu=np.maximum):
    """x [2][n] -> z [2][n], log_prob [n], trace [n_couplings][n] (the conditioner input each coupling saw)"""
    blocks, b = f64_blocks(f, blob)
    with np.errstate(all="ignore"):
        xx = np.asarray(x, np.float64)
        z0, z1, lq = xx[0], xx[1], np.zeros(xx.shape[1])
        trace = np.empty((len(blocks), xx.shape[1]))
        for c in range(len(blocks) - 1, -1, -1):
            t0, t1 = z1, z0
            trace[c] = t0
            shift, log_s = f64_conditioner(blocks[c], t0, relu)
            z0, z1 = t0, (t1 - shift) * np.exp(-log_s)
            lq = lq - log_s
        e0, e1 = (z0 - b["loc"][0]) / b["sc"][0], (z1 - b["loc"][1]) / b["sc"][1]
        lp = b["c0"] - ((b["ls"][0] + 0.5 * e0 ** 2) + (b["ls"][1] + 0.5 * e1 ** 2))
    return np.stack([z0, z1]), lq + lp, trace


# ---------------------------------------------------------------------------------------------------------------- checker
def chk_sample(oracle, f, eps, n, seed=0, row0=0):
    z, lq = np.empty((2, n), np.float32), np.empty(n, np.float32)
    e = None if eps is None else np.ascontiguousarray(eps, np.float32)
    assert oracle.oracle_nf_sample(C.byref(f), None if e is None else e.ctypes.data, seed, row0, n, z.ctypes.data,
                                   lq.ctypes.data) == 0
    return z, lq


def chk_inverse(oracle, f, x):
    x = np.ascontiguousarray(x, np.float32)
    n = x.shape[1]
    z, lq, tr = np.empty((2, n), np.float32), np.empty(n, np.float32), np.empty((f.n_couplings, n), np.float32)
    assert oracle.oracle_nf_inverse(C.byref(f), x.ctypes.data, n, z.ctypes.data, lq.ctypes.data, tr.ctypes.data) == 0
    return z, lq, tr


def chk_log_prob(oracle, f, x):
    x = np.ascontiguousarray(x, np.float32)
    lq = np.empty(x.shape[1], np.float32)
    assert oracle.oracle_nf_log_prob(C.byref(f), x.ctypes.data, x.shape[1], lq.ctypes.data) == 0
    return lq


_CASES = {}


def case(n_couplings, n, kind="make_flow", scale=0.3):
    """(flow, host descriptor, host blob, eps [2][n]) of a shape: one flow per coupling count, one noise array per n"""
    key = (n_couplings, n, kind, scale)
    if key not in _CASES:
        if kind == "init":
            torch.manual_seed(300 + n_couplings)
            flow = RealNVP(n_couplings)                       # the reference's initialisation: W3 = b3 = 0
        else:
            flow = make_flow(n_couplings, 20 + n_couplings, scale)      # the flows of tests/test_nf.py
        f, blob = host_descriptor(flow)
        eps = np.random.default_rng(1000 + n).standard_normal((2, n)).astype(np.float32)
        _CASES[key] = (flow, f, blob, eps)
    return _CASES[key]


def same(a, b):
    """bit-equal, or NaN in both (payloads are not compared)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def classes(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN -- of the value as a float32 holds it"""
    with np.errstate(all="ignore"):
        a = np.asarray(a, np.float64).astype(np.float32)
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 1, np.where(np.isneginf(a), 2, 0)))


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("n_couplings", [1, 3, 8])
def test_oracle_inverse_is_log_prob_with_the_point_and_the_trace(oracle, n_couplings):
    flow, f, blob, eps = case(n_couplings, 1000)
    x, _ = chk_sample(oracle, f, eps, 1000)
    z, lq, tr = chk_inverse(oracle, f, x)
    assert np.array_equal(bits(lq), bits(chk_log_prob(oracle, f, x)))
    # z_out and trace are optional; log_q does not depend on them
    lq2 = np.empty(1000, np.float32)
    assert oracle.oracle_nf_inverse(C.byref(f), x.ctypes.data, 1000, None, lq2.ctypes.data, None) == 0
    assert np.array_equal(bits(lq2), bits(lq))
    # the last coupling applied in sample is the first undone: it saw x1; the base point returns to eps
    assert np.array_equal(bits(tr[n_couplings - 1]), bits(x[1]))
    assert np.array_equal(bits(tr[0]), bits(z[0]))
    loc, sc = np.array(list(f.base_loc))[:, None], np.array(list(f.base_scale))[:, None]
    assert np.abs((z - loc) / sc - eps).max() < 1e-4
    assert oracle.oracle_nf_inverse(C.byref(f), None, 1000, z.ctypes.data, lq.ctypes.data, tr.ctypes.data) == ERR_NULL
    assert oracle.oracle_nf_inverse(C.byref(f), x.ctypes.data, 1000, z.ctypes.data, None, tr.ctypes.data) == ERR_NULL


def checker_errors(oracle, f, blob, eps):
    """largest |checker - float64| of (z, log_q, log_prob, inverse z_out, trace) on one flow"""
    n = eps.shape[1]
    z, lq = chk_sample(oracle, f, eps, n)
    z64, lq64 = f64_sample(f, blob, eps)
    zi, lp, tr = chk_inverse(oracle, f, z)
    zi64, lp64, tr64 = f64_inverse(f, blob, z)
    assert np.array_equal(bits(lp), bits(chk_log_prob(oracle, f, z)))
    return {"z": np.abs(z - z64).max(), "log_q": np.abs(lq - lq64).max(), "log_prob": np.abs(lp - lp64).max(),
            "z_out": np.abs(zi - zi64).max(), "trace": np.abs(tr - tr64).max()}


@pytest.mark.parametrize("n_couplings", F64_COUPLINGS)
def test_checker_matches_float64(oracle, n_couplings):
    flow, f, blob, eps = case(n_couplings, F64_ROWS)
    err = checker_errors(oracle, f, blob, eps)
    print("checker vs float64, %d couplings: %s" % (n_couplings, ", ".join("%s %.3g" % kv for kv in err.items())))
    assert max(err.values()) <= F64_ATOL, err


def test_checker_matches_float64_at_the_reference_initialisation(oracle):
    """W3 = 0 (GLMCMC_NFs.py:56): every coupling is the identity, the flow is its base density, in all three statements"""
    flow, f, blob, eps = case(4, F64_ROWS, "init")
    err = checker_errors(oracle, f, blob, eps)
    print("checker vs float64, reference initialisation: %s" % ", ".join("%s %.3g" % kv for kv in err.items()))
    assert max(err.values()) <= F64_ATOL, err
    z64, lq64 = f64_sample(f, blob, eps)
    assert np.array_equal(z64, eps.astype(np.float64))                               # 4 swaps, loc 0, scale 1
    assert np.allclose(lq64, -np.log(2 * np.pi) - 0.5 * (eps.astype(np.float64) ** 2).sum(0), rtol=0, atol=1e-7)
    assert np.allclose(f64_inverse(f, blob, eps)[1], lq64, rtol=0, atol=1e-12)


EDGE_VALUES = [np.nan, np.inf, -np.inf, 1e30, -1e30, 1e-40, 0.0, -0.0]


def edge_rows(n_values=len(EDGE_VALUES)):
    """(value, coordinate, row of the first 64) in turn: both tiles of the pair, both halves of a tile"""
    return [(v, j, (7 * (2 * k + j) + 3) % 64) for k, v in enumerate(EDGE_VALUES[:n_values]) for j in (0, 1)]


def assert_documented_classes(f, blob, value, e, xx, got_f, got_i):
    for tag, got, want_fmax, want_prop in (
            ("forward", got_f, f64_sample(f, blob, e, relu=np.fmax), f64_sample(f, blob, e, relu=np.maximum)),
            ("inverse", got_i, f64_inverse(f, blob, xx, relu=np.fmax), f64_inverse(f, blob, xx, relu=np.maximum))):
        g = classes(np.concatenate([np.ravel(a) for a in got]))
        wf = classes(np.concatenate([np.ravel(a) for a in want_fmax]))
        wp = classes(np.concatenate([np.ravel(a) for a in want_prop]))
        assert np.array_equal(g, wf), (tag, value, g, wf)
        assert (wp[g != wp] == 3).all(), (tag, value, g, wp)                  # only ever a NaN of the propagating statement
        if np.isfinite(value) and abs(value) < 1.0:
            assert np.array_equal(g, wp) and (g == 0).all(), (tag, value)
        if not np.isfinite(value):
            assert classes(np.ravel(got[1]))[0] != 0, (tag, value)            # the row's density is never a finite number


@pytest.mark.parametrize("n_couplings", [1, 2, 3])
def test_checker_edge_rows_have_the_documented_classes(oracle, n_couplings):
    flow, f, blob, eps = case(n_couplings, 64)
    x, _ = chk_sample(oracle, f, eps, 64)
    seen_finite_where_nan = False
    for value, j, row in edge_rows():
        e = eps[:, row:row + 1].copy()
        e[j] = value
        xx = x[:, row:row + 1].copy()
        xx[j] = value
        got_f, got_i = chk_sample(oracle, f, e, 1), chk_inverse(oracle, f, xx)
        assert_documented_classes(f, blob, value, e, xx, got_f, got_i)
        prop = classes(np.concatenate([np.ravel(a) for a in f64_sample(f, blob, e)]))
        seen_finite_where_nan |= bool(((classes(np.concatenate([np.ravel(a) for a in got_f])) != 3) & (prop == 3)).any())
    assert seen_finite_where_nan                                # the finding itself: fmaxf drops a NaN


def test_adam_checker_without_weight_decay_equals_torch_float64(oracle):
    """weight_decay == 0 is a branch of its own.  torch.optim.Adam in float64, step by step from the checker's float32 state (p,
    exp_avg, exp_avg_sq are written back before every step: what is held is one step's arithmetic, the tolerance form of
    test_nf_train.py::test_oracle_adam_equals_torch_adam covers one rounding of p and the float32 update)"""
    rng = np.random.default_rng(3)
    p0 = rng.standard_normal(3000).astype(np.float32)
    p = torch.nn.Parameter(torch.from_numpy(p0.astype(np.float64)))
    opt = torch.optim.Adam([p], lr=5e-4, weight_decay=0.0)
    q, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for step in range(1, 6):
        g = (rng.standard_normal(3000) * 10.0 ** rng.uniform(-6, 1, 3000)).astype(np.float32)
        if step > 1:
            with torch.no_grad():
                p.copy_(torch.from_numpy(q.astype(np.float64)))
                opt.state[p]["exp_avg"].copy_(torch.from_numpy(m.astype(np.float64)))
                opt.state[p]["exp_avg_sq"].copy_(torch.from_numpy(v.astype(np.float64)))
        p.grad = torch.from_numpy(g.astype(np.float64))
        opt.step()
        assert oracle.oracle_adam_step(q.ctypes.data, g.ctypes.data, m.ctypes.data, v.ctypes.data, q.size, 5e-4, 0.9, 0.999, 1e-8,
                                       0.0, step) == 0
        assert np.allclose(q, p.detach().numpy(), rtol=0, atol=2e-7 * 5e-4 + 1e-7 * np.abs(p0).max()), step
    assert np.abs(q - p0).max() > 1e-3                                    # it moved
    # the decay term is what separates the two branches: with zero state, exp_avg = (1 - beta1) g exactly without it
    outs = []
    for wd in (0.0, 1e-2):
        q2, m2, v2 = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
        assert oracle.oracle_adam_step(q2.ctypes.data, g.ctypes.data, m2.ctypes.data, v2.ctypes.data, q2.size, 5e-4, 0.9, 0.999,
                                       1e-8, wd, 1) == 0
        outs.append(m2)
    assert np.array_equal(bits(outs[0]), bits(g * np.float32(1.0 - 0.9))) and not np.array_equal(bits(outs[1]), bits(outs[0]))


GRAD_ROWS = (1, 31, 33, 127, 128, 129, 255, 256, 257, 65536, 65537)


def test_grad_workspace_size_never_shrinks(hip):
    """host-side call: bytes non-decreasing in n_rows and in n_couplings over the shapes of this module, and it holds what
    glabc_nf_grad carves (z, g, log_prob, trace and one parameter block per coupling and workgroup)"""
    need = C.c_int64()
    table = {}
    for nc in (1, 2, 3, 8, 32):
        for n in GRAD_ROWS + (4133, 70001):
            assert hip.glabc_nf_grad_workspace(nc, n, C.byref(need)) == 0
            table[nc, n] = need.value
            assert need.value >= 4 * (5 * n + nc * n) + 4 * nc * NC_FLOATS + 256 * 5 * 8
    for (nc, n), b in table.items():
        assert all(b <= b2 for (nc2, n2), b2 in table.items() if nc2 >= nc and n2 >= n), (nc, n)
    for nc, n in ((0, 10), (4097, 10), (1, 0), (1, -1)):
        need.value = -77
        assert hip.glabc_nf_grad_workspace(nc, n, C.byref(need)) == ERR_ARG and need.value == -77
    assert hip.glabc_nf_grad_workspace(1, 10, None) == ERR_NULL


# ---------------------------------------------------------------------------------------------------------------- GPU
NF_WAVES, NF_MAX_PAIRS, NF_CUS = 12, 5, 256


def nf_geometry(n):
    """nf_launch of glabc_nf.hip restated: (mode, rows per workgroup, state slots per wavefront)"""
    tiles = (n + 31) // 32
    if tiles <= 4 * NF_CUS:
        return "tile", 32 * ((tiles + NF_CUS - 1) // NF_CUS), 0
    pairs = (n + 63) // 64
    per = (pairs + NF_CUS - 1) // NF_CUS
    cap = NF_WAVES * NF_MAX_PAIRS
    if per > cap:
        rounds = (per + cap - 1) // cap
        per = (pairs + NF_CUS * rounds - 1) // (NF_CUS * rounds)
    return "pair", 64 * per, (per + NF_WAVES - 1) // NF_WAVES


def test_geometry_restatement_reaches_every_branch():
    assert [nf_geometry(n)[:2] for n in (1, 8192, 8193, 16385, 24577, 32768)] == [("tile", 32), ("tile", 32), ("tile", 64),
                                                                                 ("tile", 96), ("tile", 128), ("tile", 128)]
    assert nf_geometry(32769) == ("pair", 192, 1) and nf_geometry(49153) == ("pair", 256, 1)      # 3 / 4 pairs on 12 wavefronts
    assert nf_geometry(196608) == ("pair", 768, 1) and nf_geometry(196609) == ("pair", 832, 2)
    assert nf_geometry(983040) == ("pair", 3840, 5) and nf_geometry(983041) == ("pair", 1984, 3)  # 256 / 496 workgroups


class DevFlow:
    """a flow's blob on the device with its descriptor"""

    def __init__(self, flow):
        self.blob = flow.packed_params().cuda()
        self.f = flow.descriptor(self.blob)
        self.nc = self.f.n_couplings


def out_buffers(nc, n, trace=True):
    z, lq = dev(canary_f32(2 * n + TAIL)), dev(canary_f32(n + TAIL))
    tr = dev(canary_f32((nc + 1) * n + TAIL)) if trace else None
    return z, lq, tr


def split(buf, rows, n):
    """(the [rows][n] head the entry point owns -- rows = 0: a plain [n] -- and the canary behind it)"""
    a = host(buf)
    return a[:rows * n].reshape(rows, n) if rows else a[:n], a[max(rows, 1) * n:]


def hip_sample(hip, d, eps, n, seed=0, row0=0):
    z, lq, _ = out_buffers(d.nc, n, False)
    e = None if eps is None else dev(np.ascontiguousarray(eps, np.float32))
    assert hip.glabc_nf_sample(C.byref(d.f), None if e is None else e.data_ptr(), seed, row0, n, z.data_ptr(), lq.data_ptr(),
                               None) == 0
    (zz, zt), (ll, lt) = split(z, 2, n), split(lq, 0, n)
    assert_untouched(zt, lt)
    return zz, ll


def hip_log_prob(hip, d, x):
    n = x.shape[1]
    lq = dev(canary_f32(n + TAIL))
    xg = dev(np.ascontiguousarray(x, np.float32))
    assert hip.glabc_nf_log_prob(C.byref(d.f), xg.data_ptr(), n, lq.data_ptr(), None) == 0
    ll, lt = split(lq, 0, n)
    assert_untouched(lt)
    return ll


def hip_inverse(hip, d, x):
    n = x.shape[1]
    z, lq, tr = out_buffers(d.nc, n)
    xg = dev(np.ascontiguousarray(x, np.float32))
    assert hip.glabc_nf_inverse(C.byref(d.f), xg.data_ptr(), n, z.data_ptr(), lq.data_ptr(), tr.data_ptr(), None) == 0
    (zz, zt), (ll, lt), (tt, tail) = split(z, 2, n), split(lq, 0, n), split(tr, d.nc, n)
    assert_untouched(zt, lt, tail)                           # trace: the extra coupling's rows and the tail behind them
    return zz, ll, tt


def assert_kernels_equal_checker(hip, oracle, flow, f, eps, written=True):
    n = eps.shape[1]
    d = DevFlow(flow)
    z, lq = chk_sample(oracle, f, eps, n)
    zi, lp, tr = chk_inverse(oracle, f, z)
    zg, lqg = hip_sample(hip, d, eps, n)
    assert same(zg, z) and same(lqg, lq)
    lpg = hip_log_prob(hip, d, z)
    zig, lpg2, trg = hip_inverse(hip, d, z)
    assert same(lpg, lp) and same(lpg2, lp) and same(zig, zi) and same(trg, tr)
    if written:
        assert_written(zg, lqg, lpg, zig, lpg2, trg)
    return d, z, lq, zi, lp, tr


SMALL = (1, 31, 32, 33, 63, 64, 65, 8192, 8193)
LARGE = (16385, 24577, 32768, 32769, 49153, 196608, 196609)


@pytest.mark.gpu
@pytest.mark.parametrize("n_couplings,n", [(c, n) for n in SMALL for c in (1, 2, 3)] + [(2, n) for n in LARGE])
def test_kernels_equal_checker_at_every_launch_shape(hip, oracle, n_couplings, n):
    flow, f, blob, eps = case(n_couplings, n)
    assert_kernels_equal_checker(hip, oracle, flow, f, eps)


@pytest.mark.gpu
@pytest.mark.parametrize("n_couplings", [1, 2, 3, 8, 32])
def test_kernels_match_float64(hip, n_couplings):
    """RealNVP.sample, RealNVP.log_prob and glabc_nf_inverse against the float64 restatement directly (no checker in between)"""
    flow, f, blob, eps = case(n_couplings, F64_ROWS)
    g = copy.deepcopy(flow).cuda()
    z, lq = g.sample(F64_ROWS, eps=torch.from_numpy(eps.T.copy()))
    lp = g.log_prob(z)
    zh = np.ascontiguousarray(host(z).T)
    zi, lp2, tr = hip_inverse(hip, DevFlow(flow), zh)
    z64, lq64 = f64_sample(f, blob, eps)
    zi64, lp64, tr64 = f64_inverse(f, blob, zh)
    err = {"z": np.abs(zh - z64).max(), "log_q": np.abs(host(lq) - lq64).max(), "log_prob": np.abs(host(lp) - lp64).max(),
           "z_out": np.abs(zi - zi64).max(), "trace": np.abs(tr - tr64).max()}
    print("kernels vs float64, %d couplings: %s" % (n_couplings, ", ".join("%s %.3g" % kv for kv in err.items())))
    assert max(err.values()) <= F64_ATOL, err
    assert np.array_equal(bits(lp2), bits(host(lp)))


def large_subset(n):
    mode, rows_per_wg, slots = nf_geometry(n)
    starts = np.arange(0, n, rows_per_wg)
    edge = (starts[:, None] + np.concatenate([np.arange(64), np.arange(rows_per_wg - 64, rows_per_wg)])[None, :]).ravel()
    pick = np.concatenate([edge[edge < n], np.arange(n - 130, n), np.random.default_rng(n).integers(0, n, 20000)])
    return np.unique(pick)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [983040, 983041])
def test_largest_lds_grant_and_two_rounds_per_cu(hip, oracle, n):
    """983 040 rows: 60 pairs per workgroup, five state slots per wavefront; 983 041: two rounds of workgroups per CU.  The checker
    on the first and last 64 rows of every workgroup, the last 130 rows and 20 000 random rows (rows are independent: with the
    noise supplied a subset is the same function), and every row against the same rows through the kernel 8192 at a time, the
    form test_kernels_equal_checker_at_every_launch_shape pins."""
    flow, f, blob, eps = case(2, n)
    d = DevFlow(flow)
    zg, lqg = hip_sample(hip, d, eps, n)
    lpg = hip_log_prob(hip, d, zg)
    zig, lpg2, trg = hip_inverse(hip, d, zg)
    assert_written(zg, lqg, lpg, zig, lpg2, trg)
    assert np.array_equal(bits(lpg), bits(lpg2))
    sub = large_subset(n)
    assert len(sub) > 20000 and sub[-1] == n - 1 and sub[0] == 0
    e = np.ascontiguousarray(eps[:, sub])
    z, lq = chk_sample(oracle, f, e, len(sub))
    assert np.array_equal(bits(zg[:, sub]), bits(z)) and np.array_equal(bits(lqg[sub]), bits(lq))
    zi, lp, tr = chk_inverse(oracle, f, z)
    assert np.array_equal(bits(lpg[sub]), bits(lp)) and np.array_equal(bits(zig[:, sub]), bits(zi))
    assert np.array_equal(bits(trg[:, sub]), bits(tr))
    # every row: the same launch 8192 rows at a time
    eg, xg = dev(eps), dev(zg)
    zc, lqc = torch.empty(2, n, device="cuda"), torch.empty(n, device="cuda")
    zic, lpc, trc = torch.empty(2, n, device="cuda"), torch.empty(n, device="cuda"), torch.empty(2, n, device="cuda")
    for a in range(0, n, 8192):
        m = min(8192, n - a)
        ee, xx = eg[:, a:a + m].contiguous(), xg[:, a:a + m].contiguous()
        z1, l1 = torch.empty(2, m, device="cuda"), torch.empty(m, device="cuda")
        z2, l2, t2 = torch.empty(2, m, device="cuda"), torch.empty(m, device="cuda"), torch.empty(2, m, device="cuda")
        assert hip.glabc_nf_sample(C.byref(d.f), ee.data_ptr(), 0, 0, m, z1.data_ptr(), l1.data_ptr(), None) == 0
        assert hip.glabc_nf_inverse(C.byref(d.f), xx.data_ptr(), m, z2.data_ptr(), l2.data_ptr(), t2.data_ptr(), None) == 0
        zc[:, a:a + m], lqc[a:a + m], zic[:, a:a + m], lpc[a:a + m], trc[:, a:a + m] = z1, l1, z2, l2, t2
    for got, want in ((zg, zc), (lqg, lqc), (zig, zic), (lpg, lpc), (trg, trc)):
        assert np.array_equal(bits(got), bits(host(want)))


@pytest.mark.gpu
@pytest.mark.parametrize("n,row0", [(65, 2 ** 32 - 17), (32769, 2 ** 32 - 17), (32769, 2 ** 32 - 20000)])
def test_philox_row_counter_crosses_two_to_the_32(hip, oracle, n, row0):
    flow, f, blob, _ = case(2, n)
    z, lq = chk_sample(oracle, f, None, n, seed=77, row0=row0)
    zg, lqg = hip_sample(hip, DevFlow(flow), None, n, seed=77, row0=row0)
    assert np.array_equal(bits(zg), bits(z)) and np.array_equal(bits(lqg), bits(lq))
    assert_written(zg, lqg)
    # the rows on either side of the crossing are different draws, and the high word matters
    k = 2 ** 32 - row0
    assert len(np.unique(bits(z[0, k - 3:k + 3]))) == 6
    z_low, _ = chk_sample(oracle, f, None, 8, seed=77, row0=0)             # the same low word, high word 0
    assert not (bits(z_low) == bits(z[:, k:k + 8])).any()


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [1, 5, 12])
def test_tile_waves_knob_equals_checker(hip, oracle, monkeypatch, waves):
    n = 3 * 32 * waves + 7
    flow, f, blob, eps = case(2, n)
    monkeypatch.setenv("GLABC_NF_TILE_WAVES", str(waves))
    assert_kernels_equal_checker(hip, oracle, flow, f, eps)


@pytest.mark.gpu
@pytest.mark.parametrize("value", ["0", "13"])
def test_tile_waves_knob_out_of_range_is_the_default_geometry(hip, oracle, monkeypatch, value):
    n = 3 * 32 * 5 + 7
    flow, f, blob, eps = case(2, n)
    monkeypatch.delenv("GLABC_NF_TILE_WAVES", raising=False)
    d = DevFlow(flow)
    z0, lq0 = hip_sample(hip, d, eps, n)
    i0 = hip_inverse(hip, d, z0)
    monkeypatch.setenv("GLABC_NF_TILE_WAVES", value)
    d, z, lq, zi, lp, tr = assert_kernels_equal_checker(hip, oracle, flow, f, eps)
    assert np.array_equal(bits(z0), bits(z)) and np.array_equal(bits(lq0), bits(lq))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(i0, (zi, lp, tr)))


# ---- indexed log-prob
MAX_ROWS = 300


def index_list(count, rng):
    """shuffled; from three entries on it holds chains 0 and 299 and one repeat.  Entries past `count` name chain 150, which no
    list holds: a kernel that read them would write log_q[150]."""
    idx = np.full(MAX_ROWS, 150, np.int32)
    if count == 1:
        idx[0] = 299
    elif count >= 3:
        others = rng.permutation(np.setdiff1d(np.arange(1, 299), [150]))[:count - 3]
        lst = np.concatenate([[0, 299], others]).astype(np.int32)
        lst = np.concatenate([lst, lst[-1:]])                     # the repeat
        idx[:count] = rng.permutation(lst)
        assert len(lst) == count and len(np.unique(lst)) == count - 1
    return idx


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [300, 311])
def test_indexed_log_prob_at_every_count(hip, oracle, stride):
    flow, f, blob, _ = case(3, MAX_ROWS)
    d = DevFlow(flow)
    rng = np.random.default_rng(stride)
    theta = np.full((2, stride), np.nan, np.float32)
    theta[:, :MAX_ROWS] = rng.standard_normal((2, MAX_ROWS)) * 1.3
    want_all = chk_log_prob(oracle, f, theta[:, :MAX_ROWS])
    tg = dev(theta)
    n_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    for count in (0, 1, 31, 32, 33, 299, 300):
        idx = index_list(count, rng)
        before = np.concatenate([rng.standard_normal(MAX_ROWS).astype(np.float32), canary_f32(TAIL)])
        lq, ig = dev(before), dev(idx)
        n_dev.fill_(count)
        assert hip.glabc_nf_log_prob_indexed(C.byref(d.f), tg.data_ptr(), stride, ig.data_ptr(), n_dev.data_ptr(), MAX_ROWS,
                                             lq.data_ptr(), None) == 0
        got = host(lq)
        listed = np.zeros(MAX_ROWS + TAIL, bool)
        listed[idx[:count]] = True
        assert listed.sum() == max(count - 1, 0) + (count == 1) and not listed[150]
        assert np.array_equal(bits(got[:MAX_ROWS][listed[:MAX_ROWS]]), bits(want_all[listed[:MAX_ROWS]])), count
        assert np.array_equal(bits(got[~listed]), bits(before[~listed])), count
        # the count is read on the device: the same host arguments, another count
        other = 5 if count != 5 else 7
        lq2 = dev(before)
        n_dev.fill_(other)
        assert hip.glabc_nf_log_prob_indexed(C.byref(d.f), tg.data_ptr(), stride, ig.data_ptr(), n_dev.data_ptr(), MAX_ROWS,
                                             lq2.data_ptr(), None) == 0
        got2 = host(lq2)
        listed2 = np.zeros(MAX_ROWS + TAIL, bool)
        listed2[idx[:other]] = True
        assert np.array_equal(bits(got2[:MAX_ROWS][listed2[:MAX_ROWS]]), bits(want_all[listed2[:MAX_ROWS]])), count
        assert np.array_equal(bits(got2[~listed2]), bits(before[~listed2])), count


@pytest.mark.gpu
def test_indexed_log_prob_refusals(hip):
    flow, f, blob, _ = case(3, MAX_ROWS)
    d = DevFlow(flow)
    theta, idx = dev(np.zeros((2, 311), np.float32)), dev(np.arange(MAX_ROWS, dtype=np.int32))
    n_dev = torch.full((1,), 300, dtype=torch.int32, device="cuda")
    lq = dev(canary_f32(MAX_ROWS + TAIL))

    def call(flow_d=d.f, th=theta.data_ptr(), stride=311, ix=idx.data_ptr(), nd=n_dev.data_ptr(), rows=MAX_ROWS, out=lq.data_ptr()):
        return hip.glabc_nf_log_prob_indexed(C.byref(flow_d) if flow_d is not None else None, th, stride, ix, nd, rows, out, None)

    assert call(stride=299) == ERR_ARG
    no_params = DevFlow(flow).f
    no_params.params = None
    assert call(flow_d=None) == ERR_NULL and call(flow_d=no_params) == ERR_NULL
    assert call(th=None) == ERR_NULL and call(ix=None) == ERR_NULL and call(nd=None) == ERR_NULL and call(out=None) == ERR_NULL
    assert call(rows=0, stride=0) == 0 and call(rows=-1) == ERR_ARG
    assert_untouched(host(lq))


# ---- edge rows inside a shared tile
@pytest.mark.gpu
@pytest.mark.parametrize("n", [64, 32769])
def test_edge_row_leaves_its_tile_alone(hip, oracle, n):
    """one row of the first 64 carries NaN, +-Inf, +-1e30, a denormal or +-0 in one coordinate: the other rows keep the bits of
    the run without it, the row itself has the checker's bits and the documented classes"""
    assert nf_geometry(n)[0] == ("tile" if n == 64 else "pair")
    flow, f, blob, eps = case(2, n)
    d, x, lq, zi, lp, tr = assert_kernels_equal_checker(hip, oracle, flow, f, eps)
    for value, j, row in edge_rows():
        e, xx = eps.copy(), x.copy()
        e[j, row], xx[j, row] = value, value
        others = np.arange(n) != row
        zg, lqg = hip_sample(hip, d, e, n)
        zig, lpg, trg = hip_inverse(hip, d, xx)
        assert np.array_equal(bits(hip_log_prob(hip, d, xx)[others]), bits(lp[others]))
        for got, base in ((zg, x), (lqg, lq), (zig, zi), (lpg, lp), (trg, tr)):
            assert np.array_equal(bits(got[..., others]), bits(base[..., others])), (value, j, row)
        one = slice(row, row + 1)
        want_f, want_i = chk_sample(oracle, f, e[:, one], 1), chk_inverse(oracle, f, xx[:, one])
        got_f, got_i = (zg[:, one], lqg[one]), (zig[:, one], lpg[one], trg[:, one])
        assert all(same(a, b) for a, b in zip(got_f + got_i, want_f + want_i)), (value, j, row)
        assert_documented_classes(f, blob, value, e[:, one], xx[:, one], got_f, got_i)


@pytest.mark.gpu
@pytest.mark.parametrize("n_couplings,n", [(2, 4096 + 33), (3, 32769 + 64)])
def test_extreme_scale_equals_checker_infinities_included(hip, oracle, n_couplings, n):
    """make_flow(scale=30): exp(log_s) overflows for some rows and underflows for others"""
    flow, f, blob, eps = case(n_couplings, n, scale=30.0)
    d, z, lq, zi, lp, tr = assert_kernels_equal_checker(hip, oracle, flow, f, eps)
    assert np.isinf(z).any() and np.isfinite(z).all(0).any() and (np.isinf(lp) | np.isnan(lp)).any() and np.isfinite(lp).any()
    assert (zi[1] == 0).any() or np.isinf(zi).any()


# ---- refusals
def bad_flow(d, **kw):
    f = A.Flow.from_buffer_copy(d.f)
    for k, v in kw.items():
        if k in ("base_loc", "base_log_scale", "base_scale"):
            getattr(f, k)[1] = v
        else:
            setattr(f, k, v)
    return f


@pytest.mark.gpu
def test_refusals_launch_nothing(hip):
    flow, f, blob, eps = case(2, 64)
    d = DevFlow(flow)
    n = 64
    z, lq, tr = out_buffers(d.nc, n)
    io = dev(eps)

    def calls(fl, inp=io.data_ptr(), rows=n, zz=z.data_ptr(), ll=lq.data_ptr(), which=(0, 1, 2)):
        fp = C.byref(fl) if fl is not None else None
        fns = (lambda: hip.glabc_nf_sample(fp, inp, 0, 0, rows, zz, ll, None),
               lambda: hip.glabc_nf_log_prob(fp, inp, rows, ll, None),
               lambda: hip.glabc_nf_inverse(fp, inp, rows, zz, ll, tr.data_ptr(), None))
        return tuple(fns[k]() for k in which)

    for kw in (dict(n_couplings=0), dict(n_couplings=4097), dict(hidden=64), dict(base_scale=0.0), dict(base_scale=-1.0),
               dict(base_loc=float("nan")), dict(base_loc=float("inf")), dict(base_log_scale=float("-inf")),
               dict(base_log_scale=float("nan"))):
        assert calls(bad_flow(d, **kw)) == (ERR_ARG,) * 3, kw
    assert calls(d.f, rows=-1) == (ERR_ARG,) * 3
    assert calls(None) == (ERR_NULL,) * 3 and calls(bad_flow(d, params=None)) == (ERR_NULL,) * 3
    assert calls(d.f, ll=None) == (ERR_NULL,) * 3
    assert calls(d.f, zz=None, which=(0, 2)) == (ERR_NULL,) * 2                # (log_prob has no z_out)
    assert calls(d.f, inp=None, which=(1, 2)) == (ERR_NULL,) * 2               # (sample without eps draws its own noise)
    # every call so far was refused: nothing ran, every output and the tail behind it holds its canary
    assert_untouched(host(z), host(lq), host(tr))
    assert calls(d.f, rows=0) == (0, 0, 0)
    assert_untouched(host(z), host(lq), host(tr))
    # and the same buffers are written by the calls that are not refused (the canaries above could have been overwritten)
    assert calls(d.f) == (0, 0, 0)
    (zz, zt), (ll, lt), (tt, tail) = split(z, 2, n), split(lq, 0, n), split(tr, d.nc, n)
    assert_written(zz, ll, tt)
    assert_untouched(zt, lt, tail)


@pytest.mark.gpu
def test_python_surface_empty_and_strided_inputs(hip):
    flow, f, blob, eps = case(2, 65)
    g = copy.deepcopy(flow).cuda()
    z, lq = g.sample(0)
    assert tuple(z.shape) == (0, 2) and tuple(lq.shape) == (0,) and z.dtype == lq.dtype == torch.float32
    lp = g.log_prob(torch.empty(0, 2, device="cuda"))
    assert tuple(lp.shape) == (0,) and lp.dtype == torch.float32
    x32 = torch.from_numpy(eps.T.copy()).cuda()                                # (65, 2) float32, contiguous
    wide = torch.zeros(65, 5, dtype=torch.float64, device="cuda")
    wide[:, 1::3] = x32.double()
    x64 = wide[:, 1::3]                                                        # (65, 2) float64, strides (5, 3)
    assert not x64.is_contiguous() and tuple(x64.shape) == (65, 2)
    assert torch.equal(g.log_prob(x64).view(torch.int32), g.log_prob(x32).view(torch.int32))


# ---- training kernels
@pytest.mark.gpu
@pytest.mark.parametrize("n_couplings,n", [(c, n) for n in (1, 31, 33, 255, 256, 257) for c in (1, 2)] + [(1, 65536), (1, 65537)])
def test_gradient_at_every_batch_boundary(hip, oracle, n_couplings, n):
    flow = trained_looking_flow(n_couplings, 11 + n_couplings)
    x = torch.randn(n, 2, generator=torch.Generator().manual_seed(n)) * 1.3
    loss_o, gp, gb = oracle_gradient(oracle, flow, x)
    loss_h, gph, gbh, opt = hip_gradient(flow.cuda(), x)
    assert abs(loss_h - loss_o) <= 2e-6 * abs(loss_o), (loss_h, loss_o)
    assert_close(gph, gp, 2e-4, "hip vs checker")                             # (its "pad" section: the padding entries are zero)
    assert np.allclose(gbh, gb, rtol=2e-4, atol=2e-6)
    loss2, gp2, gb2 = opt.gradient(x.cuda())
    torch.cuda.synchronize()
    assert np.array_equal(bits(gp2.cpu().numpy()), bits(gph)) and np.array_equal(bits(gb2.cpu().numpy()), bits(gbh))
    assert float(loss2) == loss_h


def raw_grad(hip, d, x_cm, ws_bytes=None, short=0):
    """glabc_nf_grad on a workspace of exactly the advertised size (minus `short`) with a 4 KiB canary behind it"""
    n = x_cm.shape[1]
    need = C.c_int64()
    assert hip.glabc_nf_grad_workspace(d.nc, n, C.byref(need)) == 0
    size = need.value - short
    ws = torch.full((size + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    gp, gb, loss = dev(canary_f32(d.nc * NC_FLOATS + TAIL)), dev(canary_f32(4 + TAIL)), dev(canary_f32(1 + TAIL))
    xg = dev(np.ascontiguousarray(x_cm, np.float32))
    rc = hip.glabc_nf_grad(C.byref(d.f), xg.data_ptr(), n, ws.data_ptr(), size, gp.data_ptr(), gb.data_ptr(), loss.data_ptr(), None)
    torch.cuda.synchronize()
    assert bool((ws[size:] == 0xA5).all()), "glabc_nf_grad wrote behind its workspace"
    return rc, host(gp), host(gb), host(loss)


@pytest.mark.gpu
@pytest.mark.parametrize("n_couplings,n", [(2, 257), (1, 65537), (3, 129)])
def test_grad_workspace_is_exactly_enough(hip, oracle, n_couplings, n):
    """(also run by test_nf_train.py::test_hip_gradient_other_kernel_forms under GLABC_NF_BW=1 and 4: the workspace is carved
    with one geometry and used with the kernel form's own, which must never need more)"""
    flow = trained_looking_flow(n_couplings, 11 + n_couplings)
    x = torch.randn(n, 2, generator=torch.Generator().manual_seed(n)) * 1.3
    d = DevFlow(flow)
    x_cm = x.numpy().T
    rc, gp, gb, loss = raw_grad(hip, d, x_cm)
    assert rc == 0
    total = n_couplings * NC_FLOATS
    assert_untouched(gp[total:], gb[4:], loss[1:])
    assert_written(gp[:total], gb[:4], loss[:1])
    loss_o, gpo, gbo = oracle_gradient(oracle, flow, x)
    assert abs(float(loss[0]) - loss_o) <= 2e-6 * abs(loss_o)
    assert_close(gp[:total].reshape(n_couplings, NC_FLOATS), gpo, 2e-4, "hip vs checker")
    assert np.allclose(gb[:4], gbo, rtol=2e-4, atol=2e-6)
    rc, gp, gb, loss = raw_grad(hip, d, x_cm, short=1)
    assert rc == ERR_ARG
    assert_untouched(gp, gb, loss)


@pytest.mark.gpu
def test_grad_refusals_launch_nothing(hip):
    flow = trained_looking_flow(2, 13)
    d = DevFlow(flow)
    n = 33
    need = C.c_int64()
    assert hip.glabc_nf_grad_workspace(2, n, C.byref(need)) == 0
    ws = torch.zeros(need.value, dtype=torch.uint8, device="cuda")
    gp, gb, loss = dev(canary_f32(2 * NC_FLOATS)), dev(canary_f32(4)), dev(canary_f32(1))
    xg = dev(np.zeros((2, n), np.float32))

    def call(fl=d.f, x=xg.data_ptr(), rows=n, w=ws.data_ptr(), g=gp.data_ptr(), b=gb.data_ptr(), l=loss.data_ptr()):
        return hip.glabc_nf_grad(C.byref(fl) if fl is not None else None, x, rows, w, need.value, g, b, l, None)

    assert call(rows=0) == ERR_ARG and call(rows=-1) == ERR_ARG
    assert call(fl=bad_flow(d, n_couplings=0)) == ERR_ARG and call(fl=bad_flow(d, n_couplings=4097)) == ERR_ARG
    assert call(fl=bad_flow(d, hidden=64)) == ERR_ARG
    assert call(fl=None) == ERR_NULL and call(fl=bad_flow(d, params=None)) == ERR_NULL
    for k in ("x", "w", "g", "b", "l"):
        assert call(**{k: None}) == ERR_NULL, k
    assert_untouched(host(gp), host(gb), host(loss))
    assert not bool(ws.any())


@pytest.mark.gpu
def test_hipadam_reuses_the_larger_workspace(hip):
    from glabcmcmc_amd.flows import HipAdam
    flow = trained_looking_flow(2, 13).cuda()
    gen = torch.Generator().manual_seed(8)
    big, small = torch.randn(4133, 2, generator=gen) * 1.3, torch.randn(33, 2, generator=gen) * 1.3
    alone = [t.clone() for t in HipAdam(flow).gradient(small)]
    opt = HipAdam(flow)
    opt.gradient(big)
    ws = opt._ws
    got = opt.gradient(small)
    torch.cuda.synchronize()
    assert opt._ws is ws
    need = C.c_int64()
    assert hip.glabc_nf_grad_workspace(2, 33, C.byref(need)) == 0 and need.value < ws.numel()
    for a, b in zip(got, alone):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def zero_gate_flow(n_couplings, zeroed):
    """zeroed = "b1": the issue's case -- rows with a conditioner input of +-0 have every first-layer pre-activation +-0, while
    the second layer's (= b2) are not, so dh1 is non-zero and only the first-layer gate keeps db1 at 0.  zeroed = "b1b2": the
    second layer's pre-activations of those rows are +-0 as well, so its gate is what keeps db2 at 0."""
    flow = trained_looking_flow(n_couplings, 17 + n_couplings)
    with torch.no_grad():
        for c in flow.couplings:
            c.l1.bias.zero_()
            if zeroed == "b1b2":
                c.l2.bias.zero_()
    return flow


def zero_gate_batches(n_regular, n_zero):
    gen = torch.Generator().manual_seed(n_regular)
    reg = torch.randn(n_regular, 2, generator=gen) * 1.3
    z = torch.randn(n_zero, 2, generator=gen) * 1.3
    z[:, 1] = 0.0                                              # the conditioner input of the coupling undone first
    z[::2, 1] = -0.0
    both = torch.cat([reg, z])[torch.randperm(n_regular + n_zero, generator=gen)]
    return reg, both


# the tensors to which rows with every gate of the named layers shut contribute exactly 0 (h1 = 0: dW2 = da2 h1^T = 0 either way)
GATED = {"b1": ("W1", "b1", "W2"), "b1b2": ("W1", "b1", "W2", "b2", "W3")}
OPEN = {"b1": ("b2", "W3", "b3"), "b1b2": ("b3",)}


@pytest.mark.parametrize("zeroed", ["b1", "b1b2"])
def test_checker_gates_at_zero_are_shut_like_autograd(oracle, zeroed):
    """a conditioner input of +-0 with b1 = 0 (and b2 = 0): pre-activations of exactly +-0; relu'(0) = 0 in torch"""
    for nc in (1, 2):
        flow = zero_gate_flow(nc, zeroed)
        reg, both = zero_gate_batches(90, 70)
        loss_o, gp, gb = oracle_gradient(oracle, flow, both)
        loss_t, gpt, gbt = autograd_gradient(flow, both, torch.float64)
        assert abs(loss_o - loss_t) <= 2e-6 * abs(loss_t)
        assert_close(gp, gpt.numpy(), 2e-6, "checker vs autograd f64, gates at zero")
        only_zero = both[both[:, 1] == 0]
        assert len(only_zero) == 70
        _, gz, _ = oracle_gradient(oracle, flow, only_zero)
        _, gzt, _ = autograd_gradient(flow, only_zero, torch.float64)
        for name in GATED[zeroed]:
            assert not sections(gz)[name][nc - 1].any(), name            # exactly 0 from rows whose gates are shut
            assert not sections(gzt.numpy())[name][nc - 1].any(), name   # ... as in autograd
        for name in OPEN[zeroed]:
            assert sections(gz)[name][nc - 1].any(), name                # (the gradient does reach the layer behind the gate)


@pytest.mark.gpu
@pytest.mark.parametrize("zeroed", ["b1", "b1b2"])
@pytest.mark.parametrize("n_couplings", [1, 2])
def test_gate_exactly_at_zero_is_shut(hip, oracle, n_couplings, zeroed):
    flow = zero_gate_flow(n_couplings, zeroed)
    gflow = copy.deepcopy(flow).cuda()
    last = n_couplings - 1                                    # log_prob undoes the last coupling first: it sees x[:, 1]
    reg, both = zero_gate_batches(300, 213)
    only_zero = both[both[:, 1] == 0]
    loss_h, gz, _, _ = hip_gradient(gflow, only_zero)
    for name in GATED[zeroed]:
        assert not sections(gz)[name][last].any(), name       # exactly 0: no gate of these rows is open
    for name in OPEN[zeroed]:
        assert sections(gz)[name][last].any(), name           # with b1 = 0 alone dh1 is not 0: only the gate keeps db1 at 0
    loss_o, gp, gb = oracle_gradient(oracle, flow, both)
    loss_b, gpb, gbb, _ = hip_gradient(gflow, both)
    assert abs(loss_b - loss_o) <= 2e-6 * abs(loss_o)
    assert_close(gpb, gp, 2e-4, "hip vs checker, gates at zero")
    loss_t, gpt, gbt = autograd_gradient(flow, both, torch.float64)
    assert_close(gpb, gpt.numpy(), 2e-4, "hip vs autograd f64, gates at zero")
    # the batch without those rows, scaled by the row counts (the loss is a mean)
    _, gpr, _, _ = hip_gradient(gflow, reg)
    for name in GATED[zeroed]:
        a, b = sections(gpb)[name][last] * float(len(both)), sections(gpr)[name][last] * float(len(reg))
        assert np.abs(a - b).max() <= 2e-4 * np.abs(b).max(), name


# ---- Adam
def adam_inputs(count, rng):
    p = rng.standard_normal(count).astype(np.float32)
    g = (rng.standard_normal(count) * 10.0 ** rng.uniform(-30, 30, count)).astype(np.float32)
    m = (rng.standard_normal(count) * 1e-2).astype(np.float32)
    v = (rng.uniform(0, 1, count) * 1e-3).astype(np.float32)
    special = {}
    if count >= 255:
        special = {3: 0.0, 100: np.inf, 101: -np.inf, 200: np.nan, 254: 0.0}
        for j, val in special.items():
            g[j] = val
        m[3] = v[3] = 0.0                                                      # an exact 0 gradient with zero state
        m[254] = v[254] = 0.0
        g[[10, 11]] = [1e-30, 1e30]
    elif count == 1:
        g[0] = 0.0
        m[0] = v[0] = 0.0
    return p, g, m, v


@pytest.mark.gpu
@pytest.mark.parametrize("weight_decay", [0.0, 1e-5])
@pytest.mark.parametrize("count", [0, 1, 255, 256, 257])
def test_adam_equals_checker_at_every_count(hip, oracle, count, weight_decay):
    rng = np.random.default_rng(count)
    p, g, m, v = adam_inputs(count, rng)
    for step in (1, 2, 1000000):
        tail = canary_f32(TAIL)
        dp, dm, dv = (dev(np.concatenate([a, tail])) for a in (p, m, v))
        dg = dev(np.concatenate([g, tail]))
        q, qm, qv = p.copy(), m.copy(), v.copy()
        assert hip.glabc_adam_step(dp.data_ptr(), dg.data_ptr(), dm.data_ptr(), dv.data_ptr(), count, 5e-4, 0.9, 0.999, 1e-8,
                                   weight_decay, step, None) == 0
        assert oracle.oracle_adam_step(q.ctypes.data, g.ctypes.data, qm.ctypes.data, qv.ctypes.data, count, 5e-4, 0.9, 0.999, 1e-8,
                                       weight_decay, step) == 0
        for got, want, what in ((dp, q, "p"), (dm, qm, "m"), (dv, qv, "v")):
            got = host(got)
            assert same(got[:count], want), (what, step)
            assert_untouched(got[count:])
        assert same(host(dg)[:count], g)
        if count >= 255:
            assert np.isnan(q[[100, 101, 200]]).all() and np.isfinite(np.delete(q, [100, 101, 200])).all()
            assert q[3] == p[3] if weight_decay == 0.0 else q[3] != p[3]      # zero gradient, zero state: only the decay moves it
        if step == 1000000:
            assert np.float32(5e-4 / (1.0 - 0.9 ** step)) == np.float32(5e-4)  # both bias corrections are 1
        p, m, v = q, qm, qv
        p[~np.isfinite(p)] = 0.5                                               # keep later steps informative
        m[~np.isfinite(m)] = 0.0
        v[~np.isfinite(v)] = 0.0


@pytest.mark.gpu
def test_adam_refusals_write_nothing(hip):
    arrays = [dev(canary_f32(64)) for _ in range(4)]
    ptrs = [a.data_ptr() for a in arrays]

    def call(p=ptrs, count=64, lr=5e-4, b1=0.9, b2=0.999, eps=1e-8, wd=1e-5, step=1):
        return hip.glabc_adam_step(p[0], p[1], p[2], p[3], count, lr, b1, b2, eps, wd, step, None)

    assert call(step=0) == ERR_ARG and call(step=-1) == ERR_ARG and call(count=-1) == ERR_ARG
    assert call(b1=1.0) == ERR_ARG and call(b2=1.0) == ERR_ARG and call(b1=1.5) == ERR_ARG
    assert call(lr=-1e-3) == ERR_ARG and call(eps=-1e-8) == ERR_ARG and call(wd=-1e-5) == ERR_ARG
    assert call(lr=float("nan")) == ERR_ARG
    for k in range(4):
        assert call(p=[None if j == k else q for j, q in enumerate(ptrs)]) == ERR_NULL
    assert call(count=0) == 0
    assert_untouched(*[host(a) for a in arrays])
