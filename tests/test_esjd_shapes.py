"""glabc_esjd and glabc_moments_esjd (ESJD.py:2-25) at every theta_dim 1 .. 8, against a float64 reference.

The reference is exp(slogdet(D^T D / (n_rows - 1)) / d) in float64 NumPy, D = the float32 consecutive differences of the
history widened to float64 (ESJD.py:17 forms them in float32).  It shares no code with oracle/ or csrc/.

CPU: the checker (oracle_esjd, float32 throughout, the only ESJD the rest of the suite trusts) against that reference, and
the conditions that keep the GPU part honest: at d >= 2 a third or more of the chains need a row exchange in the first
column of the elimination, every matrix used for a tolerance comparison has a float64 condition number of at most 200, and
no launch is all zeros.  GPU: both kernels against the reference and against each other at 1, 63, 64, 65 and 321 chains
(BLOCK = 64: a ragged last workgroup), with stride == n_chains and with 17 padding columns that hold NaN; the Python
surface; the cases whose sums are exact; every refusal.

Inputs (esjd_histories): float64 jumps, positions rounded to float32 once.  Every coordinate has its own scale, the scales
span 2^-1 .. 2^1.5; in units of its scale coordinate j >= 1 follows coordinate j - 1 with a weight of 0.5 .. 0.8 (0.9 would
pass the condition cap at d = 2 already: 34 / (1 - 0.81) = 179 before sampling noise).  About 30 % of the steps are rejected
(a zero jump).  The history lists the smallest coordinate first and the largest, which follows it, second:
|M[1][0]| = rho s0 s1 > s0^2 = |M[0][0]|, so the elimination has to exchange rows 0 and 1; every other chain lists that pair
the other way round and needs no exchange.  n_rows = 48 d + (0 .. 16): 48 .. 400.

Tolerance.  ESJD_RTOL is four times the largest relative difference between oracle_esjd and the float64 reference over
this module's own inputs, measured on the CPU (test_checker_matches_float64 re-measures it and holds it below 2e-5, the
bound tests/test_hip_parity.py::test_esjd_kernel had).  The kernels accumulate D^T D in double and get the same bound:
the factor 4 is for their different elimination order (they bubble the exchanges, the checker picks the largest pivot),
not for conditioning, which the cap of 200 controls.
Measured: checker on the CPU 1.3e-6 (at d = 2; 8.6e-7 .. 1.1e-6 at d = 3 .. 8, 3.0e-7 at d = 1; 514 chains each);
esjd_kernel and moments_esjd_kernel on the MI355X 2.6e-7 (at d = 3; 9.2e-8 at d = 1), and 0 against each other.

Exact cases: jumps that are powers of two, one coordinate moving at a time, 16 difference rows, so that every sum, the
division by n_rows - 1 and (d <= 2) the root are exact.  For d >= 3 the root goes through exp(log(det) / d) with
det = 2 or 4: |log det| < 2, so the logarithm's ulp is at most 2^-23, divided by d >= 3, plus half an ulp of the quotient,
plus the exponential's own ulp -- under 2 ulp of the result; the tests allow EXACT_ULPS = 4.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from glabcmcmc_amd import _capi as A
from helpers import assert_untouched, assert_written, bits, canary_f32, canary_f64, dev, host

ERR_NULL, ERR_DIM, ERR_ARG = -1, -2, -4          # glabc_status, include/glabc.h

DIMS = range(1, 9)
CHAINS = (1, 63, 64, 65, 321)
PAD = 17
TAIL = 5                                          # canary elements behind the n_chains outputs

# 4 x the checker's largest relative error against the float64 reference over esjd_histories(d, n), d = 1 .. 8, n in CHAINS:
# measured 1.3e-6 on the CPU (x86-64, glibc powf).  The kernels on the MI355X: 2.6e-7, both.
ESJD_RTOL = 4 * 1.3e-6
COND_CAP = 200.0
EXACT_ULPS = 4


# ---------------------------------------------------------------------------------- inputs and the float64 reference
@functools.lru_cache(maxsize=None)
def esjd_histories(d, n_chains, seed=0):
    """float32 history [n_rows][d][n_chains] (chain-major, as the samplers write it); read-only"""
    rng = np.random.default_rng([seed, d, n_chains])
    n_rows = 48 * d + int(rng.integers(0, 17))
    ex = np.linspace(-1.0, 1.5, d) if d > 1 else np.array([0.5])
    if d > 2:                                      # the smallest scale first, the largest second, the others ascending
        ex = np.concatenate([[ex[0], ex[-1]], ex[1:-1]])
    rho = rng.uniform(0.5, 0.8, (n_chains, d))
    z = rng.standard_normal((n_rows - 1, n_chains, d))
    unit = np.empty_like(z)                        # unit-variance coordinates, each following the one before it
    unit[..., 0] = z[..., 0]
    for j in range(1, d):
        unit[..., j] = rho[:, j] * unit[..., j - 1] + np.sqrt(1 - rho[:, j] ** 2) * z[..., j]
    jump = unit * 2.0 ** ex
    jump *= rng.random((n_rows - 1, n_chains, 1)) >= 0.3                   # rejected steps
    if d > 1:                                      # every other chain: the large coordinate first -- no exchange there
        flip = np.arange(n_chains) % 2 == 1
        jump[:, flip] = jump[:, flip][:, :, [1, 0] + list(range(2, d))]
    pos = np.concatenate([rng.standard_normal((1, n_chains, d)), jump], 0).cumsum(0)
    hist = np.ascontiguousarray(pos.astype(np.float32).transpose(0, 2, 1))
    hist.setflags(write=False)
    return hist


def jump_matrices(hist):
    """D^T D in float64 from the float32 differences, [n_chains][d][d]"""
    diff = np.diff(np.asarray(hist), axis=0)
    assert diff.dtype == np.float32
    diff = diff.astype(np.float64)
    return np.einsum("tpc,tqc->cpq", diff, diff)


def esjd_reference(hist):
    """-> (esjd float64 [n_chains], M = D^T D / (n_rows - 1))"""
    n_rows, d, _ = hist.shape
    m = jump_matrices(hist) / (n_rows - 1)
    sign, logdet = np.linalg.slogdet(m)
    with np.errstate(over="ignore"):
        return np.where(sign > 0, np.exp(logdet / d), 0.0), m


@functools.lru_cache(maxsize=None)
def case(d, n):
    hist = esjd_histories(d, n)
    ref, m = esjd_reference(hist)
    ref.setflags(write=False)
    m.setflags(write=False)
    return hist, ref, m


def padded(hist, pad):
    """the same chains with `pad` columns of NaN behind them (stride = n_chains + pad)"""
    n_rows, d, n = hist.shape
    out = np.full((n_rows, d, n + pad), np.nan, np.float32)
    out[:, :, :n] = hist
    return out


def tri_rows(mats, stride):
    """glabc_moments.sum_jump: row-major upper triangle, [tri(d)][stride] float64, canaries in the padding"""
    n, d, _ = mats.shape
    out = canary_f64(d * (d + 1) // 2, stride)
    k = 0
    for p in range(d):
        for q in range(p, d):
            out[k, :n] = mats[:, p, q]
            k += 1
    return out


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all() and (ref > 0).all()
    return float(np.max(np.abs(got - ref) / ref))


def oracle_esjd(oracle, hist, n=None):
    n_rows, d, stride = hist.shape
    n = stride if n is None else n
    hist = np.ascontiguousarray(hist)
    out = canary_f32(n + TAIL)
    assert oracle.oracle_esjd(hist.ctypes.data, n_rows, d, n, stride, out.ctypes.data) == 0
    assert_written(out[:n])
    assert_untouched(out[n:])
    return out[:n]


# ---------------------------------------------------------------------------------- exact cases
def exact_history(d, kind):
    """(history [17][d][1], expected float64) with power-of-two jumps, one coordinate at a time"""
    pos = np.full((17, d), 0.5)
    if kind == "still":
        return pos.astype(np.float32)[:, :, None], 0.0
    if kind.startswith("one"):                     # only coordinate j moves: singular for d >= 2
        j = int(kind[3:])
        pos[1::2, j] += 0.25                       # sixteen jumps of +-1/4: mean square 1/16
        return pos.astype(np.float32)[:, :, None], 0.0625 if d == 1 else 0.0
    assert kind == "independent"
    e = [(j % 4) - 1 for j in range(d)]
    e[0] += (3 * d) // 2 + 1 - sum(e)              # det = prod(2 s_j^2 / 16) = 2^(2 sum(e) - 3 d) = 2 (odd d) or 4 (even d)
    jumps = np.zeros((16, d))
    for j in range(d):                             # coordinate j moves at rows 2j and 2j + 1: there and back
        jumps[2 * j, j] = 2.0 ** e[j]
        jumps[2 * j + 1, j] = -(2.0 ** e[j])
    pos[1:] += jumps.cumsum(0)
    return pos.astype(np.float32)[:, :, None], 2.0 ** ((2 * sum(e) - 3 * d) / d)


def exact_kinds(d):
    return ["still", "independent"] + ["one%d" % j for j in range(d)]


def assert_exact(got, want, d, what):
    got = float(got)
    if d <= 2 or want == 0.0:
        assert got == want, (what, d, got, want)
    else:
        assert abs(got - want) <= EXACT_ULPS * 2.0 ** -23 * want, (what, d, got, want)


KNOWN_D2 = np.array([[0, 0], [1, 0], [1, 2], [1, 2], [0, 1.0]], np.float32)          # tests/test_hip_parity.py: 0.75


# ---------------------------------------------------------------------------------- CPU: the checker and the inputs
def test_inputs_exercise_the_exchange_and_stay_conditioned():
    for d in DIMS:
        for n in CHAINS:
            hist, ref, m = case(d, n)
            assert 48 <= hist.shape[0] <= 400 and hist.shape[1:] == (d, n)
            still = (np.diff(hist, axis=0) == 0).all(axis=1).mean()
            assert n == 1 or 0.2 < still < 0.4, (d, n, still)
            assert np.linalg.cond(m).max() <= COND_CAP, (d, n, np.linalg.cond(m).max())
            assert (ref > 0).all()
            if d >= 2:
                share = (np.abs(m[:, 1, 0]) > np.abs(m[:, 0, 0])).mean()
                assert share >= 1 / 3 if n > 1 else share == 1, (d, n, share)
                if n > 1:
                    assert share <= 0.8                       # and chains without an exchange remain


@pytest.mark.parametrize("d", DIMS)
def test_checker_matches_float64(oracle, d):
    worst = 0.0
    for n in CHAINS:
        hist, ref, _ = case(d, n)
        got = oracle_esjd(oracle, hist)
        worst = max(worst, rel_err(got, ref))
        # padding columns (NaN) are never read
        assert np.array_equal(bits(oracle_esjd(oracle, padded(hist, PAD), n)), bits(got))
    print("oracle_esjd d=%d: largest relative error %.3g" % (d, worst))
    assert worst < 2e-5
    assert worst <= ESJD_RTOL


@pytest.mark.parametrize("d", DIMS)
def test_checker_exact_cases(oracle, d):
    for kind in exact_kinds(d):
        hist, want = exact_history(d, kind)
        assert float(esjd_reference(hist)[0][0]) == pytest.approx(want, rel=1e-14, abs=0)
        assert_exact(oracle_esjd(oracle, hist)[0], want, d, kind)
    if d == 1:
        assert oracle_esjd(oracle, np.array([0.5, 2.0], np.float32).reshape(2, 1, 1))[0] == np.float32(2.25)
    if d == 2:
        assert oracle_esjd(oracle, KNOWN_D2[:, :, None])[0] == np.float32(0.75)


def test_checker_refusals(oracle):
    hist = np.zeros((4, 2, 3), np.float32)
    out = canary_f32(3)
    for rc, args in ((ERR_ARG, (hist.ctypes.data, 1, 2, 3, 3, out.ctypes.data)),
                     (ERR_DIM, (hist.ctypes.data, 4, 0, 3, 3, out.ctypes.data)),
                     (ERR_DIM, (hist.ctypes.data, 4, 9, 3, 3, out.ctypes.data)),
                     (ERR_NULL, (None, 4, 2, 3, 3, out.ctypes.data)),
                     (ERR_NULL, (hist.ctypes.data, 4, 2, 3, 3, None))):
        assert oracle.oracle_esjd(*args) == rc
        assert_untouched(out)
    assert oracle.oracle_esjd(hist.ctypes.data, 4, 2, 0, 3, out.ctypes.data) == 0
    assert_untouched(out)


# ---------------------------------------------------------------------------------- GPU
def hip_esjd(hip, hist, n=None):
    n_rows, d, stride = hist.shape
    n = stride if n is None else n
    out = dev(canary_f32(n + TAIL))
    assert hip.glabc_esjd(dev(np.array(hist)).data_ptr(), n_rows, d, n, stride, out.data_ptr(), None) == 0
    out = host(out)
    assert_written(out[:n])
    assert_untouched(out[n:])
    return out[:n]


def hip_moments_esjd(hip, mats, n_steps, stride):
    n, d, _ = mats.shape
    sj = dev(tri_rows(mats, stride))
    out = dev(canary_f32(n + TAIL))
    ms = A.Moments(None, None, sj.data_ptr())
    assert hip.glabc_moments_esjd(C.byref(ms), n_steps, d, n, stride, out.data_ptr(), None) == 0
    out = host(out)
    assert_written(out[:n])
    assert_untouched(out[n:])
    return out[:n]


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_esjd_kernel_matches_float64(hip, oracle, d):
    worst = worst_chk = 0.0
    for n in CHAINS:
        hist, ref, _ = case(d, n)
        got = hip_esjd(hip, hist)
        worst = max(worst, rel_err(got, ref))
        worst_chk = max(worst_chk, rel_err(got, oracle_esjd(oracle, hist).astype(np.float64)))
        assert np.array_equal(bits(hip_esjd(hip, padded(hist, PAD), n)), bits(got)), "stride > n_chains changed the result"
    print("esjd_kernel d=%d: largest relative error %.3g to float64, %.3g to the checker" % (d, worst, worst_chk))
    assert worst <= ESJD_RTOL
    assert worst_chk <= 2 * ESJD_RTOL                                  # both are within ESJD_RTOL of the reference


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_moments_esjd_kernel_matches_float64(hip, d):
    worst = worst_pair = 0.0
    for n in CHAINS:
        hist, ref, _ = case(d, n)
        mats, n_steps = jump_matrices(hist), hist.shape[0] - 1
        got = hip_moments_esjd(hip, mats, n_steps, n)
        worst = max(worst, rel_err(got, ref))
        assert np.array_equal(bits(hip_moments_esjd(hip, mats, n_steps, n + PAD)), bits(got))
        worst_pair = max(worst_pair, rel_err(got, hip_esjd(hip, hist).astype(np.float64)))
    print("moments_esjd_kernel d=%d: largest relative error %.3g to float64, %.3g to esjd_kernel" % (d, worst, worst_pair))
    assert worst <= ESJD_RTOL
    assert worst_pair <= ESJD_RTOL                                     # the two kernels, against each other


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_esjd_exact_cases(hip, d):
    for kind in exact_kinds(d):
        hist, want = exact_history(d, kind)
        assert_exact(hip_esjd(hip, hist)[0], want, d, "esjd " + kind)
        assert_exact(hip_moments_esjd(hip, jump_matrices(hist), 16, 1)[0], want, d, "moments " + kind)
    if d == 1:
        two = np.array([0.5, 2.0], np.float32).reshape(2, 1, 1)
        assert hip_esjd(hip, two)[0] == np.float32(2.25)
        assert hip_moments_esjd(hip, jump_matrices(two), 1, 1)[0] == np.float32(2.25)
    if d == 2:
        assert hip_esjd(hip, KNOWN_D2[:, :, None])[0] == np.float32(0.75)
        assert hip_moments_esjd(hip, jump_matrices(KNOWN_D2[:, :, None]), 4, 1)[0] == np.float32(0.75)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_esjd_python_surface(hip, d):
    from glabcmcmc_amd import engine, esjd
    from glabcmcmc_amd.ESJD import esjd_per_chain
    n = 65
    hist, ref, _ = case(d, n)
    per_chain = host(esjd_per_chain(dev(np.array(hist))))
    assert rel_err(per_chain, ref) <= ESJD_RTOL
    rows = np.array(hist.transpose(0, 2, 1), order="C")                # (N, C, D), a writable copy
    many = esjd(torch.from_numpy(rows))
    assert many.shape == (n,) and many.dtype == np.float32
    assert np.array_equal(bits(many), bits(per_chain))
    one = esjd(torch.from_numpy(rows[:, 3]))                           # (N, D)
    assert one.shape == () and one.dtype == np.float32 and bits(one) == bits(per_chain[3])
    wide = esjd(torch.from_numpy(rows.astype(np.float64)))             # a float64 CPU tensor holding float32 values
    assert np.array_equal(bits(wide), bits(per_chain))
    mom = engine.Moments(n, d, torch.device("cuda"))
    mom.sum_jump.copy_(dev(tri_rows(jump_matrices(hist), n)))
    mom.steps = hist.shape[0] - 1
    streamed = host(mom.esjd())
    assert rel_err(streamed, ref) <= ESJD_RTOL and rel_err(streamed, per_chain.astype(np.float64)) <= ESJD_RTOL
    for bad in (torch.zeros(5), torch.zeros(5, 2, d, 2)):
        with pytest.raises(ValueError):
            esjd(bad)


@pytest.mark.gpu
def test_esjd_refusals(hip):
    n_rows, d, n = 6, 3, 70
    hist = dev(np.asarray(esjd_histories(3, 321)[:n_rows, :, :n]))
    out = dev(canary_f32(n + TAIL))
    h, o = hist.data_ptr(), out.data_ptr()
    for rc, args in ((ERR_ARG, (h, 1, d, n, n, o)), (ERR_DIM, (h, n_rows, 0, n, n, o)), (ERR_DIM, (h, n_rows, 9, n, n, o)),
                     (ERR_ARG, (h, n_rows, d, n, n - 1, o)), (ERR_ARG, (h, n_rows, d, -1, n, o)),
                     (ERR_NULL, (None, n_rows, d, n, n, o)), (ERR_NULL, (h, n_rows, d, n, n, None)),
                     (0, (h, n_rows, d, 0, n, o)), (0, (h, n_rows, d, 0, 0, o))):
        assert hip.glabc_esjd(*args, None) == rc, args
        assert_untouched(host(out))
    sj = dev(tri_rows(np.tile(np.eye(d), (n, 1, 1)), n))
    ms, no_sums = A.Moments(None, None, sj.data_ptr()), A.Moments(None, None, None)
    for rc, args in ((ERR_ARG, (C.byref(ms), 0, d, n, n, o)), (ERR_DIM, (C.byref(ms), 5, 0, n, n, o)),
                     (ERR_DIM, (C.byref(ms), 5, 9, n, n, o)), (ERR_ARG, (C.byref(ms), 5, d, n, n - 1, o)),
                     (ERR_ARG, (C.byref(ms), 5, d, -1, n, o)), (ERR_NULL, (None, 5, d, n, n, o)),
                     (ERR_NULL, (C.byref(no_sums), 5, d, n, n, o)), (ERR_NULL, (C.byref(ms), 5, d, n, n, None)),
                     (0, (C.byref(ms), 5, d, 0, n, o))):
        assert hip.glabc_moments_esjd(*args, None) == rc, args
        assert_untouched(host(out))
