"""The device form of Box-Muller and of the logarithm's front end (include/glabc_numerics.h, offline gfx950 builds) returns
the bits of the host text -- the specification -- on EVERY input the kernels can feed it.  GPU only.

glabc_normal_pair(a, b) reads `a` only through glabc_uniform_pos_f32 (the radius) and `b` only through b >> 8 (the angle),
and the pair is (radius * cos, radius * sin): sweeping every radius at one angle and every angle at several radii covers both
factors exhaustively."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CHUNK = 1 << 24


def _device(hip, op, words):
    w = torch.from_numpy(words.view(np.int32)).cuda()
    n = words.size if op < 4 else words.size // 2
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    assert hip.glabc_selftest_numerics(op, w.data_ptr(), out.data_ptr(), n, None) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def _host_pair(oracle, a, b):
    z0 = np.empty(a.size, np.float32)
    z1 = np.empty(a.size, np.float32)
    oracle.oracle_normal_pair_v(a.ctypes.data, b.ctypes.data, a.size, z0.ctypes.data, z1.ctypes.data)
    return z0.view(np.uint32), z1.view(np.uint32)


def _pair_mismatches(hip, oracle, a, b):
    h0, h1 = _host_pair(oracle, a, b)
    words = np.stack([a, b], axis=1).reshape(-1).copy()
    return int((_device(hip, 4, words) != h0).sum()), int((_device(hip, 5, words) != h1).sum())


def test_every_radius_equals_host(hip, oracle):
    """b = 0: the pair is (rad * 1, rad * 0), so z0 is the radius itself.  Every word `a` whose (float)a is distinct: all
    a < 2^24, m << k for m in [2^23, 2^24) and k = 1 .. 8, and 0xffffffff ((float)a = 2^32) -- about 8.4e7 words; signs of
    zero included (u1 == 1 gives the radius -0)."""
    small = np.arange(1 << 24, dtype=np.uint32)
    m = np.arange(1 << 23, 1 << 24, dtype=np.uint32)
    chunks = [small] + [m << np.uint32(k) for k in range(1, 9)] + [np.array([0xffffffff], np.uint32)]
    seen_neg_zero = False
    for a in chunks:
        a = np.ascontiguousarray(a)
        b = np.zeros_like(a)
        h0, _ = _host_pair(oracle, a, b)
        seen_neg_zero = seen_neg_zero or bool((h0 == 0x80000000).any())
        assert _pair_mismatches(hip, oracle, a, b) == (0, 0)
    assert seen_neg_zero                                       # the sweep did reach log(1) = 0


def test_every_angle_equals_host(hip, oracle):
    """b = k << 8 for all 2^24 k, at the extreme radii and a few random ones"""
    rng = np.random.default_rng(5)
    fixed = [0, 1, 0xffffff80, 0xffffffff] + [int(x) for x in rng.integers(0, 2 ** 32, 3, dtype=np.uint64)]
    b = np.arange(1 << 24, dtype=np.uint32) << np.uint32(8)
    for a0 in fixed:
        a = np.full(b.size, a0, np.uint32)
        assert _pair_mismatches(hip, oracle, a, b) == (0, 0), hex(a0)
    # the low byte of b is not read
    a = np.full(b.size, fixed[4], np.uint32)
    assert _pair_mismatches(hip, oracle, a, b | np.uint32(0xa5)) == (0, 0)


def test_log_of_every_positive_normal_float_equals_host(hip, oracle):
    """glabc_logf on every positive normal float (bit patterns 0x00800000 .. 0x7f7fffff): the domain of glabc_logf_normal, whose
    front end the device build evaluates with v_frexp_exp_i32_f32 (the lowest binade goes through a subnormal there)"""
    bad = 0
    for first in range(0x00800000, 0x7f800000, CHUNK):
        x = np.arange(first, min(first + CHUNK, 0x7f800000), dtype=np.uint32)
        h = np.empty(x.size, np.float32)
        oracle.oracle_logf_v(x.ctypes.data, x.size, h.ctypes.data)
        bad += int((_device(hip, 1, x) != h.view(np.uint32)).sum())
    assert bad == 0
