"""The device Philox with its three-input XOR, and the certified fast iSIR weights of the index search
(csrc/glabc_device.h isir_weight_approx):
  - glabc_philox4x32_10 on the device (v_bitop3_b32 from round 3 on) equals the host build for random counters and keys;
  - the fast weight is within the bound the fast pass's 4e-6 margin assumes, for every float argument;
  - chains whose weights sit at the ends of the float range (log-weights near -104 and above 88.7, tiny and huge epsilon),
    where the fast pass must hand over to the specified weights, equal the CPU checker in the team, one-lane and
    GLABC_DEBUG_EXACT_INDEX geometries.
GPU only."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import bits, descriptors
from test_hip_parity import hip_run, oracle_run, assert_same_state

pytestmark = pytest.mark.gpu


def test_philox_device_equals_host(hip, oracle):
    rng = np.random.default_rng(5)
    n = 1 << 16
    words = rng.integers(0, 2 ** 32, (n, 6), dtype=np.uint64).astype(np.uint32)
    words[:4] = [[0, 0, 0, 0, 0, 0], [0xffffffff] * 6, [1, 0, 7, 3, 2026, 0], [5, 0, 1, 0, 0xffffffff, 0]]
    w = torch.from_numpy(words.reshape(-1).view(np.int32)).cuda()
    out = torch.empty(4 * n, dtype=torch.int32, device="cuda")
    assert hip.glabc_selftest_numerics(6, w.data_ptr(), out.data_ptr(), n, None) == 0
    torch.cuda.synchronize()
    dev = out.cpu().numpy().view(np.uint32).reshape(n, 4)
    host = np.empty((n, 4), np.uint32)
    ctr = (C.c_uint32 * 4)()
    key = (C.c_uint32 * 2)()
    res = (C.c_uint32 * 4)()
    for i in range(n):
        ctr[:] = [int(v) for v in words[i, :4]]
        key[:] = [int(v) for v in words[i, 4:]]
        oracle.oracle_philox4x32_10(ctr, key, res)
        host[i] = res[:]
    assert np.array_equal(dev, host)


def _weights(hip, op, x):
    out = torch.empty_like(x)
    assert hip.glabc_selftest_numerics(op, x.data_ptr(), out.data_ptr(), x.numel(), None) == 0
    return out.view(torch.float32)


def test_fast_weight_bound_every_float(hip):
    """|approx - exact| <= 1e-6 * exact + 2^-149 for all 2^32 arguments (the bound the 4e-6 margin of the fast index pass
    is derived from, glabc_device.h); where the exact weight overflows the approximate one is at least 2^127."""
    chunk = 1 << 26
    worst_rel = 0.0
    for lo in range(-(1 << 31), 1 << 31, chunk):
        x = torch.arange(lo, lo + chunk, dtype=torch.int64, device="cuda").to(torch.int32)
        a = _weights(hip, 7, x).double()
        e = _weights(hip, 8, x).double()
        fin = torch.isfinite(e)
        assert bool((e >= 0).all()) and not bool(torch.isnan(a).any())
        err = (a[fin] - e[fin]).abs()
        assert bool((err <= 1e-6 * e[fin] + 2.0 ** -149).all()), "bound broken in chunk %d" % lo
        assert bool((a[~fin] >= 2.0 ** 127).all())
        nrm = fin & (e >= 2.0 ** -126)
        if bool(nrm.any()):
            worst_rel = max(worst_rel, float(((a[nrm] - e[nrm]).abs() / e[nrm]).max()))
        torch.cuda.synchronize()
    assert 0.0 < worst_rel <= 1e-6
    print("isir_weight_approx: max relative error %.3g on normal weights" % worst_rel)


# kern_c0 is the additive constant of the log kernel: moving it puts every log-weight of the iteration near one end of the
# float range -- weights that overflow (above 88.72), weights in the denormals and totals below the fast pass's floor
# (around -104), totals just above that floor (-60, -75); the epsilons make most weights underflow or all of them equal.
EDGE_CASES = [
    # kern_c0 (None: the model's own), eps
    (88.6, 0.05), (87.0, 0.05), (-60.0, 0.05), (-75.0, 0.05), (-100.0, 0.05), (-103.0, 0.3),
    (None, 1e-4), (None, 0.002), (None, 3e6),
]


@pytest.mark.parametrize("geometry", ["team3", "team2", "lanes1", "lanes2", "lanes4", "exact"])
@pytest.mark.parametrize("c0,eps", EDGE_CASES, ids=lambda v: str(v))
def test_weights_at_the_ends_of_the_range_equal_the_checker(hip, oracle, c0, eps, geometry, monkeypatch):
    from glabcmcmc_amd import _capi as A
    model, local, glob = descriptors(dict(epsilon=eps, local=("gauss", [0, 0], [0.35, 0.35]),
                                          **{"global": ("gauss", [0, 0], [1, 1])}))
    if c0 is not None:
        model.kern_c0 = c0
    rng = np.random.default_rng(17)
    n, T, N, seed, gf = 1000, 120, 5, 4242, 0.8
    theta0 = (rng.standard_normal((n, 2)) * 1.5).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((n, 2))).astype(np.float32)
    lanes, flags = 0, 0
    if geometry.startswith("team"):
        monkeypatch.setenv("GLABC_TEAM_WAVES", geometry[4:])
        flags = A.DEBUG_TEAM
    elif geometry.startswith("lanes"):
        lanes, flags = int(geometry[5:]), A.DEBUG_NO_TEAM
    else:
        flags = A.DEBUG_EXACT_INDEX
    hist, chains, _ = hip_run("glmcmc", model, local, glob, theta0, y0, T, seed, gf, N, lanes=lanes, debug_flags=flags,
                              steps_per_launch=50)
    hh, hc, _ = oracle_run(oracle, "glmcmc", model, local, glob, theta0, y0, T, seed, gf, N)
    same = bits(hist) == bits(hh)
    assert same.all(), "first mismatch at (t, dim, chain) = %s" % (np.argwhere(~same)[0],)
    assert_same_state(chains, hc, True)
