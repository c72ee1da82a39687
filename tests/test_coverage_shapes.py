"""glabc_coverage_counts (csrc/glabc_coverage.hip) on the GPU, integer for integer against two independent statements of a pair:

(a) the restatement from the CPU checker's functions (tests/coverage_ref.py), and
(b) the on-device composition a user could write before: glabc_abc_draws for the table, then per test glabc_model_discrepancy of a
    copy of the Model whose y_obs is y*_r, the Model kernel's exponential through the device's own glabc_expf (glabc_selftest_numerics),
    NumPy integers for the rest.

Both give the multiplicity of every pair of N_REF table draws and N_TESTS tests once per (shape, row0, kernel); the two matrices must
be equal, and every call is then held to their partial sums.  Shapes: |theta| + noise at theta_dim 1 .. 8 and g-and-k; n around the
wavefront (64) and the chunk of draws (256); n_tests around the wavefront and around a tile (1, 2 and 4 wavefronts wide, and a second
tile); test_stride = n_tests + 3; row0 0 and 2^32 + 12345; both kernels.  The widths hold 0, +inf, a NaN, a width equal to one pair's
distance to the bit (<= must include it), a width below every distance (an empty test) and ordinary ones; test 0 IS table draw 5 of
row0 = 0 (distance 0 to it, and a theta* equal to a table theta to the bit, which is not below).  One call walks more chunks than the
grid has workgroups in x, which only the composition can follow.  Outputs lie between guard bands; pre-filled outputs are added to.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import coverage_ref as CR
import rejection_ref as R
from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import coverage, distribution, rejection
from glabcmcmc_amd.examples.Mixture import Mixture_set
from helpers import CANARY_I64, bits, canary_f32, dev, host

pytestmark = pytest.mark.gpu

ERR_NULL, ERR_DIM, ERR_KIND, ERR_ARG = -1, -2, -3, -4
SEED = 0x123456789ABCDEF1                  # both key words in use
TEST_SEED = SEED ^ coverage.COVERAGE_TEST_KEY
GUARD = 16
N_REF, N_TESTS = 1000, 257
ROW0S = (0, 2 ** 32 + 12345)
SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
TESTS = (1, 3, 63, 64, 65, 257)
KERNELS = ("hard", "model")
SHAPES = [("gauss", d) for d in range(1, 9)] + [("gk", 4)]
SELF = 5                                   # the table draw (row0 = 0) that test 0 is


def model_of(key):
    kind, d = key
    if kind == "gk":
        from glabcmcmc_amd.examples.GK import GK_set
        return GK_set(200.0).descriptor()
    prior = distribution.DiagGaussian(d, torch.tensor([0.1 * j for j in range(d)]), torch.log(torch.tensor([1.0 + 0.25 * j for j in range(d)])))
    return R.abs_gauss_model(d, prior, epsilon=0.4 + 0.3 * d).descriptor()


@functools.lru_cache(maxsize=None)
def table(key, row0):
    out = CR.table(model_of(key), SEED, row0, N_REF)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rows_of(key):
    """theta* [R][D], y* [R][YD], widths [R]: computed once, never modified"""
    model = model_of(key)
    ts, ys = CR.table(model, TEST_SEED, 0, N_TESTS)
    theta, y = table(key, 0)
    ts[0], ys[0] = theta[SELF], y[SELF]
    dist = CR.oracle_distance(model)
    typical = np.float32(np.median(dist(y, ys[1])))
    w = np.empty(N_TESTS, np.float32)
    for r in range(N_TESTS):
        d = np.concatenate([dist(table(key, row0)[1], ys[r]) for row0 in ROW0S])
        w[r] = (np.float32(0.0), np.float32(np.inf), np.float32(np.nan), d[0], d.min() * np.float32(0.5), typical, typical * np.float32(0.25))[r % 7]
    for a in (ts, ys, w):
        a.setflags(write=False)
    return ts, ys, w


def device_expf(hip, x):
    t, out = dev(np.ascontiguousarray(x, np.float32)), torch.empty(x.size, dtype=torch.float32, device="cuda")
    assert hip.glabc_selftest_numerics(0, t.data_ptr(), out.data_ptr(), x.size, None) == 0
    return host(out)


def composed_pairs(hip, model, row0, n, ys, widths, kernel):
    """(b) -> m [R][n] int64, theta [n][D]"""
    th, y = torch.empty(model.theta_dim, n, device="cuda"), torch.empty(model.y_dim, n, device="cuda")
    assert hip.glabc_abc_draws(C.byref(model), SEED, row0, None, n, n, th.data_ptr(), y.data_ptr(), None, None, None) == 0
    rows, dis = y.t().contiguous(), torch.empty(n, device="cuda")
    m = np.empty((ys.shape[0], n), np.int64)
    for r in range(ys.shape[0]):
        swapped = copy.copy(model)
        swapped.y_obs = type(model.y_obs)(*([float(v) for v in ys[r]] + [0.0] * (8 - ys.shape[1])))
        assert hip.glabc_model_discrepancy(C.byref(swapped), rows.data_ptr(), n, dis.data_ptr(), None) == 0
        d = host(dis)
        with np.errstate(all="ignore"):
            if kernel == "hard":
                m[r] = d <= widths[r]
            else:
                e = (d - np.float32(0.0)) / widths[r]
                p = device_expf(hip, -(np.float32(0.5) * (e * e)))
                m[r] = np.where(np.isnan(p), 0.0, np.rint(p * np.float32(65536.0)))
    return m, host(th.t().contiguous())


@functools.lru_cache(maxsize=None)
def pairs(key, row0, kernel):
    """(a) the restated multiplicities m [R][N_REF]"""
    ts, ys, w = rows_of(key)
    m = CR.pair_multiplicities(table(key, row0)[1], ys, w, kernel, CR.oracle_distance(model_of(key)))
    m.setflags(write=False)
    return m


def expected(key, row0, kernel, first, n, nt):
    ts = rows_of(key)[0]
    return CR.sums(pairs(key, row0, kernel)[:nt, first:first + n], table(key, row0)[0][first:first + n], ts[:nt])


class Sums:
    """an int64 device array of `size` sums, all `fill`, between two guard bands of canaries"""

    def __init__(self, size, fill=0):
        self.size, self.fill = size, fill
        a = np.full(size + 2 * GUARD, CANARY_I64, np.int64)
        a[GUARD:GUARD + size] = fill
        self.t = dev(a)
        self.ptr = self.t.data_ptr() + 8 * GUARD

    def read(self):
        h = host(self.t)
        assert (h[:GUARD] == CANARY_I64).all() and (h[GUARD + self.size:] == CANARY_I64).all(), "a sum outside the call's tests was written"
        return h[GUARD:GUARD + self.size] - self.fill

    def untouched(self):
        assert not self.read().any(), "a call that must write nothing wrote"


def padded(rows, nt, stride):
    """[nt][dim] host rows -> the dimension-major device array [dim][stride], columns nt .. stride - 1 canaries"""
    a = canary_f32(rows.shape[1], stride)
    a[:, :nt] = rows[:nt].T
    return dev(a)


def cov(hip, model, row0, n, rows, nt, kernel, want=("mass", "mass2", "below"), fill=0, stride=None, expect=0, null=()):
    """one glabc_coverage_counts call -> {name: what the call added}; `rows` = (theta* [R][D], y* [R][YD], widths [R])"""
    ts, ys, w = rows
    stride = max(nt, 0) + 3 if stride is None else stride
    size = max(nt, 1)
    t_dev, y_dev, w_dev = padded(ts, max(nt, 0), max(stride, size)), padded(ys, max(nt, 0), max(stride, size)), dev(np.append(w[:max(nt, 0)], canary_f32(3)))
    out = {"mass": Sums(size, fill), "mass2": Sums(size, fill), "below": Sums(size * model.theta_dim, fill)}
    p = lambda name: out[name].ptr if name in want else None           # noqa: E731
    a = lambda name, t: None if name in null else t.data_ptr()         # noqa: E731
    rc = hip.glabc_coverage_counts(C.byref(model), SEED, row0, n, a("theta_star", t_dev), a("y_star", y_dev), a("width", w_dev), nt, stride,
                                   KERNELS.index(kernel) if kernel in KERNELS else kernel, p("mass"), p("mass2"), p("below"), None)
    torch.cuda.synchronize()
    assert rc == expect, rc
    got = {}
    for name, s in out.items():
        if name in want and rc == 0 and n > 0 and nt > 0:
            got[name] = s.read()[:nt * (model.theta_dim if name == "below" else 1)]
        else:
            s.untouched()
    return got


def assert_sums(got, want, what):
    mass, mass2, below = want
    for name, ref in (("mass", mass), ("mass2", mass2), ("below", below.reshape(-1))):
        if name in got:
            assert got[name].tolist() == list(ref), "%s: %s differs" % (what, name)


# ---------------------------------------------------------------------------------- integer for integer
@pytest.mark.parametrize("key", SHAPES, ids=lambda k: "%s%d" % k)
def test_fused_equals_restatement_and_composition(hip, key):
    model, rows = model_of(key), rows_of(key)
    for row0 in ROW0S:
        for kernel in KERNELS:
            m, theta = composed_pairs(hip, model, row0, N_REF, rows[1], rows[2], kernel)
            assert np.array_equal(bits(theta), bits(table(key, row0)[0]))
            assert np.array_equal(m, pairs(key, row0, kernel)), "the composition and the restatement disagree on a pair"
            for n in SIZES:
                for nt in TESTS:
                    assert_sums(cov(hip, model, row0, n, rows, nt, kernel), expected(key, row0, kernel, 0, n, nt),
                                "%r row0 %d %s n %d n_tests %d" % (key, row0, kernel, n, nt))
    # what the widths were chosen to show, on the full table under the hard kernel
    mass, _, below = expected(key, 0, "hard", 0, N_REF, N_TESTS)
    hard = pairs(key, 0, "hard")
    assert mass[0] == 1 and hard[0, SELF] == 1                            # width 0: the test meets itself at distance 0
    assert not below[0].any()                                            # ... and its theta* equals that draw's theta: not below
    assert mass[1] == N_REF and mass[2] == 0                              # +inf keeps the table, a NaN nothing
    assert hard[3, 0] == 1 and mass[4] == 0                               # <= includes the pair's own distance; the empty test
    assert 0 < mass[5] < N_REF
    assert pairs(key, 0, "model")[1].tolist() == [65536] * N_REF and not pairs(key, 0, "model")[2].any()


@pytest.mark.parametrize("key", [("gauss", 2), ("gauss", 7), ("gk", 4)], ids=lambda k: "%s%d" % k)
def test_null_outputs_prefilled_outputs_and_split_calls(hip, key):
    model, rows = model_of(key), rows_of(key)
    for kernel in KERNELS:
        for nt in (3, 65, 257):
            want = expected(key, 0, kernel, 0, N_REF, nt)
            for outs in (("mass",), ("mass", "mass2"), ("mass", "below")):          # cov() checks that the others keep their contents
                got = cov(hip, model, 0, N_REF, rows, nt, kernel, want=outs)
                assert set(got) == set(outs)
                assert_sums(got, want, "want %r" % (outs,))
            assert_sums(cov(hip, model, 0, N_REF, rows, nt, kernel, fill=(1 << 40) + 7), want, "pre-filled outputs")
            assert_sums(cov(hip, model, 0, N_REF, rows, nt, kernel, stride=nt), want, "stride = n_tests")
        # [0, n1) and [n1, n) add up to [0, n), at both row0
        for row0 in ROW0S:
            for n1 in (1, 256, 300):
                a = cov(hip, model, row0, n1, rows, 65, kernel)
                b = cov(hip, model, row0 + n1, N_REF - n1, rows, 65, kernel)
                assert_sums(b, expected(key, row0, kernel, n1, N_REF - n1, 65), "the second part")
                assert_sums({k: a[k] + b[k] for k in a}, expected(key, row0, kernel, 0, N_REF, 65), "two calls")


@pytest.mark.parametrize("key", [("gauss", 2), ("gk", 4)], ids=lambda k: "%s%d" % k)
def test_more_chunks_than_workgroups(hip, key):
    """one tile of tests: the grid's x stops at 2048 workgroups and each walks on in steps of the grid"""
    model, rows = model_of(key), rows_of(key)
    n = 2048 * 256 + 300
    for kernel in KERNELS:
        m, theta = composed_pairs(hip, model, 0, n, rows[1][:3], rows[2][:3], kernel)
        assert_sums(cov(hip, model, 0, n, rows, 3, kernel), CR.sums(m, theta, rows[0][:3]), "%r %s" % (key, kernel))


def test_nothing_is_written_for_empty_and_refused_calls(hip):
    model, rows = model_of(("gauss", 2)), rows_of(("gauss", 2))
    assert cov(hip, model, 0, 0, rows, 5, "hard") == {} and cov(hip, model, 7, 10, rows, 0, "model") == {}
    cov(hip, model, 0, -1, rows, 5, "hard", expect=ERR_ARG)
    cov(hip, model, -1, 10, rows, 5, "hard", expect=ERR_ARG)
    cov(hip, model, 0, 10, rows, -1, "hard", stride=0, expect=ERR_ARG)
    cov(hip, model, 0, 10, rows, 5, "hard", stride=4, expect=ERR_ARG)
    cov(hip, model, 0, 10, rows, 5, 2, expect=ERR_ARG)
    cov(hip, model, 0, (1 << 30) + 1, rows, 5, "hard", expect=ERR_ARG)
    cov(hip, model, 0, 10, rows, 5, "hard", want=("mass2", "below"), expect=ERR_NULL)
    for name in ("theta_star", "y_star", "width"):
        cov(hip, model, 0, 10, rows, 5, "hard", null=(name,), expect=ERR_NULL)
    user = model_of(("gauss", 2))
    user.sim_kind = A.SIM_USER
    cov(hip, user, 0, 10, rows, 5, "hard", expect=ERR_KIND)
    gamma = Mixture_set(0.05, prior=distribution.Gamma(torch.tensor([2.0, 2.0]), torch.tensor([1.0, 1.0]))).descriptor()
    cov(hip, gamma, 0, 10, rows, 5, "hard", expect=ERR_KIND)
    odd = model_of(("gauss", 2))
    odd.y_dim = 3
    cov(hip, odd, 0, 10, rows, 5, "hard", expect=ERR_DIM)


# ---------------------------------------------------------------------------------- coverage.check on the fused path
def test_check_wrapper(hip, monkeypatch):
    d = 3
    m = R.abs_gauss_model(d, distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d)), epsilon=0.7)
    desc, n, nt = m.descriptor(), 1000, 70
    theta, y = CR.table(desc, SEED, 40, n)
    ts, ys = CR.table(desc, TEST_SEED, 0, nt)
    for kernel, eps in (("hard", 0.9), ("model", None)):
        w = np.full(nt, 0.7 if eps is None else eps, np.float32)
        want = CR.counts(theta, y, ts, ys, w, kernel, CR.oracle_distance(desc))
        c = coverage.check(m, nt, n, kernel=kernel, epsilon=eps, seed=SEED, row0=40)          # the default tests: draws under TEST_SEED
        assert c.mass.tolist() == list(want[0]) and c.mass2.tolist() == list(want[1]) and c.below.tolist() == want[2].tolist()
        assert c.kernel == kernel and c.n_draws == n and not c.mass.is_cuda and c.widths.tolist() == w.tolist()
        monkeypatch.setattr(rejection, "MAX_LAUNCH", 300)                 # a sweep of four launches adds up to the same sums
        c2 = coverage.check(m, nt, n, kernel=kernel, epsilon=eps, seed=SEED, row0=40, tests=(torch.from_numpy(ts).cuda(), torch.from_numpy(ys).cuda()))
        monkeypatch.undo()
        assert torch.equal(c2.mass, c.mass) and torch.equal(c2.mass2, c.mass2) and torch.equal(c2.below, c.below)
        # shards of the table and slices of the tests
        parts = [coverage.terms(m, t1 - t0, k, kernel=kernel, epsilon=eps, seed=SEED, row0=40 + r0, test0=t0,
                                tests=(torch.from_numpy(ts[t0:t1]).cuda(), torch.from_numpy(ys[t0:t1]).cuda()))
                 for t0, t1 in ((0, 64), (64, nt)) for r0, k in ((0, 256), (256, n - 256))]
        c3 = coverage.combine(parts)
        assert torch.equal(c3.mass, c.mass) and torch.equal(c3.mass2, c.mass2) and torch.equal(c3.below, c.below) and c3.n_draws == n
    # CPU test tensors under "auto" run the generic path on the same Philox table: the restatement fed the generic path's distance
    c4 = coverage.check(m, nt, n, kernel="hard", epsilon=0.9, seed=SEED, row0=40, tests=(torch.from_numpy(ts), torch.from_numpy(ys)))
    euclid = lambda yy, s: coverage.euclidean(torch.from_numpy(np.ascontiguousarray(yy)), torch.from_numpy(np.ascontiguousarray(s))).numpy()          # noqa: E731
    want = CR.counts(theta, y, ts, ys, np.full(nt, 0.9, np.float32), "hard", euclid)
    assert c4.mass.tolist() == list(want[0]) and c4.below.tolist() == want[2].tolist() and not c4.mass.is_cuda
