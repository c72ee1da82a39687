"""The three split-phase kernels of csrc/glabc_generic.hip -- glabc_propose, glabc_propose_redraw, glabc_select -- called
directly, one small launch per case, against their CPU checker twins (oracle_propose, oracle_propose_redraw, oracle_select)
on identical inputs.  Every buffer of a case -- chain state, step io, history, streaming sums, counters -- sits between guard
bands filled with the canaries of tests/helpers.py and is compared WHOLE, bit for bit, guard bands included; in addition

  * elements a call does not own (padding columns n_chains..stride-1, the rows of an absent proposal, history rows other than the
    addressed one, pure inputs) must hold what they held before the call,
  * elements a call owns must not hold the canary afterwards.

CPU part (no marker): the twins themselves are held to plain restatements -- oracle_select to the iSIR / MH arithmetic written
out in numpy + torch.sum from include/glabc.h and DESIGN.md 4.1f, oracle_propose to oracle_step_draws + oracle_dist_forward,
oracle_propose_redraw to the Philox slot rule GLABC_SLOT_REDRAW + 2*round + b.

The only primitives the restatements borrow from the checker are the ones other files pin on their own: Philox and the uniform
conversions (test_numerics.py), exp / log as the specified IEEE sequences of include/glabc_numerics.h (test_numerics.py),
Box-Muller (test_hip_boxmuller.py), forward() / log_prob() of a descriptor (test_oracle_golden.py) and, above 17 terms,
torch.sum's order (primitives.npz, test_oracle_golden.py::test_rowsum_order).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from helpers import CANARY_BITS, CANARY_BITS64, CANARY_I32, canary_f32, canary_f64, canary_i32, make_dist
from glabcmcmc_amd import _capi as A

G = 64                                            # guard band, elements on either side of every buffer
CHAIN_COUNTS = (1, 63, 255, 256, 257, 300)
SENTINEL = np.float32(7 * math.log(1e-10))
ALGOS = {"glmcmc": A.ALGO_GLMCMC, "globalmcmc": A.ALGO_GLOBALMCMC, "glmala": A.ALGO_GLMALA}
F32 = np.float32


# ------------------------------------------------------------------------------------------------------ buffers and canaries
def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def canary(dtype, *shape):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return canary_f32(*shape)
    if dtype == np.float64:
        return canary_f64(*shape)
    assert dtype == np.int32, dtype
    return canary_i32(*shape)


def holds_canary(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return raw(a) == CANARY_BITS
    if a.dtype == np.float64:
        return raw(a) == CANARY_BITS64
    return a == CANARY_I32


def padded(values, stride):
    """[rows][n] values -> [rows][stride] with the canary in columns n..stride-1"""
    values = np.atleast_2d(values)
    out = canary(values.dtype, values.shape[0], stride)
    out[:, :values.shape[1]] = values
    return out


def cols(rows, stride, n):
    m = np.zeros((rows, stride), bool)
    m[:, :n] = True
    return m


def ref(x):
    return None if x is None else C.byref(x)


class Case:
    """One call of one entry point: scalars, descriptors, and every buffer as a host array in its logical shape.  `owned`
    maps a buffer to the mask of the elements the call writes; a buffer without a mask is a pure input."""

    def __init__(self, entry, algo, n, N, d, yd, nd, *, pad=0, chain0=0, seed=991, step0=3, gf=0.6, local=None, glob=None,
                 rnd=0, hist_stride=0, tag=""):
        self.entry, self.algo, self.n, self.N, self.d, self.yd, self.nd = entry, algo, n, N, d, yd, nd
        self.stride, self.chain0, self.seed, self.step0, self.gf = n + pad, chain0, seed, step0, gf
        self.local, self.glob, self.rnd, self.hist_stride, self.tag = local, glob, rnd, hist_stride, tag
        self.bufs, self.owned = {}, {}

    def what(self):
        return "%s %s n=%d N=%d d=%d yd=%d nd=%d stride=%d chain0=%d %s" % (self.entry, self.algo, self.n, self.N, self.d, self.yd,
                                                                            self.nd, self.stride, self.chain0, self.tag)

    def run(self, lib, side):
        """-> (status, {name: flat array with its guard bands})"""
        hip = side == "hip"
        store = {}
        for k, v in self.bufs.items():
            flat = np.concatenate([canary(v.dtype, G), np.ascontiguousarray(v).ravel(), canary(v.dtype, G)])
            store[k] = torch.from_numpy(flat).cuda() if hip else flat

        def p(k):
            if k not in store:
                return None
            t = store[k]
            return t.data_ptr() + G * t.element_size() if hip else t.ctypes.data + G * t.itemsize

        cs = A.Chains(self.n, self.chain0, self.stride, p("theta"), p("y"), p("log_w"), p("flags"), p("n_moves"),
                      None, None, None, None)
        run = A.Run()
        run.seed, run.step0, run.n_steps, run.global_frequency, run.batch_size = self.seed, self.step0, 1, self.gf, self.N
        run.history, run.hist_stride = p("history"), self.hist_stride
        mom = None
        if "sum_theta" in store:
            mom = A.Moments(p("sum_theta"), p("sum_outer"), p("sum_jump"))
            run.moments = C.pointer(mom)
        run.step0_device, run.global_frequency_per_chain = p("step_dev"), p("gf_chain")
        io = A.StepIO(self.N, self.d, self.yd, self.nd, p("theta_prop"), p("log_q"), p("sim_noise"), p("log_u"), p("u_res"),
                      p("is_global"), p("y_prop"), p("prior_prop"), p("kern_prop"), p("prior_cur"), p("kern_cur"), p("q_cur"),
                      p("n_valid"))
        tail = (None,) if hip else ()
        pre = "glabc_" if hip else "oracle_"
        if self.entry == "propose":
            rc = getattr(lib, pre + "propose")(self.algo, ref(self.local), ref(self.glob), C.byref(cs), C.byref(run), C.byref(io), *tail)
        elif self.entry == "redraw":
            rc = getattr(lib, pre + "propose_redraw")(ref(self.local), C.byref(cs), C.byref(run), C.byref(io), self.rnd,
                                                      p("n_redrawn"), *tail)
        else:
            rc = getattr(lib, pre + "select")(self.algo, ref(self.glob), C.byref(cs), C.byref(run), C.byref(io), *tail)
        if hip:
            torch.cuda.synchronize()
            return rc, {k: t.cpu().numpy() for k, t in store.items()}
        return rc, store

    def body(self, out, k):
        return out[k][G:len(out[k]) - G].reshape(self.bufs[k].shape)

    def check_ownership(self, out, side):
        """guard bands intact; unowned elements unchanged; owned elements written"""
        for k, v in self.bufs.items():
            flat = out[k]
            assert holds_canary(flat[:G]).all() and holds_canary(flat[len(flat) - G:]).all(), ("guard band of " + k, side, self.what())
            got, init = raw(self.body(out, k)), raw(v)
            own = self.owned.get(k)
            if own is None:
                assert np.array_equal(got, init), ("input %s was written" % k, side, self.what())
                continue
            own = np.broadcast_to(own, v.shape)
            assert np.array_equal(got[~own], init[~own]), ("%s: an element the call does not own changed" % k, side, self.what())
            left = int(holds_canary(self.body(out, k))[own].sum())
            assert left == 0, ("%s: %d owned elements still hold the canary" % (k, left), side, self.what())

    def same(self, got, want):
        for k in self.bufs:
            a, b = raw(got[k]), raw(want[k])
            if not np.array_equal(a, b):
                i = int(np.flatnonzero(a != b)[0]) - G
                raise AssertionError("%s differs from the checker, first at flat element %d of %d (%s)"
                                     % (k, i, self.bufs[k].size, self.what()))


def twin_check(hip, oracle, case, finish=None):
    """the checker, then the kernel, on the case's inputs; `finish(case, want)` completes the ownership masks / quality checks
    from the checker's output"""
    rc, want = case.run(oracle, "oracle")
    assert rc == 0, (rc, case.what())
    if finish:
        finish(case, want)
    case.check_ownership(want, "oracle")
    rc, got = case.run(hip, "hip")
    assert rc == 0, (rc, case.what())
    case.same(got, want)
    case.check_ownership(got, "hip")
    return want


# ------------------------------------------------------------------------------------------------------------- descriptors
def dist_of(kind, d, rng, local=False):
    if kind is None:
        return None
    if kind == "gauss":
        loc = [0.0] * d if local else [float(x) for x in rng.uniform(-1, 1, d)]
        return make_dist(("gauss", loc, [float(x) for x in rng.uniform(0.2, 1.5, d)])).descriptor()
    if kind == "uniform":
        low = rng.uniform(-2.0, -0.5, d)
        return make_dist(("uniform", [float(x) for x in low], [float(x) for x in low + rng.uniform(0.5, 3.0, d)])).descriptor()
    shape = [(0.6, 2.5, 1.0, 0.35, 7.0)[j % 5] for j in range(d)]                # both sides of 1, and 1 itself
    return make_dist(("gamma", shape, [float(x) for x in rng.uniform(0.5, 2.0, d)])).descriptor()


def branch_uniform(oracle, seed, chain, step):
    """the float32 uniform GLMCMC.py:59 compares with global_frequency, for one (chain, step)"""
    u2, r, z = np.zeros(2, F32), np.zeros(1), np.zeros(4, F32)
    oracle.oracle_step_draws(seed, chain, step, 1, 1, 1, u2.ctypes.data, r.ctypes.data, z.ctypes.data)
    return u2[0]


# ------------------------------------------------------------------------------------------------------------ glabc_propose
def propose_case(algo, d, nd, N, n, lk, gk, rng, *, pad=0, chain0=0, seed=991, step0=3, gf=0.6, gf_chain=None, step_dev=None,
                 tag=""):
    local = dist_of(lk, d, rng, local=True) if d <= A.MAX_DIM else None
    glob = dist_of(gk, d, rng) if d <= A.MAX_DIM else None
    c = Case("propose", ALGOS[algo], n, N, d, 1, nd, pad=pad, chain0=chain0, seed=seed, step0=step0, gf=gf, local=local, glob=glob,
             tag="local=%s global=%s %s" % (lk, gk, tag))
    R = N * n
    c.bufs = dict(theta=padded(rng.standard_normal((d, n)).astype(F32), c.stride), y=padded(np.zeros((1, n), F32), c.stride),
                  theta_prop=canary(F32, R, d), log_q=canary(F32, R), log_u=canary(F32, n), u_res=canary(np.float64, n),
                  is_global=canary(np.int32, n))
    if nd > 0:
        c.bufs["sim_noise"] = canary(F32, R, nd)
    if gf_chain is not None:
        c.bufs["gf_chain"] = np.asarray(gf_chain, F32)
    if step_dev is not None:
        c.bufs["step_dev"] = np.array([step_dev], np.int32)
    for k in ("log_u", "u_res", "is_global", "sim_noise"):
        if k in c.bufs:
            c.owned[k] = np.ones(c.bufs[k].shape, bool)
    return c


def propose_finish(case, want):
    """rows of an absent proposal belong to the caller: global rows are candidates j >= 1 and row 0 of a global-branch chain"""
    n, N = case.n, case.N
    isg = case.body(want, "is_global")
    assert np.isin(isg, (0, 1)).all()
    rows = np.full((N, n), case.glob is not None)
    rows[0, isg == 0] = case.local is not None
    case.owned["log_q"] = rows.reshape(N * n)
    case.owned["theta_prop"] = rows.reshape(N * n, 1)
    case.branch = isg


PROPOSAL_PAIRS = [(lk, gk) for lk in ("gauss", "uniform", None) for gk in ("gauss", "uniform", "gamma", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6, 7, 8])
def test_hip_propose_shape_grid(hip, oracle, d):
    """theta_dim 1..8 x noise_dim {0, 1, 2, 3, 5, 9}: both parities of DP, 1 / 2 / >= 3 Philox blocks per candidate, the first
    noise word in block 0, 1 and 2; every (local, global) pair of proposals at every theta_dim (two per shape)"""
    rng = np.random.default_rng(100 + d)
    k = d
    both = set()
    for i, nd in enumerate((0, 1, 2, 3, 5, 9)):
        for rep in range(2):
            lk, gk = PROPOSAL_PAIRS[k % 12]
            n, N = CHAIN_COUNTS[k % 6], (1, 2, 5, 16, 17, 40)[(k // 2) % 6]
            k += 1
            case = propose_case("glmcmc", d, nd, N, n, lk, gk, rng, chain0=5)
            twin_check(hip, oracle, case, propose_finish)
            both.update(case.branch.tolist())
    assert both == {0, 1}


@pytest.mark.gpu
@pytest.mark.parametrize("d", [9, 12])
def test_hip_propose_callback_only_shapes(hip, oracle, d):
    """theta_dim beyond GLABC_MAX_DIM: both proposals NULL, theta_prop and log_q stay the caller's, the noise starts at word DP"""
    rng = np.random.default_rng(d)
    for nd in (0, 1, 2, 3, 5, 9):
        for n, N in ((63, 5), (300, 2), (1, 17)):
            twin_check(hip, oracle, propose_case("glmcmc", d, nd, N, n, None, None, rng), propose_finish)


@pytest.mark.gpu
@pytest.mark.parametrize("lk", ["gauss", "uniform", None])
def test_hip_propose_every_proposal_pair(hip, oracle, lk):
    """local in {gauss, uniform, NULL} x global in {gauss, uniform, gamma (shapes on both sides of 1), NULL} at theta_dim 1, 3, 5, 8"""
    rng = np.random.default_rng(7)
    for gk in ("gauss", "uniform", "gamma", None):
        for d, n, N, nd in ((1, 63, 5, 2), (3, 257, 2, 0), (5, 255, 1, 3), (8, 300, 3, 1)):
            twin_check(hip, oracle, propose_case("glmcmc", d, nd, N, n, lk, gk, rng), propose_finish)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["glmcmc", "glmala", "globalmcmc"])
def test_hip_propose_algorithms_and_batch_sizes(hip, oracle, algo):
    rng = np.random.default_rng(11)
    for i, N in enumerate((1,) if algo == "globalmcmc" else (1, 2, 5, 16, 17, 40)):
        for j, n in enumerate(CHAIN_COUNTS):
            lk, gk = PROPOSAL_PAIRS[(5 * i + j) % 12]
            d = 1 + (i + 3 * j) % 8
            twin_check(hip, oracle, propose_case(algo, d, (2, 0, 3)[j % 3], N, n, lk, gk, rng), propose_finish)


@pytest.mark.gpu
def test_hip_propose_row_edges(hip, oracle):
    """n_prop * n_chains in {1, 255, 256, 257}, and chain counts that do not divide the 256-row block: one block then holds
    rows of two candidates j (100 x 5: rows 200..299 | 300..399 ... straddle blocks 0 / 1)"""
    rng = np.random.default_rng(13)
    for n, N in ((1, 1), (255, 1), (51, 5), (256, 1), (128, 2), (16, 16), (257, 1), (100, 5), (100, 3), (37, 7), (300, 40)):
        for lk, gk in (("gauss", "gauss"), ("uniform", "gamma")):
            twin_check(hip, oracle, propose_case("glmcmc", 3, 2, N, n, lk, gk, rng), propose_finish)


@pytest.mark.gpu
@pytest.mark.parametrize("edge", ["chain0", "stride", "gf", "gf_chain", "step0_device", "seed"])
def test_hip_propose_run_edges(hip, oracle, edge):
    """each run-level field on its own"""
    rng = np.random.default_rng(17)
    seed, step0 = 991, 3
    for n in CHAIN_COUNTS:
        kws = []
        if edge == "chain0":                                   # the chain id crosses 2^32 inside the launch: Philox counter word 1
            kws = [dict(chain0=0), dict(chain0=2 ** 32 - 3), dict(chain0=2 ** 40 + 7)]
        elif edge == "stride":
            kws = [dict(pad=5)]
        elif edge == "gf":
            kws = [dict(gf=0.0), dict(gf=1.0), dict(gf=0.5)]
        elif edge == "gf_chain":
            # 0, 1, fractions, and the chain's own branch uniform (torch.rand(1) < f is strict: local) and the float above it (global)
            ub = np.array([branch_uniform(oracle, seed, c, step0) for c in range(n)], F32)
            f = np.array([(0.0, 1.0, 0.25, 0.5, 0.999)[c % 5] for c in range(n)], F32)
            f[2::7] = ub[2::7]
            f[3::7] = np.nextafter(ub[3::7], F32(2))
            kws = [dict(gf_chain=f, gf=0.0), dict(gf_chain=f, gf=1.0)]
        elif edge == "step0_device":
            kws = [dict(step_dev=step0 + 3)]
        else:
            kws = [dict(seed=0x9E3779B97F4A7C15), dict(seed=0xFFFFFFFF00000001)]
        for kw in kws:
            case = propose_case("glmcmc", 3, 2, 5, n, "gauss", "gauss", rng, tag=edge, **kw)
            want = twin_check(hip, oracle, case, propose_finish)
            isg = case.body(want, "is_global")
            if edge == "gf":
                assert kw["gf"] == 0.5 or (isg == int(kw["gf"])).all()
            if edge == "gf_chain":
                f = kw["gf_chain"]
                assert (isg[f == 0] == 0).all() and (isg[f == 1] == 1).all()
                assert (isg[2::7] == 0).all() and (isg[3::7] == 1).all()                   # decided on the boundary itself
            if edge == "step0_device":                                                    # the device word wins over run.step0
                plain = propose_case("glmcmc", 3, 2, 5, n, "gauss", "gauss", np.random.default_rng(1), step0=step0 + 3)
                _, alt = plain.run(oracle, "oracle")
                assert np.array_equal(raw(plain.body(alt, "u_res")), raw(case.body(want, "u_res")))
                assert np.array_equal(raw(plain.body(alt, "sim_noise")), raw(case.body(want, "sim_noise")))
                other = propose_case("glmcmc", 3, 2, 5, n, "gauss", "gauss", np.random.default_rng(1), step0=step0)
                _, alt = other.run(oracle, "oracle")
                assert not np.array_equal(raw(other.body(alt, "u_res")), raw(case.body(want, "u_res")))


# ----------------------------------------------------------------------------------------------------- glabc_propose_redraw
def redraw_case(d, lk, rnd, n, rng, *, pad=0, chain0=0, step_dev=None, seed=991):
    N = 3                                                       # rows j >= 1 exist and must stay untouched
    local = dist_of(lk, d, rng, local=True)
    c = Case("redraw", A.ALGO_GLMCMC, n, N, d, 1, 0, pad=pad, chain0=chain0, seed=seed, local=local, rnd=rnd,
             tag="local=%s round=%d" % (lk, rnd))
    below, above = np.nextafter(SENTINEL, F32(-np.inf)), np.nextafter(SENTINEL, F32(0))
    menu = np.array([SENTINEL, below, above, np.nan, -np.inf, -1.25, SENTINEL, 0.0, SENTINEL], F32)
    prior = menu[rng.integers(0, len(menu), N * n)]
    prior[n:] = SENTINEL                                        # only row j = 0 of a chain is looked at
    isg = rng.integers(0, 4, n).astype(np.int32)                # bit 0 decides; bit 1 is glabc_select's `moved`
    c.bufs = dict(theta=padded(rng.standard_normal((d, n)).astype(F32), c.stride), y=padded(np.zeros((1, n), F32), c.stride),
                  theta_prop=canary(F32, N * n, d), prior_prop=prior, is_global=isg, n_redrawn=np.array([11], np.int32))
    if step_dev is not None:
        c.bufs["step_dev"] = np.array([step_dev], np.int32)
    redraw = ((isg & 1) == 0) & (raw(prior[:n]) == raw(SENTINEL))
    rows = np.zeros((N, n), bool)
    rows[0] = redraw
    c.owned = dict(theta_prop=rows.reshape(N * n, 1), n_redrawn=np.ones(1, bool))
    c.redraw = redraw
    return c


def redraw_finish(case, want):
    k = int(case.redraw.sum())
    assert 1 <= k < case.n, ("a case must redraw a chain and skip a chain", k, case.what())
    assert int(case.body(want, "n_redrawn")[0]) == 11 + k


@pytest.mark.gpu
@pytest.mark.parametrize("lk", ["gauss", "uniform"])
def test_hip_redraw_shapes(hip, oracle, lk):
    """theta_dim 1..8 x rounds {1, 2, 7, 2^24}; the sentinel is matched exactly (its float32 neighbours, NaN and -inf are not);
    bit 0 of is_global decides; the counter continues from 11; every row of a chain that did not redraw, and every row
    j >= 1, keeps its bits"""
    rng = np.random.default_rng(23)
    k = 0
    for d in range(1, 9):
        for rnd in (1, 2, 7, 2 ** 24):
            n = CHAIN_COUNTS[1 + k % 5]
            k += 1
            twin_check(hip, oracle, redraw_case(d, lk, rnd, n, rng), redraw_finish)
    for kw in (dict(pad=5), dict(chain0=2 ** 32 - 3), dict(chain0=2 ** 40 + 7), dict(step_dev=6), dict(seed=0x9E3779B97F4A7C15)):
        twin_check(hip, oracle, redraw_case(3, lk, 2, 257, rng, **kw), redraw_finish)


# ------------------------------------------------------------------------------------------------------------- glabc_select
PLANTED = 11


def select_case(oracle, algo, N, d, yd, n, qsrc, rs, *, pad=0, hist=True, hist_pad=0, moments=True, n_moves=True, step_dev=None,
                n_valid=None, flags_mode="mix", plant=True, chain0=0):
    """synthetic callback results.  qsrc: 'q_cur' or the kind of the `global` descriptor that scores Theta_old.  The current
    state's terms are placed so that a chain stays with probability about one half whatever N is."""
    rng = np.random.default_rng(rs)
    step0 = 3
    isir = algo != "globalmcmc"
    glob = None if qsrc == "q_cur" else dist_of(qsrc, d, rng)
    hs = n + hist_pad if hist else 0
    c = Case("select", ALGOS[algo], n, N, d, yd, 0, pad=pad, chain0=chain0, step0=step0, glob=glob, hist_stride=hs,
             tag="q=%s flags=%s n_valid=%s seed=%d" % (qsrc, flags_mode, n_valid, rs))
    R = N * n
    f32 = lambda a: np.asarray(a, F32)                                        # noqa: E731
    theta = f32(rng.standard_normal((d, n)))
    if qsrc == "gamma":
        theta = np.abs(theta) + F32(0.05)
    if qsrc in ("gamma", "uniform"):
        theta[:, 9::10] = F32(-3.0)                                           # states outside the support: q = -inf
    if qsrc == "uniform":                                                     # most states inside the box
        lo, hi = np.array(glob.p0[:d], F32), np.array(glob.p1[:d], F32)
        inside = lo[:, None] + (hi - lo)[:, None] * f32(rng.random((d, n)))
        keep = np.ones(n, bool)
        keep[9::10] = False
        theta[:, keep] = inside[:, keep]
    prior_p, kern_p = f32(-1.5 * rng.random(R)), f32(-3.0 * rng.random(R))
    log_q = f32(-2.0 * rng.random(R)) if algo != "glmala" else f32(rng.standard_normal(R))
    isg = (rng.random(n) < 0.6).astype(np.int32)
    if n == 1:
        isg[:] = rs % 2
    flags = {"mix": (rng.random(n) < 0.5).astype(np.int32), "set": np.ones(n, np.int32), "clear": np.zeros(n, np.int32)}[flags_mode]
    flags |= 8 * (rng.random(n) < 0.3).astype(np.int32)                       # a bit glabc_select has no business with
    nv = None
    if n_valid == "all":
        nv = rng.integers(-1, N + 4, n).astype(np.int32)                      # -1, 0 .. N, N + 3
        nv[:N + 5] = np.arange(-1, N + 4)[:n]
    # the score of the current state under the importance proposal
    if glob is None:
        q = f32(-2.0 * rng.random(n))
    else:
        q = np.zeros(n, F32)
        rows = np.ascontiguousarray(theta.T)
        assert oracle.oracle_dist_log_prob(C.byref(glob), rows.ctypes.data, n, q.ctypes.data) == 0
    qf = np.where(np.isfinite(q), q, 0.0).astype(np.float64)
    prior_c = f32(-1.5 * rng.random(n))
    t = rng.normal(0.0, 1.2, n)
    lw = prior_p.astype(np.float64) + kern_p - log_q
    Nc = np.full(n, N) if nv is None else np.clip(nv, 0, N)
    with np.errstate(divide="ignore"):
        mass = np.log(np.array([np.exp(lw[np.arange(Nc[i]) * n + i]).sum() for i in range(n)]))
    mass = np.where(np.isfinite(mass), mass, 0.0)
    pk0 = prior_p[:n].astype(np.float64) + kern_p[:n]
    if isir:
        target = np.where(isg == 1, mass + t, 0.0)
        log_w = f32(target)
        kern_c = np.where(isg == 1, target - prior_c + qf, pk0 + (log_q[:n] if algo == "glmala" else 0.0) - prior_c - (t - 0.7))
    else:
        log_w = None
        kern_c = np.where(isg == 1, pk0 + qf - log_q[:n] - prior_c - (t - 0.7), pk0 - prior_c - (t - 0.7))
    kern_c = f32(kern_c)
    log_u = np.log(f32(1.0 - rng.random(n))).astype(F32)
    u_res = rng.random(n)
    if plant and n >= 63:
        assert n > PLANTED and N >= 1
        last = (N - 1) * n
        isg[[0, 1, 2, 3, 4, 8, 9, 10]] = 1
        isg[[5, 6, 7]] = 0
        if nv is not None:
            nv[:PLANTED] = N
        if isir:
            flags[[0, 3]] &= ~1                                               # the planted log_w must be the one that is used
            log_w[0] = -np.inf
            log_w[3] = -np.inf
        for j in range(N):
            prior_p[j * n + 0] = -np.inf                                      # chain 0: every weight is 0 -> 0/0 -> stays
        prior_p[1] = np.nan                                                   # chain 1: one NaN prior -> that weight is 0
        kern_p[last + 2] = np.inf                                             # chain 2: a +inf weight -> inf/inf -> stays
        u_res[3] = 0.0                                                        # chain 3: u = 0 against a running sum that starts at 0
        u_res[4] = 1.0 - 2.0 ** -53                                           # chain 4: the largest double below 1
        log_u[5] = -np.inf                                                    # chains 5..7: the MH test of the local move
        prior_p[6] = np.nan
        kern_p[7] = np.inf
        log_u[8] = -np.inf                                                    # chains 8..10: GlobalMCMC's independence test
        prior_p[9] = np.nan
        kern_p[10] = np.inf
    tri = d * (d + 1) // 2
    c.bufs = dict(theta=padded(theta, c.stride), y=padded(f32(rng.standard_normal((yd, n))), c.stride),
                  theta_prop=f32(rng.standard_normal((R, d))), y_prop=f32(rng.standard_normal((R, yd))), prior_prop=prior_p,
                  kern_prop=kern_p, log_q=log_q, log_u=log_u, u_res=u_res, is_global=isg, prior_cur=prior_c, kern_cur=kern_c)
    row = cols(1, c.stride, n)
    c.owned = dict(theta=cols(d, c.stride, n), y=cols(yd, c.stride, n), is_global=np.ones(n, bool), prior_cur=np.ones(n, bool),
                   kern_cur=np.ones(n, bool))
    # GlobalMCMC neither reads nor writes log_w / flags: there they are canaries that must survive
    c.bufs["log_w"] = padded(log_w, c.stride) if isir else canary(F32, 1, c.stride)
    c.bufs["flags"] = padded(flags, c.stride) if isir else canary(np.int32, 1, c.stride)
    if isir:
        c.owned.update(log_w=row, flags=row)
    if n_moves:
        c.bufs["n_moves"] = padded(rng.integers(0, 1000, n).astype(np.int32), c.stride)
        c.owned["n_moves"] = row
    if glob is None:
        c.bufs["q_cur"] = q
    if nv is not None:
        c.bufs["n_valid"] = nv
    if hist:
        rows_h = 1 if step_dev is None else 4
        c.bufs["history"] = canary(F32, rows_h, d, hs)
        own = np.zeros((rows_h, d, hs), bool)
        own[0 if step_dev is None else step_dev - step0, :, :n] = True
        c.owned["history"] = own
    if step_dev is not None:
        c.bufs["step_dev"] = np.array([step_dev], np.int32)
    if moments:
        c.bufs.update(sum_theta=padded(rng.standard_normal((d, n)), c.stride), sum_outer=padded(rng.standard_normal((tri, n)), c.stride),
                      sum_jump=padded(rng.standard_normal((tri, n)), c.stride))
        c.owned.update(sum_theta=cols(d, c.stride, n), sum_outer=cols(tri, c.stride, n), sum_jump=cols(tri, c.stride, n))
    return c


def moved_of(case, out):
    return (case.body(out, "is_global") & 2) != 0


def balanced_select_cases(oracle, *args, **kw):
    """the case(s) of the first seed(s) at which, on the checker, at least a quarter of the chains move and at least a quarter
    stay; a single chain cannot do both, so one chain gives two cases: one that moves and one that stays"""
    n = args[4]
    found = {}
    for rs in range(1000, 1040):
        case = select_case(oracle, *args, rs, **kw)
        rc, want = case.run(oracle, "oracle")
        assert rc == 0, (rc, case.what())
        m = moved_of(case, want)
        if n == 1:
            found.setdefault(bool(m[0]), case)
            if len(found) == 2:
                return [found[True], found[False]]
        elif 4 * m.sum() >= n and 4 * (~m).sum() >= n:
            return [case]
    raise AssertionError("no balanced seed for " + case.what())


def select_finish(case, want):
    m = moved_of(case, want)
    n = case.n
    assert n == 1 or (4 * m.sum() >= n and 4 * (~m).sum() >= n), (int(m.sum()), case.what())


def select_twin(hip, oracle, *args, **kw):
    for case in balanced_select_cases(oracle, *args, **kw):
        twin_check(hip, oracle, case, select_finish)


QSRC = ("q_cur", "gauss", "uniform", "gamma")


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["glmcmc", "globalmcmc", "glmala"])
def test_hip_select_batch_sizes(hip, oracle, algo):
    """n_prop 1..16, 17, 40 (GlobalMCMC: 1) with theta_dim cycling through 1..8, y_dim through {1, 3, 8, 11}, q(Theta_old) from
    q_cur or a gauss / uniform / gamma descriptor, every chain count, the planted chains in every case of 63 chains or more"""
    sizes = (1,) * 8 if algo == "globalmcmc" else tuple(range(1, 17)) + (17, 40)
    for i, N in enumerate(sizes):
        d, yd = 1 + i % 8, (1, 3, 8, 11)[i % 4]
        select_twin(hip, oracle, algo, N, d, yd, CHAIN_COUNTS[i % 6], QSRC[(i // 2) % 4])


@pytest.mark.gpu
def test_hip_select_first_cascade_level_of_the_row_sum(hip, oracle):
    """511, 512 and 513 weights: aten_rowsum_rt meets torch.sum's first cascade level inside select_kernel"""
    for N in (510, 511, 512):
        select_twin(hip, oracle, "glmcmc", N, 2, 3, 70, "q_cur")
    select_twin(hip, oracle, "glmala", 511, 3, 1, 70, "gauss")


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["glmcmc", "globalmcmc", "glmala"])
def test_hip_select_dimensions(hip, oracle, algo):
    """theta_dim 1..8 with every source of q(Theta_old), theta_dim 12 with q_cur; y_dim in {1, 3, 8, 11}"""
    N = 1 if algo == "globalmcmc" else 5
    k = 0
    for d in range(1, 9):
        for qsrc in QSRC:
            select_twin(hip, oracle, algo, N, d, (1, 3, 8, 11)[k % 4], CHAIN_COUNTS[k % 6], qsrc)
            k += 1
    for yd in (1, 3, 8, 11):
        select_twin(hip, oracle, algo, N, 12, yd, 257, "q_cur")


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["glmcmc", "glmala"])
def test_hip_select_flags_and_n_valid(hip, oracle, algo):
    """GLABC_FLAG_LOCAL set and clear (log_weight_old refreshed or carried; the bit is cleared on the global branch and set by an
    accepted GLMCMC local move only); n_valid in {-1, 0 .. N, N + 3}, ignored on the local branch"""
    for N in (1, 6, 16, 17):
        for flags_mode in ("set", "clear", "mix"):
            for nv in (None, "all"):
                select_twin(hip, oracle, algo, N, 3, 3, 300, "q_cur" if N % 2 else "gauss", flags_mode=flags_mode, n_valid=nv)
    case = balanced_select_cases(oracle, algo, 6, 3, 3, 300, "q_cur", n_valid="all")[0]
    _, want = case.run(oracle, "oracle")
    nv, isg = case.bufs["n_valid"], case.bufs["is_global"]
    local_moves = moved_of(case, want) & (isg == 0) & (nv <= 0)
    assert local_moves.sum() > 3                                   # local-branch chains move whatever n_valid says
    assert not (moved_of(case, want) & (isg == 1) & (nv <= 0)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["glmcmc", "globalmcmc", "glmala"])
def test_hip_select_optional_outputs(hip, oracle, algo):
    """n_moves / history / moments given and NULL, hist_stride > n_chains, stride > n_chains, and step0_device = step0 + 2
    addressing history row 2 alone"""
    N = 1 if algo == "globalmcmc" else 4
    for n in (63, 256, 257):
        for kw in (dict(n_moves=False), dict(hist=False), dict(moments=False), dict(n_moves=False, hist=False, moments=False),
                   dict(hist_pad=7), dict(pad=5), dict(pad=5, hist_pad=3), dict(step_dev=5), dict(step_dev=5, hist_pad=7),
                   dict(chain0=2 ** 40 + 7)):
            select_twin(hip, oracle, algo, N, 3, 2, n, "q_cur", **kw)


# ================================================================================================== the twins, on the CPU
def expf(oracle, x):
    x = np.ascontiguousarray(x, F32)
    o = np.empty_like(x)
    oracle.oracle_expf_v(x.ctypes.data, x.size, o.ctypes.data)
    return o


def restate_select(oracle, case):
    """glabc_select as include/glabc.h and DESIGN.md 4.1f state it, chain by chain, on the inputs of `case` -> dict of the
    outputs in their logical shapes.  float32 arithmetic is numpy's on float32 scalars, in the stated association order; the
    normalising sum is torch.sum taken live (from 18 terms on: the checker's torch.sum order, which primitives.npz pins)."""
    b = {k: v.copy() for k, v in case.bufs.items()}
    n, N_all, d, yd, S = case.n, case.N, case.d, case.yd, case.stride
    algo = case.algo
    isir = algo in (A.ALGO_GLMCMC, A.ALGO_GLMALA)
    if "q_cur" in b:
        q_state = b["q_cur"]
    else:
        q_state = np.zeros(n, F32)
        rows = np.ascontiguousarray(b["theta"][:, :n].T)
        assert oracle.oracle_dist_log_prob(C.byref(case.glob), rows.ctypes.data, n, q_state.ctypes.data) == 0
    P, K, Q = b["prior_prop"], b["kern_prop"], b["log_q"]
    step = int(b["step_dev"][0]) if "step_dev" in b else case.step0
    err = np.errstate(all="ignore")
    err.__enter__()
    for c in range(n):
        glob = bool(b["is_global"][c] & 1)
        N = N_all
        if "n_valid" in b and glob:
            N = min(max(int(b["n_valid"][c]), 0), N_all)
        prior_c, kern_c = b["prior_cur"][c], b["kern_cur"][c]
        ind = 0
        lw = None
        if isir and glob:
            if b["flags"][0, c] & 1:                                                      # GLMCMC.py:60-64
                b["log_w"][0, c] = F32(F32(prior_c + kern_c) - q_state[c])
            b["flags"][0, c] &= ~1                                                        # :65
            rows = np.arange(N) * n + c
            lw = np.concatenate([b["log_w"][0, c:c + 1], ((P[rows] + K[rows]) - Q[rows]).astype(F32)])      # :74-75
            w = expf(oracle, lw)                                                          # :78
            w[np.isnan(w)] = F32(0)                                                       # :80-81
            if len(w) <= 17:
                tot = torch.sum(torch.from_numpy(w)).numpy()[()]                          # :82
            else:
                tot = F32(oracle.oracle_aten_rowsum_f32(w.ctypes.data, len(w)))
            wn = (w / tot).astype(F32)
            s, ind = 0.0, None
            for k, x in enumerate(wn.tolist()):                                           # :17-22, Python floats
                s = s + x
                if b["u_res"][c] < s:
                    ind = k
                    break
            ind = ind or 0                                                                # None -> stay, :84
        else:
            pk = F32(P[c] + K[c])
            if algo == A.ALGO_GLOBALMCMC and glob:
                log_acc = F32(F32(F32(F32(pk + q_state[c]) - Q[c]) - prior_c) - kern_c)   # GlobalMCMC.py:44-46
            elif algo == A.ALGO_GLMALA:
                log_acc = F32(F32(F32(pk + Q[c]) - prior_c) - kern_c)                     # GLMALA.py:190-193
            else:
                log_acc = F32(F32(pk - prior_c) - kern_c)                                 # GLMCMC.py:96-97
            ind = 1 if b["log_u"][c] < log_acc else 0
        old = b["theta"][:, c].copy()
        if ind > 0:
            r = (ind - 1) * n + c
            b["theta"][:, c] = b["theta_prop"][r]
            b["y"][:, c] = b["y_prop"][r]
            b["prior_cur"][c], b["kern_cur"][c] = P[r], K[r]
            if isir and glob:
                b["log_w"][0, c] = lw[ind]
            elif isir and algo == A.ALGO_GLMCMC:
                b["flags"][0, c] |= 1
            if "n_moves" in b:
                b["n_moves"][0, c] += 1
            b["is_global"][c] |= 2
        new = b["theta"][:, c]
        if "history" in b:
            b["history"][(step - case.step0) if "step_dev" in b else 0, :, c] = new
        if "sum_theta" in b:
            k = 0
            for p in range(d):
                b["sum_theta"][p, c] += float(new[p])
                for q in range(p, d):
                    b["sum_outer"][k, c] += float(new[p]) * float(new[q])
                    b["sum_jump"][k, c] += (float(new[p]) - float(old[p])) * (float(new[q]) - float(old[q]))
                    k += 1
    err.__exit__(None, None, None)
    return b


def hold_select_to_restatement(oracle, case):
    rc, want = case.run(oracle, "oracle")
    assert rc == 0
    case.check_ownership(want, "oracle")
    mine = restate_select(oracle, case)
    for k in case.bufs:
        if not np.array_equal(raw(case.body(want, k)), raw(mine[k])):
            bad = np.argwhere(raw(case.body(want, k)) != raw(mine[k]))[0]
            raise AssertionError("oracle_select and the restatement differ in %s at %s (%s)" % (k, bad, case.what()))
    return moved_of(case, want)


@pytest.mark.parametrize("algo", ["glmcmc", "globalmcmc", "glmala"])
def test_oracle_select_equals_the_plain_restatement(oracle, algo):
    """every decision, every moved state, every carried term, counter, history row and streaming sum of oracle_select equals
    the restatement's, no chain excluded: n_prop 1..16 with the planted chains (all weights 0, a NaN prior, a +inf weight,
    u = 0 against a zero first weight, u = 1 - 2^-53, log u = -inf, a NaN and a +inf acceptance ratio), 17 / 40 / 511 with the
    checker's torch.sum, n_valid, every source of q(Theta_old), a device iteration index"""
    sizes = (1,) * 4 if algo == "globalmcmc" else tuple(range(1, 17)) + (17, 40, 511)
    moved = stayed = 0
    for i, N in enumerate(sizes):
        n = 70 if N > 40 else (63, 257, 300)[i % 3]
        kw = dict(n_valid="all" if i % 3 == 1 else None, flags_mode=("mix", "set", "clear")[i % 3])
        if i % 5 == 4:
            kw.update(step_dev=5, hist_pad=3, pad=5)
        for case in balanced_select_cases(oracle, algo, N, 1 + i % 8, (1, 3, 8, 11)[i % 4], n, QSRC[i % 4], **kw):
            m = hold_select_to_restatement(oracle, case)
            moved, stayed = moved + int(m.sum()), stayed + int((~m).sum())
            # the planted chains did what the reference's lines do with such numbers
            glob_isir = algo != "globalmcmc"
            if glob_isir:
                assert not m[0] and not m[2]                      # 0/0 and inf/inf: no index, the chain stays
                assert m[3] or N == 0                             # u = 0, first weight 0: the first candidate with weight > 0
            assert m[5] and not m[6] and m[7]                     # log u = -inf accepts, NaN never does, +inf always
            if not glob_isir:
                assert m[8] and not m[9] and m[10]
    assert moved > 100 and stayed > 100
    for case in balanced_select_cases(oracle, algo, 1, 2, 2, 1, "q_cur"):
        hold_select_to_restatement(oracle, case)


def philox(oracle, chain, step, slot, seed):
    ctr = np.array([chain & 0xFFFFFFFF, chain >> 32, step, slot], np.uint32)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint32)
    out = np.zeros(4, np.uint32)
    oracle.oracle_philox4x32_10(ctr.ctypes.data, key.ctypes.data, out.ctypes.data)
    return out


def noise_of_words(oracle, words, uniform):
    """8 Philox words -> 8 proposal draws: Box-Muller on the pairs (0,1), (2,3) ..., or one [0,1) uniform per word"""
    words = np.ascontiguousarray(words, np.uint32)
    if uniform:
        u, up, u64 = np.zeros(8, F32), np.zeros(8, F32), np.zeros(8)
        oracle.oracle_uniforms_v(words.ctypes.data, words.ctypes.data, 8, u.ctypes.data, up.ctypes.data, u64.ctypes.data)
        return u
    a, b_ = np.ascontiguousarray(words[0::2]), np.ascontiguousarray(words[1::2])
    z0, z1 = np.zeros(4, F32), np.zeros(4, F32)
    oracle.oracle_normal_pair_v(a.ctypes.data, b_.ctypes.data, 4, z0.ctypes.data, z1.ctypes.data)
    return np.stack([z0, z1], 1).reshape(8)


def forward(oracle, dist, noise_rows):
    noise_rows = np.ascontiguousarray(noise_rows, F32)
    z, lp = np.zeros_like(noise_rows), np.zeros(len(noise_rows), F32)
    assert oracle.oracle_dist_forward(C.byref(dist), noise_rows.ctypes.data, len(noise_rows), z.ctypes.data, lp.ctypes.data) == 0
    return z, lp


@pytest.mark.parametrize("d,nd,N,n,lk,gk,kw", [
    (2, 2, 5, 63, "gauss", "gauss", {}),
    (3, 3, 2, 70, "gauss", "gauss", dict(chain0=2 ** 32 - 3, pad=5)),
    (1, 4, 16, 17, "gauss", "gauss", dict(seed=0x9E3779B97F4A7C15)),
    (8, 8, 3, 20, "gauss", "gauss", dict(step_dev=9)),
    (5, 1, 17, 9, "gauss", "gauss", dict(chain0=2 ** 40 + 7)),
    (4, 0, 4, 33, "uniform", "uniform", {}),
    (7, 5, 2, 33, "uniform", "gauss", {}),
])
def test_oracle_propose_equals_step_draws_and_forward(oracle, d, nd, N, n, lk, gk, kw):
    """oracle_propose against the draws the fused samplers consume (oracle_step_draws: branch / accept / resampling numbers,
    the candidates' normals) pushed through forward() (oracle_dist_forward); a Uniform proposal's [0,1) draws come from the
    candidate's Philox words"""
    rng = np.random.default_rng(d + N)
    case = propose_case("glmcmc", d, nd, N, n, lk, gk, rng, gf=0.55, **kw)
    rc, want = case.run(oracle, "oracle")
    assert rc == 0
    propose_finish(case, want)
    case.check_ownership(want, "oracle")
    step = kw.get("step_dev", case.step0)
    dp = d + (d & 1)
    spp = (dp + nd + 3) // 4
    theta_prop, log_q = case.body(want, "theta_prop"), case.body(want, "log_q")
    seen = set()
    for c in range(n):
        chain = case.chain0 + c
        u2, r, z = np.zeros(2, F32), np.zeros(1), np.zeros((N, d + nd), F32)
        oracle.oracle_step_draws(case.seed, chain, step, N, d, nd, u2.ctypes.data, r.ctypes.data, z.ctypes.data)
        isg = int(u2[0] < F32(0.55))
        seen.add(isg)
        assert case.body(want, "is_global")[c] == isg
        lu = np.zeros(1, F32)
        oracle.oracle_logf_v(u2[1:].ctypes.data, 1, lu.ctypes.data)
        assert raw(case.body(want, "log_u"))[c] == raw(lu)[0]
        assert raw(case.body(want, "u_res"))[c] == raw(r)[0]
        rows = np.arange(N) * n + c
        if nd:
            assert np.array_equal(raw(case.body(want, "sim_noise")[rows]), raw(z[:, d:]))
        e = z[:, :d].copy()
        for j in range(N):
            g = case.local if (j == 0 and not isg) else case.glob
            if g.kind == A.DIST_UNIFORM:
                words = np.concatenate([philox(oracle, chain, step, 1 + j * spp + b, case.seed) for b in range(min(spp, 2))] +
                                       [np.zeros(4, np.uint32)])[:8]
                e[j] = noise_of_words(oracle, words, True)[:d]
        zg, lq = forward(oracle, case.glob, e)
        if not isg:
            zl, _ = forward(oracle, case.local, e[:1])
            zg[0] = zl[0] + case.bufs["theta"][:, c]                                # Theta_old + increment, GLMCMC.py:91
            lq[0] = 0.0
        assert np.array_equal(raw(theta_prop[rows]), raw(zg)), c
        assert np.array_equal(raw(log_q[rows]), raw(lq)), c
    assert seen == {0, 1}


@pytest.mark.parametrize("d,lk,rnd,kw", [(1, "gauss", 1, {}), (2, "uniform", 2, dict(chain0=2 ** 32 - 3)), (3, "gauss", 7, dict(pad=5)),
                                          (5, "uniform", 2 ** 24, dict(step_dev=6)), (8, "gauss", 2, dict(seed=0x9E3779B97F4A7C15)),
                                          (4, "gauss", 3, dict(chain0=2 ** 40 + 7))])
def test_oracle_redraw_equals_the_slot_rule(oracle, d, lk, rnd, kw):
    """oracle_propose_redraw: the chains on the local branch whose prior is exactly the sentinel, their increment from Philox
    blocks GLABC_SLOT_REDRAW + 2*round + b (b = 0, 1) of (chain, iteration), forward() of `local`, + Theta_old; nothing else"""
    rng = np.random.default_rng(d)
    n = 70
    case = redraw_case(d, lk, rnd, n, rng, **kw)
    rc, want = case.run(oracle, "oracle")
    assert rc == 0
    redraw_finish(case, want)
    case.check_ownership(want, "oracle")
    step = kw.get("step_dev", case.step0)
    got = case.body(want, "theta_prop")
    for c in np.flatnonzero(case.redraw):
        chain = case.chain0 + int(c)
        words = np.concatenate([philox(oracle, chain, step, A.SLOT_REDRAW + 2 * rnd + b, case.seed) for b in (0, 1)])
        e = noise_of_words(oracle, words, lk == "uniform")[:d]
        z, _ = forward(oracle, case.local, e[None])
        assert np.array_equal(raw(got[c]), raw((z[0] + case.bufs["theta"][:, c]).astype(F32))), c
