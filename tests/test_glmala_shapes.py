"""GLMALA (glabc_glmala_steps / glabc_glmala_init) at every shape it is compiled for: theta_dim 1 .. 4 x batch size 1 .. 16 x the
two square-root variants -- 128 glmala_kernel instantiations plus the theta_dim 2 team kernels.

theta_dim 2 has a gradient path of its own (glabc_mala.h coop_gradient_flat2, the team kernels); 1, 3 and 4 run the general
branch of coop_gradient: the chains of a wavefront that need a gradient are dealt to lane groups of G = 64 / 2^ceil(log2 n)
lanes through a rank table in LDS, the lanes of a group split the num_grad simulations, merge exact partial sums with
xor-shuffles and hand the result back to the owner.  G changes from iteration to iteration with the number of chains on the
local branch, so this file computes G from the checker's branch draws and ASSERTS that its inputs reach every width, with
num_grad below, at and above it -- a condition on the inputs, checked without a GPU.

Every comparison is with the CPU checker (itself pinned to the reference at 1, 3 and 4 parameters by
tests/test_oracle_golden.py and tests/golden/glmala_philox_dim*_ieee.npz), bit for bit, on every array the entry points own:
history, theta / y, the float64 state, the cached gradient, flags, n_moves and the three moment sums.  Device buffers start
as canaries (helpers.py), their padding columns (stride > n_chains) included: after GLABC_OK no owned element may still hold
one, padding always must, and after a refusal every buffer is what it was.  n_moves and the moment sums are accumulators the
kernel adds to, so their owned columns start at zero; the checker's sums they are compared with are not zero.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle_lib
from glabcmcmc_amd import _capi as A
from helpers import (GLMALA_GOLDENS_DIMS, AbsGaussModel, bits, bits64, canary_f32, canary_f64, canary_i32, canary_left, descriptors,
                     dev, host, load_golden, mala_params)

ERR_DIM, ERR_KIND, ERR_ARG = -2, -3, -4          # glabc_status, include/glabc.h
N_CHAINS = 130                                   # two full wavefronts and two lanes of a third
WIDTHS = (1, 2, 4, 8, 16, 32, 64)


# --------------------------------------------------------------------------------------------------------- inputs
def y_obs_of(d, kind):
    """'away': every |y_obs_j| well above 2^-6; 'edge': one exactly (-)2^-6, still the lean square root; 'zero' / 'tiny': one
    coordinate 0 / 1e-3, the kernels with the general square root (glabc_pack.h y_obs_away)"""
    y = [1.5, 0.8, 1.0, 0.5][:d]
    j = (d - 1) // 2
    if kind != "away":
        y[j] = {"edge": -0.015625 if d & 1 else 0.015625, "zero": 0.0, "tiny": 1e-3}[kind]
    return y


def lean(y_obs):
    return all(abs(np.float32(v)) >= np.float32(2.0 ** -6) for v in y_obs)


def make_case(d, N, n=N_CHAINS, **over):
    """The configuration of grid point (theta_dim d, batch size N): the other parameters are mixed over the grid"""
    T = (40, 50, 60)[N % 3]
    c = dict(d=d, N=N, n=n, T=T,
             gf=(0.5, 0.3, 0.8, 0.0, 0.65, 1.0)[(N + 2 * d) % 6],
             uniform=(N + d) % 3 == 0,
             num=(2, 3, 31, 64, 65, 100)[(5 * N + d) % 6],
             y_kind=("zero", "away", "tiny", "edge")[N % 4],
             spl=(7, 13, 17)[(N + d) % 3],                            # none divides 40, 50 or 60
             chain0=(N << 33) + d * 1000003,                          # above 2^32: both Philox counter words in use
             pad=(N % 3) * 3, hist_pad=(d - 1) * 2,
             eps=0.3, tau=0.25, seed=(d * 7919 + N) * 2654435761 + 12345, lanes=0)
    c.update(over)
    return c


def case_id(c):
    return "d%d-N%d-gf%g-%s-num%d-%s%s" % (c["d"], c["N"], c["gf"], "uni" if c["uniform"] else "gauss", c["num"], c["y_kind"],
                                          "-lanes%d" % c["lanes"] if c["lanes"] else "")


def case_descriptors(c):
    d = c["d"]
    glob = ("uniform", [-3.0] * d, [3.0] * d) if c["uniform"] else ("gauss", [0.1 * j for j in range(d)], [1.0 + 0.1 * j for j in range(d)])
    cfg = dict(epsilon=c["eps"], tau=c["tau"], num_grad=c["num"], y_obs=c.get("y_obs") or y_obs_of(d, c["y_kind"]),
               local=("gauss", [0.0] * d, [0.35] * d), **{"global": glob})
    model, _, gd = descriptors(cfg)
    return model, gd, mala_params(cfg)


def case_inputs(c):
    rng = np.random.default_rng(c["seed"] % (1 << 32))
    theta0 = rng.standard_normal((c["n"], c["d"])).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((c["n"], c["d"]))).astype(np.float32)
    return theta0, y0


GRID = [make_case(d, N) for d in (1, 2, 3, 4) for N in range(1, 17)]
GRID_GPU = [c for c in GRID if c["d"] != 2] + [dict(c, lanes=l) for c in GRID if c["d"] == 2 for l in (1, 2)]


# --------------------------------------------------------------------------------------------------------- checker
def checker_run(oracle, c, theta0, y0):
    """oracle_glmala_init + oracle_glmala_steps -> every array the device entry points own"""
    n, d, T = theta0.shape[0], c["d"], c["T"]
    model, glob, mala = case_descriptors(c)
    hc = oracle_lib.HostChains(theta0, y0, chain0=c["chain0"]).add_mala_state()
    hist = np.zeros((T, d, n), np.float32)
    mom = oracle_lib.HostMoments(n, d)
    run, keep = oracle_lib.make_run(seed=c["seed"], step0=1, n_steps=T, gf=c["gf"], batch=c["N"], history=hist, moments=mom)
    cs = hc.struct()
    assert oracle.oracle_glmala_init(C.byref(model), C.byref(cs)) == 0
    assert oracle.oracle_glmala_steps(C.byref(model), C.byref(glob), C.byref(mala), C.byref(cs), C.byref(run)) == 0
    return dict(history=hist, theta=hc.theta, y=hc.y, log_w=hc.log_w, theta64=hc.theta64, y64=hc.y64, log_w64=hc.log_w64,
                grad=hc.grad, flags=hc.flags, n_moves=hc.n_moves, sum_theta=mom.sum_theta, sum_outer=mom.sum_outer,
                sum_jump=mom.sum_jump)


_checker_cache = {}


def checker_case(oracle, c):
    key = tuple(sorted((k, repr(v)) for k, v in c.items() if k not in ("lanes", "spl", "pad", "hist_pad")))
    if key not in _checker_cache:
        _checker_cache[key] = checker_run(oracle, c, *case_inputs(c))
    return _checker_cache[key]


@functools.lru_cache(maxsize=None)
def _branch_uniforms(seed, chain0, n, T):
    L = oracle_lib.load()
    u = np.zeros((T, n), np.float32)
    u2, r, z = np.zeros(2, np.float32), np.zeros(1, np.float64), np.zeros(2, np.float32)
    for i in range(n):
        for t in range(T):
            L.oracle_step_draws(seed, chain0 + i, t + 1, 1, 1, 1, u2.ctypes.data, r.ctypes.data, z.ctypes.data)
            u[t, i] = u2[0]
    return u


def local_steps(c):
    """[T][n] bool: chain i takes the MALA move at iteration t (GLMALA.py:151: the branch uniform -- word 0 of the
    iteration's head block, the same for every theta_dim -- against float32 gf)"""
    return ~(_branch_uniforms(c["seed"], c["chain0"], c["n"], c["T"]) < np.float32(c["gf"]))


def width_of(count):
    G = 64
    while G * count > 64:
        G >>= 1
    return G


def gradient_widths(c):
    """The lane-group widths the two coop_gradient calls of mala_move meet in this run: g = 1 (the gradient at the proposal) is
    needed by every chain of the wavefront on the local branch, g = 0 (at the current state) only by those on their FIRST
    local step.  -> ({G of g = 0}, {G of g = 1})"""
    loc = local_steps(c)
    first = loc & (np.cumsum(loc, axis=0) == 1)
    out = []
    for need in (first, loc):
        counts = {int(v) for w in range(0, c["n"], 64) for v in need[:, w:w + 64].sum(1)}
        out.append({width_of(v) for v in counts if v > 0})
    return tuple(out)


def assert_live(c, ref):
    """the case is not idle (conditions on the checker's run alone)"""
    loc = local_steps(c)
    assert ref["n_moves"].sum() > 0 and (ref["n_moves"] > 0).mean() > 0.5
    assert (ref["sum_outer"][0] > 0).all() and (ref["sum_jump"].sum(0) > 0).any()
    if c["gf"] < 1:
        assert (ref["flags"] & A.FLAG_TH64).any() and (ref["flags"] & A.FLAG_HAS_GRAD).any()
        assert loc.any()
    if 0 < c["gf"] < 1:
        assert (~loc).any()
    # FLAG_HAS_GRAD = the chain has taken a local step: its first computed two gradients (g = 0, 1), later ones one
    assert np.array_equal((ref["flags"] & A.FLAG_HAS_GRAD) != 0, loc.any(0))
    if c["gf"] < 1 and c["T"] > 1:
        assert (loc.sum(0) >= 2).any()


# --------------------------------------------------------------------------------------------------------- device
class DeviceRun:
    """Every buffer of one glabc_glmala_init + glabc_glmala_steps run, canaries where the entry points are to write"""

    OWNED = ("history", "log_w", "flags", "theta64", "y64", "log_w64", "grad")       # start as canaries in the owned columns too

    def __init__(self, theta0, y0, T, chain0=0, pad=0, hist_pad=0, moments=True, history=True, n_moves=True):
        n, d = theta0.shape
        yd = y0.shape[1]
        self.n, self.d, self.yd, self.T, self.chain0 = n, d, yd, T, chain0
        S = self.S = n + pad
        self.HS = n + hist_pad
        tri = d * (d + 1) // 2
        h = dict(theta=canary_f32(d, S), y=canary_f32(yd, S), log_w=canary_f32(S), flags=canary_i32(S),
                 theta64=canary_f64(d, S), y64=canary_f64(yd, S), log_w64=canary_f64(S), grad=canary_f64(d, S))
        h["theta"][:, :n], h["y"][:, :n] = theta0.T, y0.T
        if n_moves:
            h["n_moves"] = canary_i32(S)
            h["n_moves"][:n] = 0
        if history:
            h["history"] = canary_f32(T, d, self.HS)
        if moments:
            for k, rows in (("sum_theta", d), ("sum_outer", tri), ("sum_jump", tri)):
                h[k] = canary_f64(rows, S)
                h[k][:, :n] = 0.0
        self.before = {k: v.copy() for k, v in h.items()}
        self.g = {k: dev(v) for k, v in h.items()}

    def chains(self):
        g = self.g
        return A.Chains(self.n, self.chain0, self.S, g["theta"].data_ptr(), g["y"].data_ptr(), g["log_w"].data_ptr(),
                        g["flags"].data_ptr(), g["n_moves"].data_ptr() if "n_moves" in g else None, g["theta64"].data_ptr(),
                        g["y64"].data_ptr(), g["log_w64"].data_ptr(), g["grad"].data_ptr())

    def init(self, hip, model):
        cs = self.chains()
        return hip.glabc_glmala_init(C.byref(model), C.byref(cs), None)

    def steps(self, hip, model, glob, mala, seed, gf, N, spl=None, lanes=0, edit=None):
        """the T iterations in launches of `spl`; `edit(run)` changes the glabc_run of every launch (refusals)"""
        cs = self.chains()
        ms = A.Moments(*(self.g[k].data_ptr() for k in ("sum_theta", "sum_outer", "sum_jump"))) if "sum_theta" in self.g else None
        done = 0
        while done < self.T:
            k = min(spl or self.T, self.T - done)
            run = A.Run()
            run.seed, run.step0, run.n_steps, run.global_frequency, run.batch_size = seed, 1 + done, k, gf, N
            run.lanes_per_chain = lanes
            if "history" in self.g:
                run.history, run.hist_stride = self.g["history"][done].data_ptr(), self.HS
            if ms is not None:
                run.moments = C.pointer(ms)
            if edit is not None:
                edit(run)
            rc = hip.glabc_glmala_steps(C.byref(model), C.byref(glob), C.byref(mala), C.byref(cs), C.byref(run), None)
            if rc != 0:
                return rc
            done += k
        return 0

    def fetch(self):
        return {k: host(v) for k, v in self.g.items()}

    def assert_unchanged(self):
        for k, v in self.fetch().items():
            assert np.array_equal(v.view(np.uint8), self.before[k].view(np.uint8)), "a refused call wrote to `%s`" % k

    def result(self):
        """the owned columns after GLABC_OK: nothing the entry points own is a canary, every padding column still is"""
        out, n = {}, self.n
        for k, v in self.fetch().items():
            own, padding = v[..., :n], v[..., n:]
            assert canary_left(padding) == padding.size, "`%s`: %d padding elements were written" % (k, padding.size - canary_left(padding))
            assert canary_left(own) == 0, "`%s`: %d of %d owned elements still hold the canary" % (k, canary_left(own), own.size)
            out[k] = np.ascontiguousarray(own)
        return out


def device_case(hip, c, theta0, y0, **kw):
    model, glob, mala = case_descriptors(c)
    opts = dict(chain0=c["chain0"], pad=c["pad"], hist_pad=c["hist_pad"])
    opts.update({k: kw.pop(k) for k in ("chain0", "pad", "hist_pad", "moments", "history", "n_moves") if k in kw})
    r = DeviceRun(theta0, y0, c["T"], **opts)
    assert r.init(hip, model) == 0
    assert r.steps(hip, model, glob, mala, c["seed"], c["gf"], c["N"], spl=kw.pop("spl", c["spl"]), lanes=kw.pop("lanes", c["lanes"])) == 0
    assert not kw
    return r.result()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return bits(a) == bits(b)
    if a.dtype == np.float64:
        return bits64(a) == bits64(b)
    return a.astype(np.uint32) == b.astype(np.uint32)


def assert_equal_runs(got, want, what):
    for k in got:
        same = same_bits(got[k], want[k])
        assert same.all(), "%s: `%s` differs in %d of %d elements, first at index %s" % (
            what, k, (~same).sum(), same.size, tuple(np.argwhere(~same)[0]))


# ------------------------------------------------------------------------- the grid is live, and reaches every width (CPU)
@pytest.mark.parametrize("d", (1, 2, 3, 4))
def test_grid_walks_every_compiled_shape_and_is_not_idle(oracle, d):
    """The parameter grid of test_hip_glmala_every_compiled_shape through the checker alone: every batch size 1 .. 16, each
    square-root variant with a batch size <= 8 and >= 9, every num_grad / gf / proposal kind somewhere, accepted moves in every
    case, the float64 switch and a cached gradient wherever gf < 1, both branches wherever 0 < gf < 1."""
    cases = [c for c in GRID if c["d"] == d]
    assert [c["N"] for c in cases] == list(range(1, 17))
    for variant in (True, False):
        ns = [c["N"] for c in cases if lean(y_obs_of(d, c["y_kind"])) == variant]
        assert min(ns) <= 8 and max(ns) >= 9
    assert {c["y_kind"] for c in cases} == {"zero", "away", "tiny", "edge"}
    assert {c["num"] for c in cases} == {2, 3, 31, 64, 65, 100} and {c["uniform"] for c in cases} == {True, False}
    assert {c["gf"] for c in cases} >= {0.0, 0.5, 1.0}
    for c in cases:
        assert c["T"] % c["spl"] != 0 and c["chain0"] > 2 ** 32
        assert_live(c, checker_case(oracle, c))
        if 0 < c["gf"] < 1:                                              # an iSIR move from a float64 state: the float64 weights
            assert (checker_case(oracle, c)["flags"] & A.FLAG_LW64).any()
    assert any(c["pad"] for c in cases) and any(not c["pad"] for c in cases)


def geometry_runs(d):
    """(chains, gf, num_grad, batch size) of test_hip_glmala_gradient_lane_groups: chosen so that every lane-group width occurs
    with num_grad on both sides of it (test_gradient_lane_group_widths_are_all_reached)"""
    runs = [(130, 0.0, 3, 2), (130, 0.6, 100, 3), (130, 0.6, 2, 9), (130, 0.8, 5, 4), (130, 0.9, 12, 1), (130, 0.95, 31, 5),
            (130, 0.97, 33, 16), (64, 0.985, 64, 2), (65, 0.985, 65, 3), (63, 0.9, 17, 6), (2, 0.3, 33, 7), (1, 0.5, 63, 8)]
    return [make_case(d, N, n=n, gf=gf, num=num, T=50, y_kind=("tiny", "away")[i % 2], uniform=i % 3 == 1, spl=17, pad=i % 2, hist_pad=0,
                      chain0=(i << 34) + d, seed=1000 * d + i)
            for i, (n, gf, num, N) in enumerate(runs)]


@pytest.mark.parametrize("d", (1, 3, 4))
def test_gradient_lane_group_widths_are_all_reached(oracle, d):
    """A condition on the inputs of test_hip_glmala_gradient_lane_groups, from the checker's branch draws: both gradient calls of
    mala_move meet every lane-group width G in {1, 2, 4, 8, 16, 32, 64}; every G >= 4 occurs in a run whose num_grad is below G
    (lanes of a group without a simulation) and in one whose num_grad is above G (more than one round per lane); G = 64 also with
    num_grad = 64 and 65; full, partial and single-chain wavefronts occur."""
    cases = geometry_runs(d)
    seen = [(c, gradient_widths(c)) for c in cases]
    for g in (0, 1):
        assert set().union(*(w[g] for _, w in seen)) == set(WIDTHS), "gradient call g = %d" % g
    for G in WIDTHS[2:]:
        nums = {c["num"] for c, w in seen if G in w[0] | w[1]}
        assert min(nums) < G < max(nums), (G, nums)
    nums64 = {c["num"] for c, w in seen if 64 in w[1]}
    assert {64, 65} <= nums64
    assert {c["n"] for c in cases} >= {1, 2, 63, 64, 65, 130}
    for c in cases:
        assert_live(c, checker_case(oracle, c))


# ---------------------------------------------------------------------------------------- (a) every compiled shape
@pytest.mark.gpu
@pytest.mark.parametrize("c", GRID_GPU, ids=case_id)
def test_hip_glmala_every_compiled_shape(hip, oracle, c):
    """glmala_kernel<D, N, LEAN> for D = 1 .. 4, N = 1 .. 16, both LEAN (theta_dim 2: one and two wavefronts per 64 chains) against
    the checker: history, final state in both precisions, cached gradient, flags, move counts, the three moment sums."""
    want = checker_case(oracle, c)
    assert_live(c, want)
    got = device_case(hip, c, *case_inputs(c))
    assert set(got) == set(want)
    assert_equal_runs(got, want, case_id(c))


# ------------------------------------------------------------------------------------ (b) lane groups of the gradient
@pytest.mark.gpu
@pytest.mark.parametrize("i", range(12))
@pytest.mark.parametrize("d", (1, 3, 4))
def test_hip_glmala_gradient_lane_groups(hip, oracle, d, i):
    """The general branch of coop_gradient at every lane-group width (test_gradient_lane_group_widths_are_all_reached says
    which run reaches which): 1, 2, 63, 64, 65 and 130 chains, num_grad below, at and above the width."""
    c = geometry_runs(d)[i]
    want = checker_case(oracle, c)
    got = device_case(hip, c, *case_inputs(c))
    assert_equal_runs(got, want, case_id(c) + " widths %s" % (gradient_widths(c),))
    # from the device's own flags: who has a cached gradient is who took a local step
    assert np.array_equal((got["flags"] & A.FLAG_HAS_GRAD) != 0, local_steps(c).any(0))


# --------------------------------------------------------------------------------------- (c) geometry is only geometry
@pytest.mark.gpu
@pytest.mark.parametrize("d", (1, 3, 4))
def test_hip_glmala_launch_geometry_never_changes_results(hip, oracle, d):
    """lanes_per_chain 0 / 1 / 2 (theta_dim 2's knob: accepted and without effect elsewhere), 1 / 7 / T iterations per launch, one
    launch against two shards cut at a non-multiple of 64, padded against dense strides, with and without moments / history /
    n_moves: every array both runs produce is the same, bit for bit."""
    c = make_case(d, 4, gf=0.6, num=31, T=30, y_kind="tiny", spl=30, pad=0, hist_pad=0, seed=77 + d)
    theta0, y0 = case_inputs(c)
    base = device_case(hip, c, theta0, y0)
    assert_equal_runs(base, checker_case(oracle, c), "base")
    variants = [dict(lanes=1), dict(lanes=2), dict(spl=1), dict(spl=7), dict(pad=5, hist_pad=0), dict(pad=0, hist_pad=9),
                dict(pad=62, hist_pad=3), dict(moments=False), dict(history=False), dict(n_moves=False),
                dict(moments=False, history=False, n_moves=False, spl=7)]
    for kw in variants:
        got = device_case(hip, c, theta0, y0, **dict(kw))
        assert set(got) == set(base) - ({"sum_theta", "sum_outer", "sum_jump"} if kw.get("moments") is False else set()) \
            - ({"history"} if kw.get("history") is False else set()) - ({"n_moves"} if kw.get("n_moves") is False else set())
        assert_equal_runs(got, base, str(kw))
    cut = 50
    parts = [device_case(hip, c, theta0[lo:hi], y0[lo:hi], chain0=c["chain0"] + lo, pad=pad)
             for lo, hi, pad in ((0, cut, 3), (cut, c["n"], 0))]
    joined = {k: np.concatenate([p[k] for p in parts], axis=-1) for k in base}
    assert_equal_runs(joined, base, "two shards cut at chain %d" % cut)


# -------------------------------------------------------------------------------- (d) the reference's chains, d = 1, 3, 4
@pytest.mark.gpu
@pytest.mark.parametrize("name", GLMALA_GOLDENS_DIMS)
def test_hip_glmala_reproduces_reference_chains_off_two_parameters(hip, name):
    """The kernels against chains the reference's own GLMALA loop wrote at 1, 3 and 4 parameters (tests/golden/make_golden.py
    AbsGauss_set, correctly rounded torch.sqrt): bit for bit, and as many accepted moves."""
    g = load_golden(name)
    cfg = g["cfg"]
    model, _, glob = descriptors(cfg, g)
    r = DeviceRun(g["theta0"], g["y0"], cfg["T"], chain0=cfg.get("chain0", 0), pad=1, hist_pad=2)
    assert r.init(hip, model) == 0
    assert r.steps(hip, model, glob, mala_params(cfg), cfg["seed"], cfg["gf"], cfg["N"], spl=97) == 0
    out = r.result()
    got = np.concatenate([g["theta0"][None], out["history"].transpose(0, 2, 1)], axis=0)
    same = bits(got) == bits(g["chains"])
    assert same.all(), "first mismatch at (t, chain, dim) = %s of %d" % (np.argwhere(~same)[0], (~same).sum())
    moves = (np.diff(g["chains"], axis=0) != 0).any(-1).sum(0)
    assert np.array_equal(out["n_moves"].astype(np.uint32), moves.astype(np.uint32)) and moves.sum() > 0
    assert (out["flags"] & A.FLAG_TH64).any()


# ------------------------------------------------------------------------------------------------------ (e) refusals
@pytest.mark.gpu
def test_hip_glmala_refuses_what_is_not_compiled(hip):
    """theta_dim 5 .. 8 -> GLABC_ERR_DIM from both entry points, the g-and-k simulator -> GLABC_ERR_KIND, batch size 0 / 17,
    num_grad 1 / 65537, lanes_per_chain 3, a tape, GLABC_MATH_FAST and a per-chain gf array -> GLABC_ERR_ARG; no buffer changes."""
    from glabcmcmc_amd.examples.GK import GK_set
    rng = np.random.default_rng(5)
    n, T = 70, 3

    def attempt(model, glob, d, yd, N=4, num=10, edit=None, also_init=False):
        theta0 = rng.standard_normal((n, d)).astype(np.float32)
        r = DeviceRun(theta0, rng.standard_normal((n, yd)).astype(np.float32), T, pad=2, hist_pad=1)
        rcs = [r.steps(hip, model, glob, A.Mala(0.3, 0.09, 0.09, num, 0), 1, 0.5, N, edit=edit)]
        if also_init:
            rcs.append(r.init(hip, model))
        r.assert_unchanged()
        return rcs

    def gauss(d):
        return descriptors(dict(epsilon=0.3, dim=d, local=("gauss", [0.0] * d, [1.0] * d), **{"global": ("gauss", [0.0] * d, [1.0] * d)}))

    for d in (5, 6, 7, 8):
        model, _, glob = gauss(d)
        assert attempt(model, glob, d, d, also_init=True) == [ERR_DIM, ERR_DIM]
    _, _, glob4 = gauss(4)
    assert attempt(GK_set(1.0).descriptor(), glob4, 4, 8) == [ERR_KIND]
    spare = dev(np.zeros(4 * n * T * 16, np.float32))
    tape = A.Tape(spare.data_ptr(), spare.data_ptr(), spare.data_ptr(), 4, 0)

    def set_field(name, value):
        return lambda run: setattr(run, name, value)

    for d in (1, 3, 4):
        model, _, glob = gauss(d)
        assert attempt(model, glob, d, d, N=0) == [ERR_ARG] and attempt(model, glob, d, d, N=17) == [ERR_ARG]
        assert attempt(model, glob, d, d, num=1) == [ERR_ARG] and attempt(model, glob, d, d, num=65537) == [ERR_ARG]
        assert attempt(model, glob, d, d, edit=set_field("lanes_per_chain", 3)) == [ERR_ARG]
        assert attempt(model, glob, d, d, edit=set_field("tape", C.pointer(tape))) == [ERR_ARG]
        assert attempt(model, glob, d, d, edit=set_field("math_mode", A.MATH_FAST)) == [ERR_ARG]
        assert attempt(model, glob, d, d, edit=set_field("global_frequency_per_chain", spare.data_ptr())) == [ERR_ARG]
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- (f) the user-facing path
@pytest.mark.gpu
def test_glmala_function_with_a_three_parameter_descriptor_model_is_fused(hip, oracle):
    """glabcmcmc_amd.GLMALA with a user's descriptor Model of 3 parameters (a Mixture_set subclass with its own _likelihood /
    _prior / y_obs) runs glabc_glmala_steps: its chains are the checker's for the same seed."""
    import glabcmcmc_amd as g
    d, n, T, N, tau, num, gf, seed = 3, 70, 40, 5, 0.25, 9, 0.5, 2027
    m = AbsGaussModel(0.3, [1.5, 1.0, 0.8])
    ip = g.DiagGaussian(d, torch.zeros(d), torch.zeros(d))
    rng = np.random.default_rng(3)
    theta0 = rng.standard_normal((n, d)).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((n, d))).astype(np.float32)
    st = {}
    out = g.GLMALA(m, T + 1, torch.from_numpy(theta0), torch.from_numpy(y0), tau, num, None, gf, ip, N, seed=seed, verbose=False,
                   state_out=st)
    assert "callback_device" not in st and "chains" in st                # generic.run_glmala leaves callback_device
    assert out.shape == (T + 1, n, d) and out.dtype == torch.float32
    hc = oracle_lib.HostChains(theta0, y0).add_mala_state()
    hist = np.zeros((T, d, n), np.float32)
    run, keep = oracle_lib.make_run(seed=seed, step0=1, n_steps=T, gf=gf, batch=N, history=hist)
    model, imp, mala, cs = m.descriptor(), ip.descriptor(), A.Mala(tau, tau ** 2, 0.3 ** 2, num, 0), hc.struct()
    assert oracle.oracle_glmala_init(C.byref(model), C.byref(cs)) == 0
    assert oracle.oracle_glmala_steps(C.byref(model), C.byref(imp), C.byref(mala), C.byref(cs), C.byref(run)) == 0
    want = np.concatenate([theta0[None], hist.transpose(0, 2, 1)], axis=0)
    same = bits(out.numpy()) == bits(want)
    assert same.all(), "first mismatch at (t, chain, dim) = %s" % (np.argwhere(~same)[0],)
    assert hc.n_moves.sum() > 0 and np.array_equal(st["chains"].n_moves.cpu().numpy().astype(np.uint32), hc.n_moves)
    one = g.GLMALA(m, 30, torch.zeros(d), torch.tensor([[1.4, 1.1, 0.9]]), tau, num, None, gf, ip, N, seed=3, verbose=False)
    assert one.shape == (30, d)


@pytest.mark.gpu
def test_glmala_function_with_five_parameters_takes_the_callback_path(hip):
    """The same class with 5 parameters is beyond the fused kernels (generic.fused_supported max_dim = 4): GLMALA runs
    generic.run_glmala -- state_out says so -- and returns finite chains of the reference's shapes that move."""
    import glabcmcmc_amd as g
    d, n, T = 5, 40, 60
    m = AbsGaussModel(0.5, [1.5, 1.0, 0.8, 1.2, 0.6])
    ip = g.DiagGaussian(d, torch.zeros(d), torch.zeros(d))
    theta0 = torch.zeros(n, d) + 1.0
    st = {}
    out = g.GLMALA(m, T, theta0, m.generate_samples(theta0), 0.2, 10, None, 0.5, ip, 5, seed=11, verbose=False, state_out=st)
    assert "callback_device" in st and "has_grad" in st
    assert out.shape == (T, n, d) and out.dtype == torch.float32 and torch.isfinite(out).all()
    moved = (out[1:] != out[:-1]).any(-1)
    assert moved.any(0).float().mean() > 0.9
    one = g.GLMALA(m, 30, torch.zeros(d) + 1.0, m.generate_samples(torch.zeros(d) + 1.0), 0.2, 10, None, 0.5, ip, 5, seed=3,
                   verbose=False)
    assert one.shape == (30, d) and torch.isfinite(one).all()
