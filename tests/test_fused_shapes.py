"""The default fused samplers -- sampler_kernel (csrc/glabc_sampler.h), team_sampler_kernel<.., FAST = false> and
global_team_kernel (csrc/glabc_team.h), wide_kernel (csrc/glabc_wide.h) -- on buffers the test owns, at every instantiation the
library ships: glabc_glmcmc_steps / glabc_globalmcmc_steps through the C ABI with glabc_chains / glabc_run structs of the test's
own (engine.ChainBatch cannot pad).

Every device array sits in an allocation of its own between guard elements; the chain stride is n_chains + pad, the history
stride n_chains + another pad; outputs start as canaries (helpers.py), state inputs hold the start in the owned columns and
canaries in the padding, accumulators zero and canaries.  After GLABC_OK no owned output element is a canary and every padding
and guard element still is; after a refusal every buffer is what it was.  A cell runs 130 chains (two full groups of 64 and a
ragged one of 2) from a chain id above 2^32 for 22 iterations in launches of 7, 9 or 13 -- the later ones from the state and the
sums the earlier left -- mostly with a per-chain global frequency (values 0, 0.5, 0.75, 1 inside every wavefront; the scalar of
the same run is 0.3).  Every comparison is with the CPU checker's ONE call on unpadded host arrays, bit for bit: history, theta,
y, log_w, flags, n_moves and the three moment sums as float64 bit patterns.  These kernels are exact: there is no tolerance here.

The grids (fused_shapes_cases.py) are written out by hand from the LDS rule; CPU tests hold them to the table, hold the launch
plan to them cell by cell -- so that no cell silently runs a smaller team and repeats another -- and show from the checker alone
that every candidate index of every team cell wins at least ten global moves, every lane of a wide group that holds candidates
a winner, every wavefront of a GlobalMCMC team cell both branches and both outcomes."""
import ctypes as C

import numpy as np
import pytest
import torch

import fused_shapes_cases as K
from fused_shapes_cases import GK, N_CHAINS, cell_id, checker_case, coverage
from glabcmcmc_amd import _capi as A
from helpers import bits, bits64, canary_f32, canary_f64, canary_i32, canary_left, dev, host
from test_launch_plan import DEFAULT_SCHEDULE, ERR_ARG, ERR_DIM, GLOBAL, NO_TEAM, TEAM, L, gteam, plan, team  # noqa: F401  (plan: fixture)

ERR_KIND = -3
GUARD = 64                                  # canary elements in front of and behind every allocation
ENTRY = {"glmcmc": "glabc_glmcmc_steps", "globalmcmc": "glabc_globalmcmc_steps"}
CANARY = {np.dtype(np.float32): canary_f32, np.dtype(np.float64): canary_f64, np.dtype(np.int32): canary_i32}


def debug_flags(c):
    if c["family"] in ("team", "gteam"):
        return A.DEBUG_TEAM
    if c["family"] == "sampler":
        return A.DEBUG_NO_TEAM | (A.DEBUG_DEFAULT_SCHEDULE if c["sched"] == "def" and c["lanes"] == 1 else 0)
    return 0


# ----------------------------------------------------------------------------------------------------------------- device
class Guarded:
    """one device allocation: GUARD canaries, the body (padding columns included), GUARD canaries"""

    def __init__(self, body):
        guard = CANARY[body.dtype](GUARD)
        self.shape, self.size = body.shape, body.size
        self.before = np.concatenate([guard, body.ravel(), guard])
        self.t = dev(self.before)

    def ptr(self, offset=0):
        return self.t.data_ptr() + (GUARD + offset) * self.before.itemsize

    def fetch(self):
        """(the guards, the body)"""
        a = host(self.t)
        return np.concatenate([a[:GUARD], a[GUARD + self.size:]]), a[GUARD:GUARD + self.size].reshape(self.shape)


class FusedRun:
    """Every buffer of one glabc_init_weights + glabc_glmcmc_steps (or one glabc_globalmcmc_steps) run"""

    def __init__(self, algo, theta0, y0, T, chain0, pad, hist_pad, freq=None, moments=True, history=True, n_moves=True):
        n, d = theta0.shape
        yd = y0.shape[1]
        self.algo, self.n, self.d, self.T, self.chain0 = algo, n, d, T, chain0
        S, HS = n + pad, n + hist_pad
        self.S, self.HS = S, HS
        tri = d * (d + 1) // 2
        h = dict(theta=canary_f32(d, S), y=canary_f32(yd, S), log_w=canary_f32(S), flags=canary_i32(S))
        h["theta"][:, :n], h["y"][:, :n] = theta0.T, y0.T
        # GlobalMCMC reads and writes neither log_w nor flags: they stay canaries throughout
        self.untouched = set() if algo == "glmcmc" else {"log_w", "flags"}
        if algo == "glmcmc":
            h["flags"][:n] = 0                              # glabc_init_weights ORs GLABC_FLAG_LOCAL into what is there
        if n_moves:
            h["n_moves"] = canary_i32(S)
            h["n_moves"][:n] = 0
        if history:
            h["history"] = canary_f32(T, d, HS)
        if moments:
            for k, rows in (("sum_theta", d), ("sum_outer", tri), ("sum_jump", tri)):
                h[k] = canary_f64(rows, S)
                h[k][:, :n] = 0.0
        self.g = {k: Guarded(v) for k, v in h.items()}
        self.freq = Guarded(np.ascontiguousarray(freq, np.float32)) if freq is not None else None

    def chains(self):
        g = self.g
        return A.Chains(self.n, self.chain0, self.S, g["theta"].ptr(), g["y"].ptr(), g["log_w"].ptr(), g["flags"].ptr(),
                        g["n_moves"].ptr() if "n_moves" in g else None)

    def init(self, hip, model, glob):
        cs = self.chains()
        return hip.glabc_init_weights(C.byref(model), C.byref(glob), C.byref(cs), None)

    def steps(self, hip, model, local, glob, seed, gf, N, spl=None, lanes=0, flags=0, edit=None):
        """the T iterations in launches of `spl`, each from step0 = 1 + the iterations done; `edit(run)`: refusals"""
        cs = self.chains()
        ms = A.Moments(*(self.g[k].ptr() for k in K.SUM_KEYS)) if "sum_theta" in self.g else None
        done = 0
        while done < self.T:
            k = min(spl or self.T, self.T - done)
            run = A.Run()
            run.seed, run.step0, run.n_steps, run.global_frequency, run.batch_size = seed, 1 + done, k, gf, N
            run.lanes_per_chain, run.debug_flags = lanes, flags
            if "history" in self.g:
                run.history, run.hist_stride = self.g["history"].ptr(done * self.d * self.HS), self.HS
            if ms is not None:
                run.moments = C.pointer(ms)
            if self.freq is not None:
                run.global_frequency_per_chain = self.freq.ptr()
            if edit is not None:
                edit(run)
            rc = getattr(hip, ENTRY[self.algo])(C.byref(model), C.byref(local), C.byref(glob), C.byref(cs), C.byref(run), None)
            if rc != 0:
                return rc
            done += k
        return 0

    def _all(self):
        return list(self.g.items()) + ([("global_frequency_per_chain", self.freq)] if self.freq is not None else [])

    def assert_unchanged(self):
        for k, b in self._all():
            assert np.array_equal(host(b.t).view(np.uint8), b.before.view(np.uint8)), "a refused call wrote to `%s`" % k

    def result(self):
        """the owned columns after GLABC_OK: no owned output element is a canary, every padding and guard element still is, the
        frequency array (and what the algorithm does not own) is unchanged"""
        out, n = {}, self.n
        for k, b in self._all():
            guards, v = b.fetch()
            assert canary_left(guards) == guards.size, "`%s`: %d guard elements were written" % (k, guards.size - canary_left(guards))
            if k == "global_frequency_per_chain" or k in self.untouched:
                assert np.array_equal(host(b.t).view(np.uint8), b.before.view(np.uint8)), "`%s` was written" % k
                continue
            own, padding = v[..., :n], v[..., n:]
            assert canary_left(padding) == padding.size, "`%s`: %d padding elements were written" % (k, padding.size - canary_left(padding))
            assert canary_left(own) == 0, "`%s`: %d of %d owned elements still hold the canary" % (k, canary_left(own), own.size)
            out[k] = np.ascontiguousarray(own)
        return out


def device_case(hip, monkeypatch, c, **over):
    """the cell on the device -> the owned arrays.  over: spl, pad, hist_pad, moments, history, n_moves, constant (a constant
    frequency array), scalar_only (no array, the scalar SCALAR_ALONE)"""
    if c["nw"]:
        monkeypatch.setenv("GLABC_TEAM_WAVES", str(c["nw"]))
    else:
        monkeypatch.delenv("GLABC_TEAM_WAVES", raising=False)
    model, local, glob = K.cell_descriptors(c)
    theta0, y0 = K.cell_start(c)
    gf, arr = (K.SCALAR_ALONE, None) if over.pop("scalar_only", False) else K.frequencies(c, over.pop("constant", None))
    r = FusedRun(c["algo"], theta0, y0, c["T"], c["chain0"], over.pop("pad", c["pad"]), over.pop("hist_pad", c["hist_pad"]), freq=arr,
                 **{k: over.pop(k) for k in ("moments", "history", "n_moves") if k in over})
    if c["algo"] == "glmcmc":
        assert r.init(hip, model, glob) == 0
    rc = r.steps(hip, model, local, glob, c["seed"], gf, c["N"], spl=over.pop("spl", c["spl"]), lanes=c["lanes"], flags=debug_flags(c))
    assert rc == 0 and not over, (rc, over)
    torch.cuda.synchronize()
    return r.result()


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.float32:
        return bits(a) == bits(b)
    if a.dtype == np.float64:
        return bits64(a) == bits64(b)
    return a.astype(np.uint32) == b.astype(np.uint32)


def assert_equal_runs(got, want, what, keys=None):
    for k in (keys if keys is not None else got):
        same = same_bits(got[k], want[k])
        assert same.all(), "%s: `%s` differs in %d of %d elements, first at index %s" % (
            what, k, (~same).sum(), same.size, tuple(np.argwhere(~same)[0]))


def run_cells(hip, monkeypatch, cells, label):
    """every cell against the checker; prints the counts profiles/fused_grid.txt records"""
    wins, local = [], 0
    for c in cells:
        want, cov = checker_case(c), coverage(c)
        got = device_case(hip, monkeypatch, c)
        assert set(got) == set(want), (cell_id(c), sorted(got), sorted(want))
        assert_equal_runs(got, want, cell_id(c))
        wins.append(int(cov["wins"].min()))
        local += cov["local"]
    print("fused grid %s: %d cells, wins per candidate (minimum) %d, %d accepted local moves" % (label, len(cells), min(wins), local))


# ================================================================================================================= GPU
@pytest.mark.gpu
@pytest.mark.parametrize("shape,variant,nw", K.TEAM_PARAMS, ids=lambda v: str(v))
def test_every_exact_team_kernel(hip, monkeypatch, shape, variant, nw):
    """team_sampler_kernel<D, YD, N, VAR, NW, false> at every N of the column"""
    run_cells(hip, monkeypatch, K.team_cells(shape, variant, nw), "team %s %s NW=%d" % (shape, variant, nw))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,nw", K.GLOBAL_TEAM_PARAMS, ids=lambda v: str(v))
def test_every_global_team_kernel(hip, monkeypatch, shape, nw):
    """global_team_kernel<D, YD, VAR, NW>: both variants, equal and mixed proposal kinds (NW = 3 then draws the branch in a helper)"""
    run_cells(hip, monkeypatch, K.global_team_cells(shape, nw), "global team %s NW=%d" % (shape, nw))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", K.SAMPLER_SHAPES, ids=lambda v: str(v))
def test_every_sampler_kernel_shape(hip, monkeypatch, shape):
    """sampler_kernel at every batch size of the shape: lanes per chain 1 / 2 / 4, both schedules, unit and generic mixed over N"""
    run_cells(hip, monkeypatch, K.sampler_cells(shape), "sampler %s" % (shape,))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", K.SAMPLER_SHAPES, ids=lambda v: str(v))
def test_sampler_gamma_and_globalmcmc_kernels(hip, monkeypatch, shape):
    """the VAR_GAMMA one-lane kernels and GlobalMCMC (both schedules where both exist; with a Gamma up to theta_dim 4 and g-and-k)"""
    run_cells(hip, monkeypatch, K.sampler_extra_cells(shape), "sampler extras %s" % (shape,))


@pytest.mark.gpu
@pytest.mark.parametrize("shape,lanes,gamma", K.WIDE_PARAMS, ids=lambda v: str(v))
def test_every_wide_kernel(hip, monkeypatch, shape, lanes, gamma):
    """wide_kernel<D, YD, L, GM>: batch sizes on both sides of one candidate per lane"""
    run_cells(hip, monkeypatch, K.wide_cells(shape, lanes, gamma), "wide %s L=%d%s" % (shape, lanes, " gamma" if gamma else ""))


@pytest.mark.gpu
@pytest.mark.parametrize("family,shape", K.OPTION_PARAMS, ids=lambda v: str(v))
def test_launch_cuts_optional_buffers_and_frequency_forms(hip, monkeypatch, family, shape):
    """One cell per kernel family and shape: one launch of the total gives the bits of the cut run; n_moves = NULL is accepted
    and changes nothing else; history = NULL with moments, and moments NULL with history, leave what remains unchanged; a constant
    frequency array equals the scalar run."""
    c = K.option_cell(family, shape)
    want = checker_case(c)
    base = device_case(hip, monkeypatch, c)
    assert_equal_runs(base, want, cell_id(c))
    for over, gone in ((dict(spl=c["T"]), set()), (dict(n_moves=False), {"n_moves"}), (dict(history=False), {"history"}),
                       (dict(moments=False), set(K.SUM_KEYS)), (dict(moments=False, n_moves=False, spl=c["T"], pad=0, hist_pad=0), set(K.SUM_KEYS) | {"n_moves"})):
        got = device_case(hip, monkeypatch, c, **dict(over))
        assert set(got) == set(base) - gone, (over, sorted(got))
        assert_equal_runs(got, base, "%s %s" % (cell_id(c), over))
    scalar = checker_case(c, scalar_only=True)
    assert not same_bits(scalar["history"], want["history"]).all() or c["freq"] is None
    got = device_case(hip, monkeypatch, c, constant=K.SCALAR_ALONE)
    assert_equal_runs(got, scalar, "%s constant array" % cell_id(c))
    got = device_case(hip, monkeypatch, c, scalar_only=True)
    assert_equal_runs(got, scalar, "%s scalar" % cell_id(c))


@pytest.mark.gpu
def test_refusals_leave_every_guarded_buffer_as_it_was(hip, monkeypatch):
    """a Gamma proposal at theta_dim 5 -> GLABC_ERR_KIND, batch size 17 at theta_dim 5 -> GLABC_ERR_DIM, a lanes_per_chain the
    entry point rejects (3 for the register kernels, 12 for the lane groups) -> GLABC_ERR_ARG: status, and no buffer changes"""
    monkeypatch.delenv("GLABC_TEAM_WAVES", raising=False)

    def attempt(c, N=None, edit=None, glob=None):
        model, local, g = K.cell_descriptors(c)
        theta0, y0 = K.cell_start(c)
        gf, arr = K.frequencies(dict(c, freq=3))
        r = FusedRun(c["algo"], theta0, y0, c["T"], c["chain0"], 3, 5, freq=arr)
        rc = r.steps(hip, model, local, glob if glob is not None else g, c["seed"], gf, N or c["N"], spl=9, edit=edit)
        torch.cuda.synchronize()
        if rc != 0:
            r.assert_unchanged()
        return rc

    def lanes(value):
        return lambda run: setattr(run, "lanes_per_chain", value)

    for algo in ("glmcmc", "globalmcmc"):
        five = K.make_cell("sampler", 5, 5, "unit", algo=algo, lanes=1)
        gamma5 = K.make_dist(("gamma", [4.0] * 5, [3.0] * 5)).descriptor()
        assert attempt(five, glob=gamma5) == ERR_KIND, algo
        assert attempt(K.make_cell("sampler", 2, 5, "unit", algo=algo, lanes=1), edit=lanes(3)) == ERR_ARG, algo
    assert attempt(K.make_cell("sampler", 5, 5, "unit", lanes=1), N=17) == ERR_DIM
    assert attempt(K.make_cell("wide", 2, 20, "unit", lanes=32), edit=lanes(12)) == ERR_ARG
    assert attempt(K.make_cell("sampler", 5, 1, "unit", algo="globalmcmc", lanes=1)) == 0      # ... and the same harness is served otherwise


# ================================================================================================================= CPU
def test_the_grid_is_the_table():
    G = K.TEAM_GRID
    assert sum(len(v) for v in G.values()) == 144
    assert sum(len(v) for (s, _), v in G.items() if s != GK) == 128
    assert sum(len(v) for (s, nw), v in G.items() if s != GK and nw <= 3) == 95
    for (s, nw), sizes in G.items():
        assert sizes == tuple(range(nw, sizes[-1] + 1)), (s, nw)
    assert {k: v[-1] for k, v in G.items()} == {
        (1, 2): 16, (1, 3): 16, (1, 4): 16, (2, 2): 16, (2, 3): 14, (2, 4): 12, (3, 2): 15, (3, 3): 11, (3, 4): 10,
        (4, 2): 11, (4, 3): 8, (4, 4): 7, (GK, 2): 9, (GK, 3): 7, (GK, 4): 6}
    from test_fast_team_shapes import GRID as FAST_GRID
    assert {k: v for k, v in G.items() if k[0] != GK and k[1] <= 3} == FAST_GRID
    assert all(N in G[(s, nw)] for s, N, nw in K.FILLS_LDS)
    for s, nw, N, _ in K.FIRST_PAST:
        assert N == G[(s, nw)][-1] + 1, (s, nw)
    assert {(s, nw) for s, nw, _, _ in K.FIRST_PAST} == {k for k, v in G.items() if v[-1] < 16}
    # what the GPU tests walk: every cell once per variant it exists in
    cells = K.all_team_cells()
    assert len(cells) == 2 * 128 + 16 + 95 + 13
    ids = [(c["shape"], c["N"], K.variant_of(c), c["nw"]) for c in cells]
    assert len(set(ids)) == len(ids)
    assert {(s, N, nw) for s, N, _, nw in ids} == {(s, N, nw) for (s, nw), v in G.items() for N in v}
    for s, N, nw in {(s, N, nw) for (s, nw), v in G.items() for N in v}:
        want = {"generic"} | ({"unit"} if s != GK else set()) | ({"gamma"} if nw <= 3 else set())
        assert {v for s2, N2, v, nw2 in ids if (s2, N2, nw2) == (s, N, nw)} == want, (s, N, nw)
    # the wide grid: all 40 instantiations, batch sizes below (where one exists), just above and no multiple of L
    assert len(K.WIDE_PARAMS) == 40 and len({p for p in K.WIDE_PARAMS}) == 40
    for lanes, sizes in K.WIDE_GRID.items():
        assert all(17 <= N <= 130 for N in sizes) and any(N % lanes for N in sizes)
        assert (lanes + 1 in sizes) or lanes == 8
        assert any(N < lanes for N in sizes) == (lanes >= 32)
    # sampler_kernel: every (shape, N) once; each lane count, schedule and variant meets each shape at several N
    for s in K.SAMPLER_SHAPES:
        cells = K.sampler_cells(s)
        assert [c["N"] for c in cells] == list(range(1, 17))
        for lanes in (1, 2, 4):
            assert len([c for c in cells if c["lanes"] == lanes]) >= 3, (s, lanes)
        if s != GK:
            assert len([c for c in cells if K.variant_of(c) == "unit"]) >= 3 and len([c for c in cells if K.variant_of(c) == "generic"]) >= 3
            assert {c["kind"] for c in cells} == {"unit"} | set(K.GENERIC_KINDS), s
        if s != GK and s <= 4:
            assert {c["sched"] for c in cells if c["lanes"] == 1} == {"ilp", "def"}, s
        extra = K.sampler_extra_cells(s)
        assert {c["sched"] for c in extra if c["algo"] == "globalmcmc" and "gamma" not in c["kind"]} == ({"ilp", "def"} if s != GK and s <= 4 else {"def"})
        assert len([c for c in extra if c["algo"] == "glmcmc"]) == (5 if K.dims(s)[0] <= 4 else 0)


def test_the_inputs_are_mixed_over_the_grid():
    cells = K.all_cells()
    assert all(c["T"] % c["spl"] and 8 % c["spl"] and c["T"] > c["spl"] and c["chain0"] > 2 ** 32 for c in cells)
    assert all(c["hist_pad"] != c["pad"] for c in cells)
    for fam in ("sampler", "team", "gteam", "wide"):
        sub = [c for c in cells if c["family"] == fam]
        assert {c["spl"] for c in sub} == set(K.LAUNCHES)
        assert any(c["pad"] == 0 for c in sub) and len([c for c in sub if c["pad"] > 0]) > 0.7 * len(sub), fam
        assert 0.6 * len(sub) < len([c for c in sub if c["freq"] is not None]) < len(sub), fam
        for s in (1, 2, 3, 4):
            assert {c["kind"] for c in sub if c["shape"] == s} >= {"unit"} | set(K.GENERIC_KINDS), (fam, s)
        assert {c["kind"] for c in sub if c["shape"] == GK} >= set(K.GK_KINDS), fam
    for nw in (2, 3, 4):
        assert {c["kind"] for c in cells if c["family"] == "team" and c["nw"] == nw} >= set(K.GENERIC_KINDS)
    for c in cells:
        assert K.reaches_unit(c) == (c["kind"] == "unit"), cell_id(c)
        gf, arr = K.frequencies(c)
        if arr is not None:                                 # every wavefront: both branches possible, chains that never take one
            assert gf == K.SCALAR_WITH_ARRAY and gf not in arr
            for w in (arr[:64], arr[64:128]):
                assert {0.0, 1.0, 0.5, 0.75} == set(w.tolist())
            assert (arr == 0.0).mean() < 0.08
    # the cells of the option test exist in their grids
    for fam, s in K.OPTION_PARAMS:
        c = K.option_cell(fam, s)
        assert c["family"] == fam and c["shape"] == s and cell_id(c) in {cell_id(x) for x in cells}


def planned(plan, c, **over):
    d, yd = K.dims(c["shape"])
    kw = dict(D=d, N=c["N"], C=N_CHAINS, debug=debug_flags(c), lanes=c["lanes"] if c["family"] in ("sampler", "wide") else 0,
              gamma=int("gamma" in c["kind"]), algo=GLOBAL if c["algo"] == "globalmcmc" else 0, waves=c["nw"] or None)
    kw.update(over)
    return plan(GK=c["shape"] == GK, **kw)


def test_the_plan_runs_what_each_cell_names(plan):
    """csrc/glabc_plan.h on the CPU, with the flags, lanes and GLABC_TEAM_WAVES device_case sets: every cell plans the kernel it is
    listed under; the first batch size past a column falls to the next smaller team or to sampler_kernel; a Gamma cell asked for
    four wavefronts runs three.  With variant_of and the (shape, N) of the cell that is the kernel's full template argument list:
    no two cells of a family share one, so none silently repeats another."""
    seen = {}
    for c in K.all_cells():
        got = planned(plan, c)
        want = {"team": team(c["nw"]), "gteam": gteam(c["nw"]), "wide": ("wide", c["lanes"]),
                "sampler": L(c["lanes"], c["sched"])}[c["family"]]
        assert got == want, (cell_id(c), got)
        # the kernel's template arguments: the batch size is one of them in the register and team kernels only, the variant is
        # Gamma-or-not in the wide kernel; proposal kinds and the batch size of a wide cell are run-time values
        if c["family"] == "wide":
            key = (c["shape"], "gamma" in c["kind"], got)
        else:
            key = (c["algo"], c["shape"], c["N"] if c["algo"] == "glmcmc" else 0, K.variant_of(c), got)
        if c["family"] == "team" or (c["family"] == "sampler" and c["algo"] == "glmcmc"):
            assert key not in seen, (cell_id(c), seen[key])
        seen[key] = cell_id(c)
    for s, nw, N, (kind, size) in K.FIRST_PAST:
        c = K.make_cell("team", s, N, "unit" if s != GK else "gk-gu", nw=nw)
        assert planned(plan, c) == (team(size) if kind == "team" else L(size, "def")), (s, nw, N)
    for s in K.SHAPES:                                      # VAR_GAMMA has no team of four
        for N in K.TEAM_GRID[(s, 4)]:
            c = K.make_cell("team", s, N, "gamma", nw=4)
            assert planned(plan, c) == team(3), (s, N)
    # every shipped instantiation of the team, global team and wide kernels is named by a cell
    kernels = {k for k in seen if k[-1][0] in ("team", "gteam", "wide")}
    assert len([k for k in kernels if k[-1][0] == "team"]) == 2 * 128 + 16 + 95 + 13
    assert len([k for k in kernels if k[-1][0] == "gteam"]) == 4 * 2 * 2 + 2
    assert len([k for k in kernels if k[-1][0] == "wide"]) == 40


@pytest.mark.parametrize("shape,variant,nw", K.TEAM_PARAMS, ids=lambda v: str(v))
def test_team_inputs_reach_every_candidate(oracle, shape, variant, nw):
    """from the checker alone: over each cell every candidate index wins at least 10 global moves -- so every wavefront's
    candidates are read back from LDS, from both buffers -- and at least 100 local moves are accepted"""
    for c in K.team_cells(shape, variant, nw):
        cov = coverage(c)
        assert cov["wins"].min() >= 10, "%s: candidate %d wins %d times" % (cell_id(c), int(cov["wins"].argmin()), int(cov["wins"].min()))
        assert cov["local"] >= 100, (cell_id(c), cov["local"])


@pytest.mark.parametrize("shape,nw", K.GLOBAL_TEAM_PARAMS, ids=lambda v: str(v))
def test_global_team_inputs_reach_both_branches_and_outcomes(oracle, shape, nw):
    for c in K.global_team_cells(shape, nw):
        cov = coverage(c)
        for lo in (0, 64, 128):
            b, m = cov["branch"][:, lo:lo + 64], cov["moved"][:, lo:lo + 64]
            assert b.any() and (~b).any() and m.any() and (~m).any(), (cell_id(c), lo)
        for b in (True, False):                             # ... and over the cell each branch with each outcome
            assert (cov["moved"] & (cov["branch"] == b)).sum() >= 20 and (~cov["moved"] & (cov["branch"] == b)).sum() >= 20, cell_id(c)


@pytest.mark.parametrize("shape", K.SAMPLER_SHAPES, ids=lambda v: str(v))
def test_sampler_inputs_are_live(oracle, shape):
    """every sampler_kernel cell moves on both branches; the iSIR cells win with more than one candidate index"""
    for c in K.sampler_cells(shape) + K.sampler_extra_cells(shape):
        cov = coverage(c)
        assert cov["local"] >= 20 and cov["wins"].sum() >= 20, (cell_id(c), cov["local"], cov["wins"])
        if c["algo"] == "glmcmc":
            assert (cov["wins"] > 0).sum() >= min(c["N"], 4), (cell_id(c), cov["wins"])


@pytest.mark.parametrize("shape,lanes,gamma", K.WIDE_PARAMS, ids=lambda v: str(v))
def test_wide_inputs_reach_every_lane_that_holds_candidates(oracle, shape, lanes, gamma):
    """glabc_wide.h deals candidate j to lane j mod L of the chain's group: every lane that holds one holds a winner at least
    once; at N < L the lanes from N on hold none"""
    for c in K.wide_cells(shape, lanes, gamma):
        cov = coverage(c)
        per_lane = np.bincount(np.arange(c["N"]) % lanes, weights=cov["wins"], minlength=lanes)
        holders = min(lanes, c["N"])
        assert (per_lane[:holders] > 0).all(), (cell_id(c), per_lane)
        assert (per_lane[holders:] == 0).all() and (holders < lanes) == (c["N"] < lanes)
        assert cov["local"] >= 100, (cell_id(c), cov["local"])
