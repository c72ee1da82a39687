"""The GLABC_MATH_FAST team kernels -- team_sampler_kernel<D, D, N, VAR, NW, FAST = true> (csrc/glabc_team.h, instantiated by
csrc/glabc_team_dim.hip) -- at EVERY compiled (theta_dim, batch size, team size), in the unit-Gaussian and the generic variant:
about 190 kernels, each with N, the main / helper split and the LDS layout as compile-time constants.  Per cell, on 130 chains
(two full groups of 64 and a ragged one of 2) x 16 iterations run as two launches of 8:

  1. the tape of recorded draws is written completely (it starts as NaN) and nowhere else (canaries around it);
  2. the recorded draws are the draws (seed, chain id, iteration, j) must give: uniforms bit for bit, normals within a measured
     bound of the checker's exact Box-Muller on the same Philox words;
  3. teacher-forced parity across the launch boundary (the checker replays both tapes, the second from its own state);
  4. what the kernel leaves behind: theta, y, flags, n_moves, the streamed sums, log_w;
  5. one launch of 16 gives the bits of two launches of 8;
  6. every candidate index wins often enough that every wavefront's candidates are read back from LDS.

The grid is written out by hand from the LDS budget, never computed by the rule under test; a CPU test holds the
launch plan to it, so that no cell silently runs a smaller team and repeats another cell."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle_lib
from helpers import bits, descriptors
from test_hip_parity import _fast_run, assert_same_fast_state, fast_flips, fast_replay
from test_launch_plan import ERR_ARG, plan, team          # noqa: F401  (plan: the module-scoped driver fixture)

# (theta_dim, team size) -> the batch sizes whose helpers' candidates fit 40 960 bytes of LDS
GRID = {
    (1, 2): (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16),
    (1, 3): (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16),
    (2, 2): (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16),
    (2, 3): (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14),
    (3, 2): (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15),
    (3, 3): (3, 4, 5, 6, 7, 8, 9, 10, 11),
    (4, 2): (2, 3, 4, 5, 6, 7, 8, 9, 10, 11),
    (4, 3): (3, 4, 5, 6, 7, 8),
}
FILLS_LDS = [(2, 14, 3), (3, 11, 3), (3, 14, 2), (3, 15, 2)]            # (d, N, NW) that take the 40 KiB exactly
FIRST_PAST_THREE = [(2, 15), (3, 12), (4, 9)]                            # first N past each NW = 3 column (theta_dim 1: none, 16 fits)
REFUSED = [(3, 16), (4, 12), (4, 13), (4, 14), (4, 15), (4, 16)]         # no team of any size fits

N_CHAINS, CHAIN0, T_LAUNCH, SEED, GF = 130, 2 ** 32 + 12345, 8, (0x1234 << 32) | 20261021, 0.75
EPS = {1: 0.5, 2: 0.8, 3: 0.9, 4: 1.0}
SHIFT, SCALE = [0.1, -0.1, 0.05, -0.05], [1.0, 1.25, 0.9, 1.1]         # the generic variant's global proposal (TEAM_CASES' at d = 2)

# Largest |fast - exact| of a recorded normal and largest |d log_w| / max(1, |log_w|) against the replay, measured over the whole
# grid on an MI355X (profiles/fast_team_grid.txt: 7.15e-7, which is 6 * 2^-23, in every test; 9.54e-7 at theta_dim 4), times 4 for
# seeds and shapes outside the grid.  A wrong Philox word or block gives a difference of order one; the ceilings the bounds must
# stay under are 1e-4 and 1e-3.
Z_TOL = 4 * 7.15e-7
LOGW_TOL = 4 * 9.54e-7
assert Z_TOL < 1e-4 and LOGW_TOL < 1e-3


def specs(d, variant):
    """(local, global) of a variant: 'unit' = prior = global = N(0, I) (VAR_GAUSS_UNIT), 'generic' = a shifted, scaled Gaussian
    global (VAR_GENERIC); 'uu' / 'gu' / 'ug' = Uniform local and/or global proposals (a run-time branch of VAR_GENERIC)"""
    lg, lu = ("gauss", [0.0] * d, [0.35] * d), ("uniform", [-0.6] * d, [0.6] * d)
    gu = ("uniform", [-3.0] * d, [3.0] * d)
    return {"unit": (lg, ("gauss", [0.0] * d, [1.0] * d)), "generic": (lg, ("gauss", SHIFT[:d], SCALE[:d])),
            "uu": (lu, gu), "gu": (lg, gu), "ug": (lu, ("gauss", SHIFT[:d], SCALE[:d]))}[variant]


@functools.lru_cache(maxsize=None)
def start(d):
    rng = np.random.default_rng(100 + d)
    theta0 = (1.5 * rng.standard_normal((N_CHAINS, d))).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((N_CHAINS, d))).astype(np.float32)
    theta0.setflags(write=False)
    y0.setflags(write=False)
    return theta0, y0


@functools.lru_cache(maxsize=None)
def exact_draws(d, N):
    """what (seed, chain id, iteration, j) must give, from the checker: u [C][T][2], r [C][T], the exact normals z [C][T][N][2d],
    and the proposal words as [0, 1) uniforms zu [C][T][N][d] (oracle_philox4x32_10 + oracle_uniforms_v).  Shared by every
    variant and team size of a (theta_dim, batch size); never written to."""
    L, T = oracle_lib.load(), 2 * T_LAUNCH
    u, r = np.empty((N_CHAINS, T, 2), np.float32), np.empty((N_CHAINS, T), np.float64)
    z, zu = np.empty((N_CHAINS, T, N, 2 * d), np.float32), np.empty((N_CHAINS, T, N, d), np.float32)
    spp = (d + (d & 1) + d + 3) // 4                # Philox blocks per candidate; the d proposal words are words 0 .. d-1 of the first
    key = np.array([SEED & 0xFFFFFFFF, SEED >> 32], np.uint32)
    ctr, out = np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    f, fpos, f64 = np.zeros(4, np.float32), np.zeros(4, np.float32), np.zeros(4, np.float64)
    for c in range(N_CHAINS):
        chain = CHAIN0 + c
        ctr[0], ctr[1] = chain & 0xFFFFFFFF, chain >> 32
        for t in range(T):
            L.oracle_step_draws(SEED, chain, 1 + t, N, d, d, u[c, t].ctypes.data, r[c, t:t + 1].ctypes.data, z[c, t].ctypes.data)
            ctr[2] = 1 + t
            for j in range(N):
                ctr[3] = 1 + j * spp
                L.oracle_philox4x32_10(ctr.ctypes.data, key.ctypes.data, out.ctypes.data)
                L.oracle_uniforms_v(out.ctypes.data, out.ctypes.data, 4, f.ctypes.data, fpos.ctypes.data, f64.ctypes.data)
                zu[c, t, j] = f[:d]
    for a in (u, r, z, zu):
        a.setflags(write=False)
    return u, r, z, zu


def run_cell(oracle, d, N, variant):
    """one cell of the grid under the team size the environment selects -> (flipped chains, largest |dz|, largest relative
    |d log_w|); every assertion of the module's docstring but the cap on flipped chains, which is the caller's over its cells"""
    lspec, gspec = specs(d, variant)
    model, local, glob = descriptors(dict(epsilon=EPS[d], y_obs=[1.5 - 0.25 * j for j in range(d)], local=lspec, **{"global": gspec}))
    theta0, y0 = start(d)
    n, T, what = N_CHAINS, 2 * T_LAUNCH, "d=%d N=%d %s" % (d, N, variant)

    # ---- two launches of 8, the second from the state and the sums the first left
    h1, chains, mom, tape1 = _fast_run(model, local, glob, theta0, y0, T_LAUNCH, SEED, GF, N, chain0=CHAIN0, moments=True)
    h2, chains, mom, tape2 = _fast_run(model, local, glob, theta0, y0, T_LAUNCH, SEED, GF, N, moments=mom, step0=1 + T_LAUNCH,
                                       chains=chains)
    hist = np.concatenate([h1, h2], axis=0)
    tu, tr, tz = (np.concatenate([a, b], axis=1) for a, b in zip(tape1, tape2))

    # 1. the tape is written completely (_fast_run has checked the canaries around it)
    for name, a in (("u", tu), ("r", tr), ("z", tz)):
        assert np.isfinite(a).all(), "%s: %d entries of dump_%s were never written" % (what, int((~np.isfinite(a)).sum()), name)
    assert (tu >= 0).all() and (tu < 1).all() and (tr >= 0).all() and (tr < 1).all(), what

    # 2. the recorded draws are the draws of (seed, chain id, iteration, j)
    eu, er, ez, ezu = exact_draws(d, N)
    assert np.array_equal(bits(tu), bits(eu)), what
    assert np.array_equal(tr.view(np.uint64), er.view(np.uint64)), what
    # candidate 0 of a local iteration is the local move's proposal; every other candidate draws from the global proposal
    is_global = tu[:, :, 0] < np.float32(GF)
    uni = np.full((n, T, N), gspec[0] == "uniform")
    uni[:, :, 0] = np.where(is_global, gspec[0] == "uniform", lspec[0] == "uniform")
    prop, want_u = tz[..., :d], ezu
    assert np.array_equal(bits(prop[uni]), bits(want_u[uni])), "%s: a Uniform proposal's recorded draw is not its Philox word" % what
    assert ((prop[uni] >= 0) & (prop[uni] < 1)).all(), what
    dz = np.abs(tz.astype(np.float64) - ez)
    dz[..., :d][uni] = 0.0
    dz_max = float(dz.max())
    where = np.unravel_index(int(dz.argmax()), dz.shape)
    print("%s: largest |fast - exact| normal %.3g at (chain, iteration, j, word) = %s" % (what, dz_max, where))
    assert dz_max <= Z_TOL, "%s: recorded normal at (chain, iteration, j, word) = %s is %.3g from the exact one" % (what, where, dz_max)

    # 3. teacher-forced parity across the launch boundary
    tapes = [tape1, tape2]
    hh, hc, hm = fast_replay(oracle, model, local, glob, theta0, y0, GF, N, tapes, chain0=CHAIN0, seed=SEED, moments=True)
    flipped, unexplained = fast_flips(oracle, model, local, glob, theta0, y0, GF, N, tapes, hist, hh, chain0=CHAIN0, seed=SEED)
    assert not unexplained, "%s: decisions that differ beyond rounding of their threshold: %s" % (what, unexplained[:5])
    keep = np.setdiff1d(np.arange(n), flipped)

    # 4. what the kernel leaves behind, for the chains that followed the checker
    assert_same_fast_state(chains, hc, keep)
    for name in ("sum_theta", "sum_outer", "sum_jump"):
        got, want = getattr(mom, name).cpu().numpy()[:, keep], getattr(hm, name)[:, keep]
        assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(want).view(np.uint64)), "%s: %s" % (what, name)
    lw, lw_ref = chains.log_w.cpu().numpy()[keep].astype(np.float64), hc.log_w[keep].astype(np.float64)
    fin = np.isfinite(lw_ref)
    assert np.array_equal(np.isfinite(lw), fin) and np.array_equal(lw[~fin], lw_ref[~fin], equal_nan=True), what
    rel = np.abs(lw[fin] - lw_ref[fin]) / np.maximum(1.0, np.abs(lw_ref[fin]))
    rel_max = float(rel.max()) if rel.size else 0.0
    print("%s: largest |d log_w| / max(1, |log_w|) %.3g; %d chains flipped" % (what, rel_max, len(flipped)))
    assert rel_max <= LOGW_TOL, "%s: log_w is %.3g (relative) from the replay's" % (what, rel_max)

    # 5. launch cuts are invisible: one launch of 16, without the tape
    hist16, chains16, _, _ = _fast_run(model, local, glob, theta0, y0, T, SEED, GF, N, chain0=CHAIN0, dump=False)
    same = bits(hist16) == bits(hist)
    assert same.all(), "%s: one launch differs from two at (iteration, dim, chain) = %s" % (what, np.argwhere(~same)[0])
    for name in ("theta", "y", "log_w"):
        assert np.array_equal(bits(getattr(chains16, name).cpu().numpy()), bits(getattr(chains, name).cpu().numpy())), (what, name)
    for name in ("flags", "n_moves"):
        assert np.array_equal(getattr(chains16, name).cpu().numpy(), getattr(chains, name).cpu().numpy()), (what, name)

    # 6. coverage, on the replay and the tape alone: who won each global move
    rows = np.concatenate([theta0.T[None], hh], axis=0)                              # (T + 1, d, n)
    moved = (rows[1:] != rows[:-1]).any(axis=1).T                                    # (n, T)
    p0 = np.array([glob.p0[i] for i in range(d)], np.float32)
    p2 = np.array([glob.p2[i] for i in range(d)], np.float32)
    cand = p0 + p2 * prop                                                            # float32, as the kernel: (n, T, N, d)
    hit = (cand == hh.transpose(2, 0, 1)[:, :, None, :]).all(axis=3)                # (n, T, N)
    won = moved & is_global
    assert hit[won].any(axis=1).all(), "%s: a global move's new state is none of its candidates" % what
    wins = np.bincount(hit[won].argmax(axis=1), minlength=N)
    local_moves = int((moved & ~is_global).sum())
    print("%s: wins per candidate %s, %d accepted local moves, %d moves" % (what, wins.tolist(), local_moves, int(hc.n_moves.sum())))
    assert wins.min() >= 10, "%s: candidate %d wins %d times" % (what, int(wins.argmin()), int(wins.min()))
    assert local_moves >= 100 and int(hc.n_moves.sum()) > n, what
    return len(flipped), dz_max, rel_max


def run_cells(oracle, monkeypatch, cells, nw, label):
    """cells = [(d, N, variant)] under a team of nw wavefronts: nw = 3 is what a launch this small gets, GLABC_TEAM_WAVES = 2
    forces the other instantiation (tests/test_launch_plan.py and test_the_plan_runs_the_team_each_cell_names)"""
    if nw == 2:
        monkeypatch.setenv("GLABC_TEAM_WAVES", "2")
    else:
        monkeypatch.delenv("GLABC_TEAM_WAVES", raising=False)
    got = [run_cell(oracle, d, N, variant) for d, N, variant in cells]
    flipped, total = sum(g[0] for g in got), N_CHAINS * len(cells)
    print("fast team grid %s: %d cells, %d of %d chains flipped (all explained), largest |dz| %.4g, largest relative |d log_w| %.4g"
          % (label, len(cells), flipped, total, max(g[1] for g in got), max(g[2] for g in got)))
    assert flipped <= max(4, total // 200), "%d of %d chains leave the checker's path" % (flipped, total)


@pytest.mark.gpu
@pytest.mark.parametrize("nw", [2, 3])
@pytest.mark.parametrize("variant", ["unit", "generic"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_every_fast_team_kernel(hip, oracle, monkeypatch, d, variant, nw):
    run_cells(oracle, monkeypatch, [(d, N, variant) for N in GRID[(d, nw)]], nw, "d=%d %s NW=%d" % (d, variant, nw))


# the proposal kind is a run-time branch of the generic instantiations: one cell per theta_dim, three of them LDS-filling or largest
UNIFORM_CELLS = [(1, 16, 3, "uu"), (2, 14, 3, "gu"), (3, 15, 2, "ug"), (4, 8, 3, "uu")]


@pytest.mark.gpu
@pytest.mark.parametrize("d,N,nw,variant", UNIFORM_CELLS, ids=lambda v: str(v))
def test_uniform_proposals_in_the_fast_team_kernels(hip, oracle, monkeypatch, d, N, nw, variant):
    assert N in GRID[(d, nw)]
    run_cells(oracle, monkeypatch, [(d, N, variant)], nw, "d=%d N=%d %s NW=%d" % (d, N, variant, nw))


@pytest.mark.gpu
@pytest.mark.parametrize("waves", [None, 2])
def test_sizes_no_team_fits_are_refused(hip, monkeypatch, waves):
    """GLABC_MATH_FAST exists as team kernels only: (theta_dim, N) whose candidates fit no team's LDS return GLABC_ERR_ARG from
    glabc_glmcmc_steps and leave the chains as they were"""
    from glabcmcmc_amd import _capi as A
    from glabcmcmc_amd import engine
    if waves:
        monkeypatch.setenv("GLABC_TEAM_WAVES", str(waves))
    dev = torch.device("cuda", 0)
    for d, N in REFUSED:
        lspec, gspec = specs(d, "unit")
        model, local, glob = descriptors(dict(epsilon=EPS[d], y_obs=[1.5 - 0.25 * j for j in range(d)], local=lspec, **{"global": gspec}))
        theta0, y0 = start(d)
        chains = engine.ChainBatch(torch.from_numpy(theta0), torch.from_numpy(y0), dev, chain0=CHAIN0)
        engine.init_weights(model, glob, chains)
        torch.cuda.synchronize()
        names = ("theta", "y", "log_w", "flags", "n_moves")
        before = [getattr(chains, k).cpu().numpy().copy() for k in names]
        cs, run = chains.struct(), A.Run()
        run.seed, run.step0, run.n_steps, run.global_frequency, run.batch_size, run.math_mode = SEED, 1, T_LAUNCH, GF, N, A.MATH_FAST
        assert hip.glabc_glmcmc_steps(C.byref(model), C.byref(local), C.byref(glob), C.byref(cs), C.byref(run), None) == ERR_ARG, (d, N)
        torch.cuda.synchronize()
        for k, a, b in zip(names, before, [getattr(chains, k).cpu().numpy() for k in names]):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (d, N, k)
        run.batch_size = GRID[(d, 2)][-1]                                  # the largest size that fits is served
        assert hip.glabc_glmcmc_steps(C.byref(model), C.byref(local), C.byref(glob), C.byref(cs), C.byref(run), None) == 0, (d, N)
        torch.cuda.synchronize()
        assert int(chains.n_moves.sum()) > 0


# ---------------------------------------------------------------------------------- CPU: the grid is the plan's
def test_the_grid_is_the_table():
    assert sum(len(v) for v in GRID.values()) == 95
    for (d, nw), sizes in GRID.items():
        assert sizes == tuple(range(nw, sizes[-1] + 1)), (d, nw)
    assert {k: v[-1] for k, v in GRID.items()} == {(1, 2): 16, (1, 3): 16, (2, 2): 16, (2, 3): 14, (3, 2): 15, (3, 3): 11,
                                                   (4, 2): 11, (4, 3): 8}
    assert all(N in GRID[(d, nw)] for d, N, nw in FILLS_LDS)
    assert all(N in GRID[(d, nw)] for d, N, nw, _ in UNIFORM_CELLS)


def test_the_plan_runs_the_team_each_cell_names(plan):
    """csrc/glabc_plan.h on the CPU: with fast = 1 at this module's chain count every cell plans the team size it is listed under
    (NW = 2 through GLABC_TEAM_WAVES = 2, as run_cells sets it), the first batch size past each NW = 3 column falls to a team of
    two, and the sizes no team fits are refused -- a cell that silently ran a smaller team would repeat another cell"""
    for (d, nw), sizes in GRID.items():
        for N in sizes:
            assert plan(fast=1, D=d, N=N, C=N_CHAINS, waves=(2 if nw == 2 else None)) == team(nw), (d, N, nw)
    for d, N in FIRST_PAST_THREE:
        assert N - 1 == GRID[(d, 3)][-1]
        assert plan(fast=1, D=d, N=N, C=N_CHAINS) == team(2), (d, N)
    for d, N in REFUSED:
        assert plan(fast=1, D=d, N=N, C=N_CHAINS) == ("refused", ERR_ARG), (d, N)
        assert plan(fast=1, D=d, N=N, C=N_CHAINS, waves=2) == ("refused", ERR_ARG), (d, N)
