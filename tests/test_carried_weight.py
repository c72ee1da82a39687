"""The weight a GLMCMC chain carries between iterations (Chain::w_cur, csrc/glabc_device.h) is, after a move, the winner's
fast-pass weight (isir_weight_approx); the IEEE fallback of the index search recomputes the specified one from lw_cur.
Every case runs twice, by default and with GLABC_DEBUG_EXACT_INDEX, and both runs must equal the CPU checker bit for bit:
the forced-fallback run takes every index from the recomputed w[0] (a stale or mismatched lw_cur shows at once, a wrong
last bit only where u lies that close to a partial sum or, in the denormal regimes, where the stand-in's absolute error is
large), the default run shows that the fast pass with an approximate w[0] picks the same indices.
  - 192 chains (a ragged last wavefront), 120 iterations in launches of 13, chain ids above 2^32; teams of 2, 3 and 4
    wavefronts and 1, 2 and 4 lanes per chain; N in {2, 5, 16}, theta_dim in {1, 2, 4} -- every (N, theta_dim, geometry)
    that the launch plan honours: a team the batch cannot be split into or whose candidates exceed the LDS budget, and a
    lane group wider than the batch allows, would silently run a smaller one (csrc/glabc_plan.h), i.e. repeat another case;
  - the ends of the float range (the regimes of tests/test_isir_weight.py), where the fast pass must hand over, and the
    same with global_frequency 0.5, so that the local-flag hand-over of lw_cur precedes many global steps;
  - coverage, asserted on the checker's output alone: in every case of the first group some chain moves on at least half
    of the iterations, and in its all-global cases (global_frequency 1: a chain that keeps its state took index 0) some
    chain stays after having moved within the same launch, so a carried weight is consumed.  (The regimes of the second
    group are chosen for where their weights sit, not for how often they move: there the cap is one move at all.)
GPU only."""
import numpy as np
import pytest

from helpers import bits, descriptors
from test_hip_parity import hip_run, oracle_run, assert_same_state

pytestmark = pytest.mark.gpu

N_CHAINS, T, LAUNCH = 192, 120, 13
CHAIN0 = (1 << 32) + 12345
GEOMETRIES = ["team2", "team3", "team4", "lanes1", "lanes2", "lanes4"]


# the integer rules of csrc/glabc_geometry.h that decide whether a forced geometry is the one that runs (tests/test_launch_plan.py
# pins plan_launch itself): team_main_candidates, team_config_ok with TEAM_MAX_LDS, pick_lanes with explicit lanes
def team_main_candidates(n, nw):
    na = ((10 * n + 11) // nw - 11 + 5) // 10
    return 1 if na < 1 else min(na, n - (nw - 1))


def geometry_is_honoured(geometry, N, d):
    k = int(geometry[-1])
    if geometry.startswith("team"):
        return N >= k and 2 * (N - team_main_candidates(N, k)) * (4 + d + d) * 64 * 4 <= 40 * 1024
    return k == 1 or (k == 2 and N >= 2) or (k == 4 and N >= 3)


CASES = [(N, d, g) for N in (2, 5, 16) for d in (1, 2, 4) for g in GEOMETRIES if geometry_is_honoured(g, N, d)]
# global_frequency per batch size: N = 2 runs all-global (the stay-after-move condition is read off its history); epsilon per
# theta_dim, wide enough that some chain moves on half of the iterations at every batch size (checked on the CPU checker)
GF = {2: 1.0, 5: 0.9, 16: 0.75}
EPS = {1: 0.5, 2: 0.8, 4: 1.0}

_checker = {}


def config(N, d, eps, c0=None):
    cfg = dict(epsilon=eps, local=("gauss", [0.0] * d, [0.35] * d), **{"global": ("gauss", [0.0] * d, [1.0] * d)})
    if d != 2:
        cfg["y_obs"] = [1.5 - 0.25 * j for j in range(d)]
    model, local, glob = descriptors(cfg)
    if c0 is not None:
        model.kern_c0 = c0
    rng = np.random.default_rng(1000 * N + 10 * d + 1)
    theta0 = (rng.standard_normal((N_CHAINS, d)) * 1.5).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((N_CHAINS, d))).astype(np.float32)
    seed = 77000 + 100 * N + d
    return model, local, glob, theta0, y0, seed


def checker(oracle, N, d, eps, gf, c0=None):
    """the CPU checker's history and final state of a configuration: computed once, shared by the geometries, never changed"""
    key = (N, d, eps, gf, c0)
    if key not in _checker:
        model, local, glob, theta0, y0, seed = config(N, d, eps, c0)
        hh, hc, _ = oracle_run(oracle, "glmcmc", model, local, glob, theta0, y0, T, seed, gf, N, chain0=CHAIN0)
        hh.setflags(write=False)
        _checker[key] = (hh, hc, theta0)
    return _checker[key]


def geometry_flags(geometry, monkeypatch):
    from glabcmcmc_amd import _capi as A
    if geometry.startswith("team"):
        monkeypatch.setenv("GLABC_TEAM_WAVES", geometry[4:])
        return 0, A.DEBUG_TEAM
    return int(geometry[5:]), A.DEBUG_NO_TEAM


def both_runs_equal_the_checker(oracle, geometry, monkeypatch, N, d, eps, gf, c0=None):
    from glabcmcmc_amd import _capi as A
    hh, hc, _ = checker(oracle, N, d, eps, gf, c0)
    lanes, flags = geometry_flags(geometry, monkeypatch)
    model, local, glob, theta0, y0, seed = config(N, d, eps, c0)
    for name, extra in (("default", 0), ("exact index", A.DEBUG_EXACT_INDEX)):
        hist, chains, _ = hip_run("glmcmc", model, local, glob, theta0, y0, T, seed, gf, N, chain0=CHAIN0, lanes=lanes,
                                  debug_flags=flags | extra, steps_per_launch=LAUNCH)
        same = bits(hist) == bits(hh)
        assert same.all(), "%s run: first mismatch at (t, dim, chain) = %s" % (name, np.argwhere(~same)[0],)
        assert_same_state(chains, hc, True)


def moved_table(hh, theta0):
    """[t, chain]: the chain's state changed at iteration t (the checker's history against the row before it)"""
    prev = np.concatenate([theta0.T[None], hh[:-1]], axis=0)
    return (bits(hh) != bits(prev)).any(axis=1)


def stays_after_a_move_within_a_launch(moved):
    """some chain keeps its state at an iteration after one at which it moved, both inside one launch of LAUNCH iterations"""
    for t0 in range(0, T, LAUNCH):
        m = moved[t0:t0 + LAUNCH]
        seen = np.cumsum(m, axis=0) > 0
        if (seen[:-1] & ~m[1:]).any():
            return True
    return False


def test_every_geometry_and_size_is_reached():
    """teams of 2, 3 and 4 wavefronts and lane groups of 1, 2 and 4 each run at two batch sizes at least and at every theta_dim"""
    for g in GEOMETRIES:
        assert len({N for N, d, gg in CASES if gg == g}) >= 2, g
        assert {d for N, d, gg in CASES if gg == g} == {1, 2, 4}, g
    assert {(N, d) for N, d, g in CASES} == {(N, d) for N in (2, 5, 16) for d in (1, 2, 4)}


@pytest.mark.parametrize("N,d,geometry", CASES, ids=lambda v: str(v))
def test_carried_weight_equals_the_checker(hip, oracle, N, d, geometry, monkeypatch):
    hh, hc, theta0 = checker(oracle, N, d, EPS[d], GF[N])
    assert int(hc.n_moves.max()) >= T // 2, "no chain moves on half of the iterations: %d" % int(hc.n_moves.max())
    both_runs_equal_the_checker(oracle, geometry, monkeypatch, N, d, EPS[d], GF[N])


def test_a_carried_weight_is_consumed(oracle):
    """the all-global cases of the first group (N = 2): keeping the state there is the stay index 0, and some chain does so
    after a move of the same launch -- its w[0] was a carried fast-pass weight.  The checker's output alone."""
    for d in (1, 2, 4):
        assert GF[2] == 1.0
        hh, hc, theta0 = checker(oracle, 2, d, EPS[d], GF[2])
        moved = moved_table(hh, theta0)
        assert np.array_equal(moved.sum(axis=0).astype(np.uint32), hc.n_moves)
        assert stays_after_a_move_within_a_launch(moved), "theta_dim %d" % d


# tests/test_isir_weight.py EDGE_CASES (kern_c0 or None for the model's own, epsilon) at global_frequency 0.8, then the
# hand-over cases: half of the steps local, so an accepted local move's lw_cur reaches log_w at a later global step and the
# fallback (second row: every total below the fast pass's floor) takes its w[0] from it
EDGE_CASES = [(c0, eps, 0.8) for c0, eps in
              [(88.6, 0.05), (87.0, 0.05), (-60.0, 0.05), (-75.0, 0.05), (-100.0, 0.05), (-103.0, 0.3),
               (None, 1e-4), (None, 0.002), (None, 3e6)]] + [(None, 0.3, 0.5), (-100.0, 0.3, 0.5), (88.6, 0.3, 0.5)]


@pytest.mark.parametrize("geometry", ["team2", "team3", "lanes1", "lanes2", "lanes4"])
@pytest.mark.parametrize("c0,eps,gf", EDGE_CASES, ids=lambda v: str(v))
def test_ends_of_the_float_range_equal_the_checker(hip, oracle, c0, eps, gf, geometry, monkeypatch):
    assert geometry_is_honoured(geometry, 5, 2)
    hh, hc, theta0 = checker(oracle, 5, 2, eps, gf, c0)
    assert int(hc.n_moves.sum()) > 0
    if gf == 0.5:           # local moves are accepted and global steps follow them: the hand-over happens
        assert int(hc.n_moves.max()) >= T // 4
    both_runs_equal_the_checker(oracle, geometry, monkeypatch, 5, 2, eps, gf, c0)
