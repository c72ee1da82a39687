"""The cells of tests/test_fused_shapes.py: which kernel each names, the inputs it runs on, the CPU checker's run of it and what
that run reaches.  Nothing here touches a GPU.

A cell is a dict: the kernel it is listed under (family, shape, batch size, variant, team size / lanes / schedule) and the
parameters mixed over the grid (padding of both strides, launch length, per-chain frequencies, proposal kinds, seed, chain id).
The grids are written out by hand from the LDS rule of DESIGN.md 4.0 (two iterations of the helpers' candidates,
2 (N - NA) (4 + theta_dim + y_dim) 256 bytes <= 40 960, NA = the main wavefront's share); the launch plan is held to them, never
asked for them."""
import ctypes as C
import functools

import numpy as np

import oracle_lib
from glabcmcmc_amd import _capi as A
from helpers import descriptors, make_dist

N_CHAINS = 130                       # two full groups of 64 and a ragged one of 2; the wide kernel's last block is ragged at every L
T_TOTAL = 22                         # iterations of a cell; no launch length below divides it or GLOBAL_TEAM_CHUNK = 8
LAUNCHES = (7, 9, 13)
GK = "gk"                            # the g-and-k shape: theta_dim 4, y_dim 8
SHAPES = (1, 2, 3, 4, GK)

# ---- team_sampler_kernel<D, YD, N, VAR, NW, false>: (shape, team size) -> the batch sizes whose helpers' candidates fit 40 KiB
TEAM_GRID = {
    (1, 2): (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16),
    (1, 3): (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16),
    (1, 4): (4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16),
    (2, 2): (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16),
    (2, 3): (3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14),
    (2, 4): (4, 5, 6, 7, 8, 9, 10, 11, 12),
    (3, 2): (2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15),
    (3, 3): (3, 4, 5, 6, 7, 8, 9, 10, 11),
    (3, 4): (4, 5, 6, 7, 8, 9, 10),
    (4, 2): (2, 3, 4, 5, 6, 7, 8, 9, 10, 11),
    (4, 3): (3, 4, 5, 6, 7, 8),
    (4, 4): (4, 5, 6, 7),
    (GK, 2): (2, 3, 4, 5, 6, 7, 8, 9),
    (GK, 3): (3, 4, 5, 6, 7),
    (GK, 4): (4, 5, 6),
}
# (shape, N, NW) that take the 40 960 bytes exactly
FILLS_LDS = [(2, 14, 3), (2, 12, 4), (3, 14, 2), (3, 15, 2), (3, 11, 3), (3, 9, 4), (3, 10, 4), (GK, 8, 2), (GK, 9, 2), (GK, 6, 3),
             (GK, 7, 3), (GK, 6, 4)]
# (shape, NW, first N past the column, what the plan then runs: the next smaller team, or lanes of sampler_kernel)
FIRST_PAST = [(2, 3, 15, ("team", 2)), (2, 4, 13, ("team", 3)), (3, 2, 16, ("lanes", 4)), (3, 3, 12, ("team", 2)), (3, 4, 11, ("team", 3)),
              (4, 2, 12, ("lanes", 4)), (4, 3, 9, ("team", 2)), (4, 4, 8, ("team", 3)), (GK, 2, 10, ("lanes", 4)), (GK, 3, 8, ("team", 2)),
              (GK, 4, 7, ("team", 3))]
GAMMA_WAVES = (2, 3)                 # VAR_GAMMA is instantiated for teams of two and three: four asked for runs three

# ---- wide_kernel<D, YD, L, GM>: lanes per chain -> batch sizes on both sides of one candidate per lane.  N < L leaves lanes
# without a candidate; it does not exist for L = 8 and L = 16 (the kernel serves N >= 17), where 17 -- L + 1 at L = 16, two full
# rounds and one candidate at L = 8 -- stands in; then N = L + 1 (one lane with a second candidate) and an N no multiple of L
WIDE_GRID = {8: (17, 27), 16: (17, 27), 32: (20, 33, 50), 64: (40, 65, 100)}

EPS = {1: 0.5, 2: 0.8, 3: 0.9, 4: 1.0, 5: 1.0, 6: 1.0, 7: 1.0, 8: 1.0, GK: 1.0}       # each has a verified reciprocal (glabc_hip.hip)
SHIFT, SCALE = [0.1, -0.1, 0.05, -0.05, 0.1, -0.1, 0.05, -0.05], [1.0, 1.25, 0.9, 1.1, 1.0, 1.25, 0.9, 1.1]
GENERIC_KINDS = ("shift", "tiny", "uu", "gu", "ug")
GK_KINDS = ("gk-gu", "gk-gg", "gk-uu", "gk-ug")
GK_GAMMA_KINDS = ("gamma-gamma", "gamma-uniform", "uniform-gamma", "gamma-boost")
# where every candidate index (team) or lane (wide) has to win: a Gamma prior with the Uniform(0, 10)^4 proposal accepts a handful
# of global moves per cell, and a narrower Uniform proposal has states outside its support under a Gamma prior; that pair runs
# in the one-lane VAR_GAMMA cells, where the proposal's kind is the same run-time branch
GK_GAMMA_WINNING = ("gamma-gamma", "uniform-gamma", "gamma-boost")
GK_PRIOR = ("gamma", [3.0, 2.0, 2.0, 1.5], [1.0, 2.0, 1.0, 3.0])
GK_PROP = ("gamma", [9.0, 4.0, 4.0, 2.0], [3.0, 4.0, 2.0, 4.0])
GK_BOOST = ("gamma", [9.0, 0.7, 4.0, 2.0], [3.0, 1.0, 2.0, 4.0])                      # a shape below 1: the boost draw
GK_UNIFORM = ("uniform", [0.0] * 4, [10.0] * 4)
# the generic g-and-k cells: a box around the start states as prior AND as Uniform global proposal -- no state leaves the
# proposal's support, and enough candidates are plausible for every candidate index to win (Uniform(0, 10)^4 gives a handful)
GK_BOX = ("uniform", [1.0, 0.2, 0.5, 0.1], [7.0, 3.0, 5.0, 1.5])
GK_GAUSS = ("gauss", [3.0, 1.0, 2.0, 0.5], [1.0, 0.5, 0.7, 0.3])

# per-chain global frequencies: chain i takes FREQ_TABLE[(i + offset) % 16] -- one chain in 16 never moves globally, three never
# locally, the others take both branches; every group of 64 lanes holds all four values
FREQ_TABLE = (0.75, 0.5, 1.0, 0.75, 0.75, 0.5, 0.0, 0.75, 1.0, 0.75, 0.5, 0.75, 0.75, 1.0, 0.5, 0.75)
SCALAR_WITH_ARRAY = 0.3              # glabc_run.global_frequency of a run that sets the array: a kernel that read it would fail
SCALAR_ALONE = 0.75
PADS = (3, 1, 62, 5, 0, 2, 9)


def dims(shape):
    return (4, 8) if shape == GK else (shape, shape)


def make_cell(family, shape, N, kind, algo="glmcmc", nw=0, lanes=0, sched="def", salt=0):
    d, yd = dims(shape)
    mix = N + 3 * d + nw + lanes + salt
    pad = PADS[mix % 7]
    return dict(family=family, algo=algo, shape=shape, N=N, kind=kind, nw=nw, lanes=lanes, sched=sched,
                pad=pad, hist_pad=(pad + 3) % 8,                     # never the chain stride's
                spl=LAUNCHES[mix % 3], T=T_TOTAL,
                freq=None if mix % 4 == 3 else (mix % 16),           # most cells: the per-chain array, at this offset
                seed=((d * 7919 + yd * 104729 + N * 31 + salt) * 2654435761 + 20261021) & (2 ** 63 - 1),
                chain0=((1 + N % 3) << 32) + 1000003 * d + N)        # above 2^32: both Philox counter words in use


def cell_id(c):
    geo = "NW%d" % c["nw"] if c["nw"] else "L%d%s" % (c["lanes"], c["sched"] if c["family"] == "sampler" else "")
    return "%s-%s-%s-N%d-%s-%s" % (c["family"], c["algo"], c["shape"], c["N"], c["kind"], geo)


def variant_of(c):
    """the template argument VAR the cell is listed under"""
    if "gamma" in c["kind"]:
        return "gamma"
    return "unit" if c["kind"] == "unit" else "generic"


# ------------------------------------------------------------------------------------------------------------ the grids
def team_cells(shape, variant, nw):
    """every N of the column, in one variant: 'unit', 'generic' (the kinds that reach it mixed over N) or 'gamma'"""
    out = []
    for N in TEAM_GRID[(shape, nw)]:
        if variant == "gamma":
            kind = GK_GAMMA_WINNING[(N + nw) % 3] if shape == GK else "gamma"
        elif shape == GK:
            kind = GK_KINDS[(N + nw) % 4]
        else:
            kind = "unit" if variant == "unit" else GENERIC_KINDS[(N + shape + nw) % 5]
        out.append(make_cell("team", shape, N, kind, nw=nw))
    return out


TEAM_PARAMS = [(s, v, nw) for s in (1, 2, 3, 4) for v in ("unit", "generic") for nw in (2, 3, 4)] + \
              [(GK, "generic", nw) for nw in (2, 3, 4)] + [(s, "gamma", nw) for s in SHAPES for nw in GAMMA_WAVES]


def global_team_cells(shape, nw):
    """global_team_kernel<D, YD, VAR, NW>: both variants (g-and-k has the generic one only), every kind that reaches the generic"""
    kinds = GK_KINDS if shape == GK else ("unit",) + GENERIC_KINDS
    cells = [make_cell("gteam", shape, 1, k, algo="globalmcmc", nw=nw, salt=i) for i, k in enumerate(kinds)]
    for i, c in enumerate(cells):
        # offsets of FREQ_TABLE at which the two chains of the ragged wavefront take both branches; one cell on the scalar
        c["freq"] = (0, 4, None, 9, 10, 14)[(i + nw) % 6]
    return cells


GLOBAL_TEAM_PARAMS = [(s, nw) for s in SHAPES for nw in (2, 3)]

SAMPLER_SHAPES = (1, 2, 3, 4, 5, 6, 7, 8, GK)


def sampler_cells(shape):
    """sampler_kernel at every batch size of a shape, once each; lanes per chain, schedule and variant mixed over N"""
    d, yd = dims(shape)
    low = shape != GK and d <= 4                            # where the max-ilp objects exist
    out = []
    for N in range(1, 17):
        lanes = (1, 2, 4)[(N + d + (yd == 8)) % 3]
        lanes = 1 if N == 1 else 2 if (N == 2 and lanes == 4) else lanes
        sched = ("ilp", "def")[(N // 3 + d) % 2] if (low and lanes == 1) else "def"
        if shape == GK:
            kind = GK_KINDS[N % 4]
        else:
            kind = ("unit", "shift", "unit", "tiny", "unit", "gu", "unit", "ug", "unit", "uu")[(N + 3 * d) % 10]
        out.append(make_cell("sampler", shape, N, kind, lanes=lanes, sched=sched))
    return out


def sampler_extra_cells(shape):
    """the VAR_GAMMA one-lane kernels (theta_dim 1 .. 4 and g-and-k) at a handful of batch sizes, and GlobalMCMC on both schedules"""
    d, yd = dims(shape)
    low = shape != GK and d <= 4
    out = []
    if d <= 4:
        for i, N in enumerate((1, 2, 5, 11, 16)):
            # (the Uniform(0, 10)^4 proposal under a Gamma prior falls on N = 11: it accepts few global moves per candidate)
            out.append(make_cell("sampler", shape, N, GK_GAMMA_KINDS[(i + 2) % 4] if shape == GK else "gamma", lanes=1, salt=5))
    for i, sched in enumerate(("ilp", "def") if low else ("def",)):
        kinds = GK_KINDS[:2] if shape == GK else ("unit", "ug")
        out.append(make_cell("sampler", shape, 1, kinds[i % 2], algo="globalmcmc", lanes=1, sched=sched, salt=7 + i))
    if d <= 4:
        out.append(make_cell("sampler", shape, 1, "gamma-gamma" if shape == GK else "gamma", algo="globalmcmc", lanes=1, salt=9))
    return out


def wide_cells(shape, L, gamma):
    out = []
    for i, N in enumerate(WIDE_GRID[L]):
        if gamma:
            kind = GK_GAMMA_WINNING[(i + L // 8) % 3] if shape == GK else "gamma"
        elif shape == GK:
            kind = GK_KINDS[(i + L // 8) % 4]
        else:
            kind = ("unit",) + GENERIC_KINDS                # the wide kernel has one variant: all six kinds run it
            kind = kind[(i + L // 8 + shape) % 6]
        out.append(make_cell("wide", shape, N, kind, lanes=L))
    return out


WIDE_PARAMS = [(s, L, g) for s in SHAPES for L in (8, 16, 32, 64) for g in (False, True)]


def all_team_cells():
    return [c for p in TEAM_PARAMS for c in team_cells(*p)]


def all_cells():
    return all_team_cells() + [c for p in GLOBAL_TEAM_PARAMS for c in global_team_cells(*p)] + \
        [c for s in SAMPLER_SHAPES for c in sampler_cells(s) + sampler_extra_cells(s)] + [c for p in WIDE_PARAMS for c in wide_cells(*p)]


# one cell per kernel family and shape for the runs that change the launches, the optional buffers or the form of the frequency
def option_cell(family, shape):
    if family == "team":
        return team_cells(shape, "generic", 3)[2]
    if family == "gteam":
        return global_team_cells(shape, 3)[-1]
    if family == "wide":
        return wide_cells(shape, 32, False)[0]
    return sampler_cells(shape)[4]


OPTION_PARAMS = [(f, s) for f in ("sampler", "team", "gteam", "wide") for s in SHAPES]


# -------------------------------------------------------------------------------------------------------- inputs of a cell
def y_obs_of(c):
    d, _ = dims(c["shape"])
    y = [1.5 - (0.25 if d <= 4 else 0.125) * j for j in range(d)]
    if c["kind"] == "tiny":
        y[(d - 1) // 2] = 0.01                              # below 2^-6: the unit configuration falls to the generic variant
    return y


def specs_of(c):
    """(prior or None for the Model's own, local, global) as make_dist specifications"""
    d, _ = dims(c["shape"])
    k = c["kind"]
    if c["shape"] == GK:
        lg, lu = ("gauss", [0.0] * 4, [0.15] * 4), ("uniform", [-0.25] * 4, [0.25] * 4)
        return {"gk-gu": (GK_BOX, lg, GK_BOX), "gk-gg": (GK_BOX, lg, GK_GAUSS), "gk-uu": (GK_BOX, lu, GK_BOX), "gk-ug": (GK_BOX, lu, GK_GAUSS),
                "gamma-gamma": (GK_PRIOR, lg, GK_PROP), "gamma-uniform": (GK_PRIOR, lg, GK_UNIFORM), "uniform-gamma": (None, lg, GK_PROP),
                "gamma-boost": (GK_PRIOR, lg, GK_BOOST)}[k]
    lg, lu = ("gauss", [0.0] * d, [0.35] * d), ("uniform", [-0.6] * d, [0.6] * d)
    unit, shifted, gu = ("gauss", [0.0] * d, [1.0] * d), ("gauss", SHIFT[:d], SCALE[:d]), ("uniform", [-3.0] * d, [3.0] * d)
    if k == "gamma":
        return ("gamma", [2.0] * d, [1.0] * d), lg, ("gamma", [4.0] * d, [3.0] * d)
    return {"unit": (None, lg, unit), "tiny": (None, lg, unit), "shift": (None, lg, shifted), "uu": (None, lu, gu), "gu": (None, lg, gu),
            "ug": (None, lu, shifted)}[k]


def cell_descriptors(c):
    prior, local, glob = specs_of(c)
    if c["shape"] == GK:
        from glabcmcmc_amd.examples.GK import GK_set
        model = GK_set(EPS[GK], prior=None if prior is None else make_dist(prior)).descriptor()
        return model, make_dist(local).descriptor(), make_dist(glob).descriptor()
    model, ld, gd = descriptors(dict(epsilon=EPS[c["shape"]], y_obs=y_obs_of(c), local=local, **{"global": glob}))
    if prior is not None:
        model.prior = make_dist(prior).descriptor()
    return model, ld, gd


def reaches_unit(c):
    """glabc_pack.h gauss_unit_config on the cell's specifications: prior = global = N(0, I), a Gaussian local increment, every
    |y_obs_j| >= 2^-6 (the reciprocal of every EPS is a verified one) -- and neither g-and-k nor a Gamma"""
    prior, local, glob = specs_of(c)
    d, yd = dims(c["shape"])
    return (yd == d and prior is None and local[0] == "gauss" and glob == ("gauss", [0.0] * d, [1.0] * d) and
            all(abs(np.float32(v)) >= np.float32(2.0 ** -6) for v in y_obs_of(c)))


@functools.lru_cache(maxsize=None)
def start(shape, positive):
    """(theta0 [n][d], y0 [n][yd]), read-only; `positive`: on the support of a Gamma"""
    d, yd = dims(shape)
    rng = np.random.default_rng(300 + 10 * d + yd + positive)
    if shape == GK:
        theta0 = (np.array([3.0, 1.0, 2.0, 0.5]) * np.exp(0.2 * rng.standard_normal((N_CHAINS, 4)))).astype(np.float32)
        theta0 = np.clip(theta0, np.float32(1.01) * np.array(GK_BOX[1], np.float32), np.float32(0.99) * np.array(GK_BOX[2], np.float32))
        y0 = np.sort(3.0 + 2.0 * rng.standard_normal((N_CHAINS, 8)), axis=1).astype(np.float32)
    else:
        theta0 = (1.5 * rng.standard_normal((N_CHAINS, d))).astype(np.float32)
        if positive:
            theta0 = (np.abs(theta0) + 0.2).astype(np.float32)
        y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((N_CHAINS, d))).astype(np.float32)
    theta0.setflags(write=False)
    y0.setflags(write=False)
    return theta0, y0


def cell_start(c):
    return start(c["shape"], "gamma" in c["kind"])


def frequencies(c, constant=None):
    """(scalar of glabc_run, per-chain array or None)"""
    if constant is not None:
        return SCALAR_WITH_ARRAY, np.full(N_CHAINS, constant, np.float32)
    if c["freq"] is None:
        return SCALAR_ALONE, None
    return SCALAR_WITH_ARRAY, np.array([FREQ_TABLE[(i + c["freq"]) % 16] for i in range(N_CHAINS)], np.float32)


# ------------------------------------------------------------------------------------------------------------ the checker
STATE_KEYS = ("theta", "y", "log_w", "flags", "n_moves")
SUM_KEYS = ("sum_theta", "sum_outer", "sum_jump")
_CHECKER, _COVERAGE = {}, {}


def _key(c, scalar_only):
    return (c["algo"], c["shape"], c["N"], c["kind"], c["T"], c["freq"], c["seed"], c["chain0"], scalar_only)


def checker_case(c, scalar_only=False):
    """The CPU checker's run of the cell on unpadded host arrays, in ONE call of T iterations: every array the entry points own.
    scalar_only: the run with glabc_run.global_frequency = SCALAR_ALONE and no array.  Computed once, never written to."""
    key = _key(c, scalar_only)
    if key in _CHECKER:
        return _CHECKER[key]
    L = oracle_lib.load()
    model, local, glob = cell_descriptors(c)
    theta0, y0 = cell_start(c)
    d = theta0.shape[1]
    isir = c["algo"] == "glmcmc"
    hc = oracle_lib.HostChains(theta0, y0, chain0=c["chain0"], with_isir=isir)
    hist = np.zeros((c["T"], d, N_CHAINS), np.float32)
    mom = oracle_lib.HostMoments(N_CHAINS, d)
    gf, arr = (SCALAR_ALONE, None) if scalar_only else frequencies(c)
    run, keep = oracle_lib.make_run(seed=c["seed"], step0=1, n_steps=c["T"], gf=gf, batch=c["N"], history=hist, moments=mom)
    if arr is not None:
        run.global_frequency_per_chain = arr.ctypes.data
    cs = hc.struct()
    if isir:
        assert L.oracle_init_weights(C.byref(model), C.byref(glob), C.byref(cs)) == 0
        rc = L.oracle_glmcmc_steps(C.byref(model), C.byref(local), C.byref(glob), C.byref(cs), C.byref(run))
    else:
        rc = L.oracle_globalmcmc_steps(C.byref(model), C.byref(local), C.byref(glob), C.byref(cs), C.byref(run))
    assert rc == 0, cell_id(c)
    out = dict(history=hist, theta=hc.theta, y=hc.y, n_moves=hc.n_moves, sum_theta=mom.sum_theta, sum_outer=mom.sum_outer,
               sum_jump=mom.sum_jump)
    if isir:
        out.update(log_w=hc.log_w, flags=hc.flags)
    for a in out.values():
        a.setflags(write=False)
    _CHECKER[key] = out
    return out


def coverage(c):
    """What the checker's run of the cell reaches, from its history and its own candidate draws (oracle_propose: the candidates
    of every chain at one iteration -- Gaussian, Uniform or Gamma -- and the branch each chain takes):
      wins[j]     global moves whose new state is candidate j (GlobalMCMC: its one candidate)
      local       accepted local moves
      branch      [T][n] the chain is on the global branch;  moved  [T][n] the state changed"""
    key = _key(c, False)
    if key in _COVERAGE:
        return _COVERAGE[key]
    L = oracle_lib.load()
    ref = checker_case(c)
    model, local, glob = cell_descriptors(c)
    theta0, y0 = cell_start(c)
    d, yd = dims(c["shape"])
    n, T, N = N_CHAINS, c["T"], c["N"] if c["algo"] == "glmcmc" else 1
    rows = np.concatenate([theta0.T[None], ref["history"]], axis=0)                 # (T + 1, d, n)
    moved = (rows[1:] != rows[:-1]).any(axis=1)                                      # (T, n)
    gf, arr = frequencies(c)
    hc = oracle_lib.HostChains(np.zeros_like(theta0), np.zeros_like(y0), chain0=c["chain0"])
    cs = hc.struct()
    prop, log_q = np.zeros((N * n, d), np.float32), np.zeros(N * n, np.float32)
    log_u, u_res, is_global = np.zeros(n, np.float32), np.zeros(n, np.float64), np.zeros(n, np.int32)
    io = A.StepIO()
    io.n_prop, io.theta_dim, io.y_dim, io.noise_dim = N, d, yd, yd
    io.theta_prop, io.log_q, io.log_u, io.u_res, io.is_global = (a.ctypes.data for a in (prop, log_q, log_u, u_res, is_global))
    branch, wins = np.zeros((T, n), bool), np.zeros(N, np.int64)
    algo = A.ALGO_GLMCMC if c["algo"] == "glmcmc" else A.ALGO_GLOBALMCMC
    for t in range(T):
        run, keep = oracle_lib.make_run(seed=c["seed"], step0=1 + t, n_steps=1, gf=gf, batch=N)
        if arr is not None:
            run.global_frequency_per_chain = arr.ctypes.data
        assert L.oracle_propose(algo, C.byref(local), C.byref(glob), C.byref(cs), C.byref(run), C.byref(io)) == 0
        branch[t] = is_global != 0
        won = branch[t] & moved[t]
        hit = (prop.reshape(N, n, d) == ref["history"][t].T[None]).all(axis=2)      # (N, n)
        assert hit[:, won].any(axis=0).all(), "%s: a global move's new state is none of its candidates" % cell_id(c)
        wins += np.bincount(hit[:, won].argmax(axis=0), minlength=N)
    out = dict(wins=wins, local=int((moved & ~branch).sum()), branch=branch, moved=moved)
    _COVERAGE[key] = out
    return out
