"""The reference chain of glabc_glmala_mix_steps (include/glabc.h), assembled for the tests.

The CPU checker's GLMALA move is hard-wired to a glabc_dist importance proposal, so a chain with a GaussianMixture is put
together iteration by iteration (n_steps = 1):
  1. snapshot the checker's chain arrays;
  2. oracle_glmala_steps on ALL chains with some valid DiagGaussian importance proposal (`filler`): a chain whose branch uniform
     is >= gf took the MALA move, which never reads the proposal -- its result stands;
  3. the chains on the global branch get their snapshot back and the iSIR move of GLMALA.py:152-180 restated here in numpy, as
     include/glabc.h specifies it: the LOCAL refresh of log_w in the state's precision, the candidates, the Model's prior /
     simulator / kernel through the checker's row-wise exports, the weights through oracle_expf_v (float32) or oracle_exp_v
     (float64, once GLABC_FLAG_LW64 is set), NaN -> 0, oracle_aten_rowsum_f32 / _f64 over the N + 1 terms, the running sum of
     w / tot in double against u_res, the state / log_w / n_moves / flag updates, the history row and the three moment sums.
The float64 prior and ABC kernel of a GLABC_FLAG_TH64 state (dist_log_prob_f64 / model_log_kernel_f64 of glabc_mala.h) are plain
IEEE operations and are restated too, their row sums through mixture_ref.rowsum_f64.

What is proposal-specific comes from a candidate PROVIDER: theta' and log q' of the N candidates, and log q of the current state
in either precision.  MixProvider is the mixture (mixture_ref.MixtureRef).  DistProvider is a DiagGaussian or Uniform glabc_dist
through oracle_dist_forward / oracle_dist_log_prob: with it the assembled chain must equal an uninterrupted oracle_glmala_steps
run bit for bit (tests/test_glmala_mix_host.py), which holds the restatement itself to the checker.
"""
import ctypes as C

import numpy as np

import mixture_ref
import oracle_lib
from glabcmcmc_amd import _capi as A

LOG_2PI = 1.8378770664093453                 # GLABC_LOG_2PI, include/glabc_numerics.h
LOCAL, TH64, LW64 = A.FLAG_LOCAL, A.FLAG_TH64, A.FLAG_LW64
STATE_ARRAYS = ("theta", "y", "log_w", "theta64", "y64", "log_w64", "grad", "flags", "n_moves")
COMBOS = ("f32", "th64_w32", "th64_lw64")     # the state slot's precision: state dtype + weight dtype


def _c(a, dt):
    return np.ascontiguousarray(a, dt)


def _vec(t, d, dt=np.float64):
    """a ctypes float array's first d elements: float32 values, promoted exactly"""
    return np.array([t[j] for j in range(d)], np.float32).astype(dt)


# ---- the checker's row-wise exports ------------------------------------------------------------------------------------------
def prior_f32(L, model, th):
    th, out = _c(th, np.float32), np.empty(len(th), np.float32)
    assert L.oracle_model_prior_log_prob(C.byref(model), th.ctypes.data, len(th), out.ctypes.data) == 0
    return out


def kernel_f32(L, model, y):
    y, out = _c(y, np.float32), np.empty(len(y), np.float32)
    assert L.oracle_model_log_kernel(C.byref(model), y.ctypes.data, len(y), out.ctypes.data) == 0
    return out


def simulate(L, model, th, eps):
    th, eps = _c(th, np.float32), _c(eps, np.float32)
    out = np.empty((len(th), model.y_dim), np.float32)
    assert L.oracle_model_simulate(C.byref(model), th.ctypes.data, eps.ctypes.data, len(th), out.ctypes.data) == 0
    return out


def expf(L, x):
    x = _c(x, np.float32)
    out = np.empty_like(x)
    L.oracle_expf_v(x.ctypes.data, x.size, out.ctypes.data)
    return out


def rowsum32(L, w):
    w = _c(w, np.float32)
    return np.array([L.oracle_aten_rowsum_f32(r.ctypes.data, w.shape[1]) for r in w], np.float32)


def rowsum64(L, w):
    w = _c(w, np.float64)
    return np.array([L.oracle_aten_rowsum_f64(r.ctypes.data, w.shape[1]) for r in w], np.float64)


# ---- glabc_mala.h dist_log_prob_f64 / model_log_kernel_f64: plain IEEE double operations ---------------------------------------
def dist_log_prob_f64(g, z):
    d = g.dim
    z = np.asarray(z, np.float64).reshape(-1, d)
    p0, p1, p2 = _vec(g.p0, d), _vec(g.p1, d), _vec(g.p2, d)
    if g.kind == A.DIST_DIAG_GAUSS:
        e = (z - p0) / p2
        t = p1 + 0.5 * (e * e)
        return (-0.5 * float(d) * LOG_2PI) - mixture_ref.rowsum_f64(t)
    assert g.kind == A.DIST_UNIFORM
    out = ((z < p0) | (z > p1)).any(1)
    return np.where(out, -np.inf, float(g.c0))


def model_log_kernel_f64(model, y):
    yd = model.y_dim
    dd = np.asarray(y, np.float64).reshape(-1, yd) - _vec(model.y_obs, yd)
    dis = np.sqrt(mixture_ref.rowsum_f64(dd * dd))
    e = (dis - 0.0) / float(model.kern_scale)
    return (-0.5 * 1.0 * LOG_2PI) - (float(model.kern_log_scale) + 0.5 * (e * e))


# ---- providers -------------------------------------------------------------------------------------------------------------------
class MixProvider:
    """the mixture of a glabc_mixture descriptor, as include/glabc.h specifies it"""

    def __init__(self, desc):
        self.ref = mixture_ref.MixtureRef.from_descriptor(desc)
        self.mode_counts = np.zeros(self.ref.K, np.int64)

    def state_log_q_f32(self, th32):
        return self.ref.log_prob_f32(th32)

    def state_log_q_f64(self, th64):
        return self.ref.log_prob(th64)

    def candidates(self, seed, ids, step, N, draws):
        lo, hi = (ids & np.uint64(0xFFFFFFFF)), (ids >> np.uint64(32))
        for j in range(N):                       # bookkeeping for the conditions on the inputs: which modes were drawn
            w = mixture_ref.philox4x32_10(lo, hi, step, mixture_ref.SLOT_MIX + j, seed & 0xFFFFFFFF, seed >> 32)
            self.mode_counts += np.bincount(self.ref.mode(mixture_ref.uniform_f64(w[0], w[1])), minlength=self.ref.K)
        return self.ref.candidates(seed, ids, step, N, draws.shape[2] - self.ref.d)


class DistProvider:
    """a DiagGaussian / Uniform glabc_dist through the checker's exports, on the draws glabc_glmala_steps reads"""

    def __init__(self, L, desc):
        self.L, self.g = L, desc

    def state_log_q_f32(self, th32):
        th32, out = _c(th32, np.float32), np.empty(len(th32), np.float32)
        assert self.L.oracle_dist_log_prob(C.byref(self.g), th32.ctypes.data, len(th32), out.ctypes.data) == 0
        return out

    def state_log_q_f64(self, th64):
        return dist_log_prob_f64(self.g, th64)

    def candidates(self, seed, ids, step, N, draws):
        n, d = len(ids), self.g.dim
        noise = draws[:, :, :d].copy()                                               # [n][N][d] proposal normals
        if self.g.kind == A.DIST_UNIFORM:
            # words 0..d-1 of the candidate's first block as float32 uniforms (draws_from_philox, prop_uniform)
            yd = draws.shape[2] - d
            spp = (d + (d & 1) + yd + 3) // 4
            lo, hi = (ids & np.uint64(0xFFFFFFFF)), (ids >> np.uint64(32))
            for j in range(N):
                w = mixture_ref.philox4x32_10(lo, hi, step, 1 + j * spp, seed & 0xFFFFFFFF, seed >> 32)
                for q in range(d):
                    a = _c(w[q], np.uint32)
                    u, upos, u64 = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.float64)
                    self.L.oracle_uniforms_v(a.ctypes.data, a.ctypes.data, n, u.ctypes.data, upos.ctypes.data, u64.ctypes.data)
                    noise[:, j, q] = u
        noise = _c(noise.reshape(n * N, d), np.float32)
        z, lq = np.empty((n * N, d), np.float32), np.empty(n * N, np.float32)
        assert self.L.oracle_dist_forward(C.byref(self.g), noise.ctypes.data, n * N, z.ctypes.data, lq.ctypes.data) == 0
        return z.reshape(n, N, d).transpose(1, 0, 2).copy(), lq.reshape(n, N).T.copy()


# ---- the iSIR move of GLMALA.py:152-180 on the rows of a state --------------------------------------------------------------------
def isir_move(L, model, provider, seed, ids, step, N, st, draws, u_res, stats):
    """st: dict of the chains' state (theta64 [n][d], y64 [n][yd], log_w64 [n], flags [n], n_moves [n]), updated in place"""
    n, d = st["theta64"].shape
    flags = st["flags"]
    th32, y32 = st["theta64"].astype(np.float32), st["y64"].astype(np.float32)
    loc, t64 = (flags & LOCAL) != 0, (flags & TH64) != 0
    # :152-156, log_weight_old in the state's precision
    a = loc & t64
    if a.any():
        prior, kern = dist_log_prob_f64(model.prior, st["theta64"][a]), model_log_kernel_f64(model, st["y64"][a])
        st["log_w64"][a] = (prior + kern) - provider.state_log_q_f64(st["theta64"][a])
        flags[a] |= LW64
    b = loc & ~t64
    if b.any():
        q = provider.state_log_q_f32(th32[b])
        st["log_w64"][b] = ((prior_f32(L, model, th32[b]) + kernel_f32(L, model, y32[b])) - q).astype(np.float64)
    flags &= ~np.uint32(LOCAL)                                                                      # :157
    # :158-165
    th_c, lq = provider.candidates(seed, ids, step, N, draws)                                      # [N][n][d], [N][n]
    lw0, y_c = np.empty((N, n), np.float32), np.empty((N, n, model.y_dim), np.float32)
    for j in range(N):
        y_c[j] = simulate(L, model, th_c[j], draws[:, j, d:])
        lw0[j] = (prior_f32(L, model, th_c[j]) + kernel_f32(L, model, y_c[j])) - lq[j]
    # :169-174
    w64 = (flags & LW64) != 0
    ind = np.full(n, -1, np.int64)
    if w64.any():
        m = int(w64.sum())
        w = np.empty((m, N + 1), np.float64)
        w[:, 0] = mixture_ref.glabc_exp(st["log_w64"][w64])
        w[:, 1:] = mixture_ref.glabc_exp(lw0[:, w64].T.astype(np.float64))
        w[np.isnan(w)] = 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            frac = w / rowsum64(L, w)[:, None]
        ind[w64] = _pick(frac, u_res[w64])
    if (~w64).any():
        m = int((~w64).sum())
        w = np.empty((m, N + 1), np.float32)
        w[:, 0] = expf(L, st["log_w64"][~w64].astype(np.float32))
        w[:, 1:] = expf(L, lw0[:, ~w64].T)
        w[np.isnan(w)] = np.float32(0.0)
        with np.errstate(invalid="ignore", divide="ignore"):
            frac = (w / rowsum32(L, w)[:, None]).astype(np.float64)
        ind[~w64] = _pick(frac, u_res[~w64])
    # :175-179
    mv = ind > 0
    rows = np.nonzero(mv)[0]
    st["theta64"][rows] = th_c[ind[rows] - 1, rows].astype(np.float64)
    st["y64"][rows] = y_c[ind[rows] - 1, rows].astype(np.float64)
    st["log_w64"][rows] = lw0[ind[rows] - 1, rows].astype(np.float64)
    st["n_moves"][rows] += 1
    if stats is not None:
        combo = np.where(~t64, 0, np.where(w64, 2, 1))
        assert not (~t64 & w64).any()                     # a float32 state never has float64 weights
        for k, name in enumerate(COMBOS):
            stats[name] += int((combo == k).sum())
            stats[name + "_moved"] += int(((combo == k) & mv).sum())
        stats["stay"] += int((ind <= 0).sum())
        stats["none"] += int((ind < 0).sum())
        stats["zero_weight"] += int((lw0 == -np.inf).sum())
        stats["all_zero_weight"] += int((lw0 == -np.inf).all(0).sum())
    return ind


def _pick(frac, u):
    """the first k with u < the running double sum of frac[:, k], else -1"""
    ind = np.full(len(u), -1, np.int64)
    acc = np.zeros(len(u), np.float64)
    for k in range(frac.shape[1]):
        acc = acc + frac[:, k]
        ind = np.where((ind < 0) & (u < acc), k, ind)
    return ind


def new_stats():
    s = {k: 0 for k in COMBOS}
    s.update({k + "_moved": 0 for k in COMBOS})
    s.update(stay=0, none=0, zero_weight=0, all_zero_weight=0, both_branches_in_a_wavefront=0, global_steps=0, local_steps=0)
    return s


def step_draws(L, seed, ids, step, N, d, yd):
    """(branch uniforms f32 [n], resampling uniforms f64 [n], normals [n][N][d + yd]) of the chains at one iteration"""
    n = len(ids)
    ub, ur, zz = np.empty(n, np.float32), np.empty(n, np.float64), np.empty((n, N, d + yd), np.float32)
    u2, r = np.empty(2, np.float32), np.empty(1, np.float64)
    for i in range(n):
        L.oracle_step_draws(C.c_uint64(int(seed)), C.c_uint64(int(ids[i])), int(step), N, d, yd, u2.ctypes.data, r.ctypes.data,
                            zz[i].ctypes.data)
        ub[i], ur[i] = u2[0], r[0]
    return ub, ur, zz


def assemble(L, model, mala, provider, filler, theta0, y0, *, seed, chain0, T, N, gf, stats=None):
    """glabc_glmala_init + T iterations of the assembled chain -> every array the device entry points own"""
    n, d = theta0.shape
    yd = model.y_dim
    hc = oracle_lib.HostChains(theta0, y0, chain0=chain0).add_mala_state()
    hist = np.zeros((T, d, n), np.float32)
    mom = oracle_lib.HostMoments(n, d)
    cs = hc.struct()
    assert L.oracle_glmala_init(C.byref(model), C.byref(cs)) == 0
    ids = np.uint64(chain0) + np.arange(n, dtype=np.uint64)
    gf32 = np.float32(gf)
    tri = [(p, q) for p in range(d) for q in range(p, d)]
    for t in range(T):
        step = 1 + t
        snap = {k: getattr(hc, k).copy() for k in STATE_ARRAYS}
        msnap = {k: getattr(mom, k).copy() for k in ("sum_theta", "sum_outer", "sum_jump")}
        run, keep = oracle_lib.make_run(seed=seed, step0=step, n_steps=1, gf=gf, batch=N, history=hist[t], moments=mom)
        assert L.oracle_glmala_steps(C.byref(model), C.byref(filler), C.byref(mala), C.byref(cs), C.byref(run)) == 0
        ub, ur, zz = step_draws(L, seed, ids, step, N, d, yd)
        g = np.nonzero(ub < gf32)[0]                                                  # GLMALA.py:151
        if stats is not None:
            stats["global_steps"] += len(g)
            stats["local_steps"] += n - len(g)
            for w0 in range(0, n, 64):
                k = int((ub[w0:w0 + 64] < gf32).sum())
                stats["both_branches_in_a_wavefront"] += int(0 < k < len(ub[w0:w0 + 64]))
        if len(g) == 0:
            continue
        st = dict(theta64=snap["theta64"][:, g].T.copy(), y64=snap["y64"][:, g].T.copy(), log_w64=snap["log_w64"][g].copy(),
                  flags=snap["flags"][g].copy(), n_moves=snap["n_moves"][g].copy())
        prev = st["theta64"].astype(np.float32)
        isir_move(L, model, provider, seed, ids[g], step, N, st, zz[g], ur[g], stats)
        hc.theta64[:, g], hc.y64[:, g], hc.log_w64[g] = st["theta64"].T, st["y64"].T, st["log_w64"]
        hc.theta[:, g], hc.y[:, g] = st["theta64"].T.astype(np.float32), st["y64"].T.astype(np.float32)
        hc.log_w[g] = st["log_w64"].astype(np.float32)
        hc.grad[:, g] = snap["grad"][:, g]
        hc.flags[g], hc.n_moves[g] = st["flags"], st["n_moves"]
        cur = st["theta64"].astype(np.float32)                                        # Theta_Re is float32, :148,180
        hist[t][:, g] = cur.T
        c64, p64 = cur.astype(np.float64), prev.astype(np.float64)
        mom.sum_theta[:, g] = msnap["sum_theta"][:, g] + c64.T
        for k, (p, q) in enumerate(tri):
            # glabc_add_prod_f32: the product of two float32 values is exact in double, so fused or not it rounds once
            mom.sum_outer[k, g] = msnap["sum_outer"][k, g] + c64[:, p] * c64[:, q]
            mom.sum_jump[k, g] = msnap["sum_jump"][k, g] + (c64[:, p] - p64[:, p]) * (c64[:, q] - p64[:, q])
    return dict(history=hist, theta=hc.theta, y=hc.y, log_w=hc.log_w, theta64=hc.theta64, y64=hc.y64, log_w64=hc.log_w64,
                grad=hc.grad, flags=hc.flags, n_moves=hc.n_moves, sum_theta=mom.sum_theta, sum_outer=mom.sum_outer,
                sum_jump=mom.sum_jump)


def uninterrupted(L, model, mala, imp, theta0, y0, *, seed, chain0, T, N, gf):
    """oracle_glmala_init + one oracle_glmala_steps call of T iterations with a glabc_dist importance proposal"""
    n, d = theta0.shape
    hc = oracle_lib.HostChains(theta0, y0, chain0=chain0).add_mala_state()
    hist = np.zeros((T, d, n), np.float32)
    mom = oracle_lib.HostMoments(n, d)
    run, keep = oracle_lib.make_run(seed=seed, step0=1, n_steps=T, gf=gf, batch=N, history=hist, moments=mom)
    cs = hc.struct()
    assert L.oracle_glmala_init(C.byref(model), C.byref(cs)) == 0
    assert L.oracle_glmala_steps(C.byref(model), C.byref(imp), C.byref(mala), C.byref(cs), C.byref(run)) == 0
    return dict(history=hist, theta=hc.theta, y=hc.y, log_w=hc.log_w, theta64=hc.theta64, y64=hc.y64, log_w64=hc.log_w64,
                grad=hc.grad, flags=hc.flags, n_moves=hc.n_moves, sum_theta=mom.sum_theta, sum_outer=mom.sum_outer,
                sum_jump=mom.sum_jump)
