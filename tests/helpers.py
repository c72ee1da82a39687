"""Shared helpers for the tests: golden loading, descriptor construction, output canaries."""
import os

import numpy as np
import torch

from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import distribution
from glabcmcmc_amd.examples.Mixture import Mixture_set

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as f:
        g = {k: f[k] for k in f.files}
    if "cfg" in g:
        g["cfg"] = eval(str(g["cfg"]), {"__builtins__": {}}, {"dict": dict})     # repr() of a plain dict
    return g


def make_dist(spec):
    """('gauss', loc, scale) / ('uniform', low, high) / ('gamma', shape, rate) -> host-mirror distribution object"""
    kind = spec[0]
    if kind == "gamma":
        return distribution.Gamma(torch.tensor(spec[1], dtype=torch.float32), torch.tensor(spec[2], dtype=torch.float32))
    if kind == "gauss":
        return distribution.DiagGaussian(len(spec[1]), torch.tensor(spec[1], dtype=torch.float32),
                                         torch.log(torch.tensor(spec[2], dtype=torch.float32)))
    if kind == "uniform":
        return distribution.Uniform(len(spec[1]), torch.tensor(spec[1], dtype=torch.float32),
                                    torch.tensor(spec[2], dtype=torch.float32))
    raise ValueError(kind)


class AbsGaussModel(Mixture_set):
    """Mixture_set at d parameters: y = |theta| + N(0, 0.05 I), prior N(0, I), `y_obs` given (d = len(y_obs)) -- the Model
    of the d-parameter GLMALA fixtures (tests/golden/make_golden.py AbsGauss_set) on the build's side, and a user's
    descriptor Model of another dimension than 2."""

    def __init__(self, epsilon, y_obs):
        super().__init__(epsilon)
        self.theta_dim = len(y_obs)
        self.y_obs = torch.tensor([list(y_obs)], dtype=torch.float32)
        self.y_dim = self.theta_dim

    def _likelihood(self):
        d = self.theta_dim
        return distribution.DiagGaussian(d, torch.tensor([0.0] * d), torch.log(torch.tensor([0.05] * d).sqrt()))

    def _prior(self):
        d = self.theta_dim
        return distribution.DiagGaussian(d, torch.tensor([0.0] * d), torch.tensor([0.0] * d))


def model_y_obs(cfg):
    """y_obs of a d-parameter configuration ('y_obs', or 'dim' alone: 1.5 everywhere); None = the 2-parameter Mixture_set"""
    if "y_obs" in cfg:
        return list(cfg["y_obs"])
    return [1.5] * cfg["dim"] if "dim" in cfg else None


def descriptors(cfg, consts=None):
    """(model, local, global) descriptors of a test configuration; cfg['y_obs'] / cfg['dim'] select the d-parameter
    |theta| + noise Model (AbsGaussModel), without them the reference's Mixture_set.  `consts` = a golden fixture: the
    host-computed float32 constants (exp(log_scale), log(eps) ...) are then taken from the fixture, i.e.
    the values the reference computed on the machine that generated the golden chains -- torch's CPU
    log / exp differ in the last bits between CPU types, and GLMALA's chains depend on them."""
    gk = cfg.get("model") == "gk"
    if gk:
        from glabcmcmc_amd.examples.GK import GK_set
        model = GK_set(cfg["epsilon"]).descriptor()
    elif model_y_obs(cfg) is not None:
        model = AbsGaussModel(cfg["epsilon"], model_y_obs(cfg)).descriptor()
    else:
        model = Mixture_set(cfg["epsilon"]).descriptor()
    local, glob = make_dist(cfg["local"]).descriptor(), make_dist(cfg["global"]).descriptor()
    if consts is not None:
        for j in range(0 if gk else model.theta_dim):
            model.noise.p1[j] = float(consts["c_noise_log_scale"][j])
            model.noise.p2[j] = float(consts["c_noise_scale"][j])
        model.kern_log_scale = float(consts["c_kern_log_scale"][0])
        model.kern_scale = float(consts["c_kern_scale"][0])
        for d, tag in ((local, "local"), (glob, "global")):
            if "c_%s_p1" % tag in consts:
                for j in range(d.dim):
                    d.p1[j] = float(consts["c_%s_p1" % tag][j])
                    d.p2[j] = float(consts["c_%s_p2" % tag][j])
    return model, local, glob


SAMPLER_GOLDENS = [
    "glmcmc_philox_bench", "glmcmc_philox_n8", "glmcmc_philox_n1", "glmcmc_philox_n3", "glmcmc_philox_n16",
    "glmcmc_philox_n32", "glmcmc_philox_n100",
    "glmcmc_philox_uniform", "globalmcmc_philox_bench", "globalmcmc_philox_wide",
    "glmcmc_tape_small", "globalmcmc_tape_small",
    "glmcmc_philox_gk", "glmcmc_philox_gk_gauss", "globalmcmc_philox_gk",
]

# reference run with a correctly rounded torch.sqrt (see make_golden.py): bit parity expected
GLMALA_GOLDENS_EXACT = ["glmala_philox_bench_ieee", "glmala_philox_local_ieee", "glmala_philox_uniform_ieee",
                        "glmala_philox_allglobal"]
# reference run as-is (torch.sqrt = MKL VML, 1 ulp low for 0.65 % of float32 inputs): parity until the
# first sqrt-ulp event of a chain, which the float32 finite-difference prior gradient then amplifies
GLMALA_GOLDENS_MKL = ["glmala_philox_bench", "glmala_philox_local", "glmala_philox_alllocal", "glmala_philox_uniform"]
GLMALA_GOLDENS = GLMALA_GOLDENS_EXACT + GLMALA_GOLDENS_MKL
# theta_dim 1, 3, 4 (make_golden.py AbsGauss_set, correctly rounded sqrt): the general branch of the cooperative gradient
GLMALA_GOLDENS_DIMS = ["glmala_philox_dim1_ieee", "glmala_philox_dim3_ieee", "glmala_philox_dim4_ieee",
                       "glmala_philox_dim4_away_ieee"]


def mala_params(cfg):
    """glabc_mala with tau**2 and epsilon**2 evaluated in Python floats, as GLMALA.py:43,90 do"""
    from glabcmcmc_amd import _capi as A
    return A.Mala(float(cfg["tau"]), float(cfg["tau"]) ** 2, float(cfg["epsilon"]) ** 2, int(cfg["num_grad"]), 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- canaries: what an output buffer holds before the call (tests/test_pool_shapes.py, tests/test_glmala_shapes.py).  After
# GLABC_OK no element the entry point owns may still hold it, after an error every element must.
CANARY_BITS = 0xFFC0DEAD                 # float32: a negative quiet NaN with payload 0xDEAD
CANARY_BITS64 = 0xFFF8DEADC0DEDEAD        # float64: a negative quiet NaN with a payload no arithmetic produces
CANARY_I64 = -0x0DEAD0C0DE0DEAD
CANARY_I32 = -0x0DEAD0C


def canary_f32(*shape):
    return np.full(shape, CANARY_BITS, np.uint32).view(np.float32)


def canary_f64(*shape):
    return np.full(shape, CANARY_BITS64, np.uint64).view(np.float64)


def canary_i64(*shape):
    return np.full(shape, CANARY_I64, np.int64)


def canary_i32(*shape):
    return np.full(shape, CANARY_I32, np.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def canary_left(a):
    """number of elements that still hold the canary"""
    a = np.asarray(a)
    if a.dtype == np.float32:
        return int((np.ascontiguousarray(a).view(np.uint32) == CANARY_BITS).sum())
    if a.dtype == np.float64:
        return int((np.ascontiguousarray(a).view(np.uint64) == CANARY_BITS64).sum())
    return int((a == (CANARY_I64 if a.dtype == np.int64 else CANARY_I32)).sum())


def assert_written(*arrays):
    for a in arrays:
        assert canary_left(a) == 0, "%d of %d elements were never written" % (canary_left(a), np.asarray(a).size)


def assert_untouched(*arrays):
    for a in arrays:
        assert canary_left(a) == np.asarray(a).size, "an entry point that returned an error wrote to its output"


# ---- KernelDensity: the checker's fit, the glabc_kde descriptor over host arrays, the rule-of-thumb factor
def oracle_fit(oracle, X, w, h, bw_fixed):
    n, d = X.shape
    xs = np.ascontiguousarray(X.T)
    weights, log_w = np.empty(n, np.float32), np.empty(n, np.float32)
    wq, consts = np.empty(n, np.int64), np.empty(d + 2, np.float32)
    bwp = None if bw_fixed is None else np.ascontiguousarray(bw_fixed, np.float32).ctypes.data
    rc = oracle.oracle_kde_fit(xs.ctypes.data, None if w is None else w.ctypes.data, n, d, float(h), bwp, weights.ctypes.data,
                               log_w.ctypes.data, wq.ctypes.data, consts.ctypes.data)
    assert rc == 0
    return xs, weights, log_w, wq, consts


def kde_struct(xs, log_w, cum_q, consts, d, n):
    k = A.Kde()
    k.dim, k.n_samples = d, n
    k.x, k.log_w = xs.ctypes.data, log_w.ctypes.data
    k.cum_q = None if cum_q is None else cum_q.ctypes.data
    for j in range(d):
        k.bandwidth[j] = float(consts[j])
    k.sum_log_bw, k.c_2pi = float(consts[d]), float(consts[d + 1])
    return k


def rule(kind, n, d):
    return (n * (d + 2) / 4.) ** (-1. / (d + 4)) if kind == "silverman" else n ** (-1. / (d + 4))
