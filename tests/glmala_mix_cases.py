"""The cases of the glabc_glmala_mix_steps tests and their reference chains (tests/mala_mix_ref.py), computed once and shared by
tests/test_glmala_mix_host.py (the conditions on the inputs, no GPU) and tests/test_glmala_mix_shapes.py (GPU parity)."""
import numpy as np

import mala_mix_ref as ref
from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import distribution
from helpers import AbsGaussModel, make_dist
from test_glmala_shapes import y_obs_of
from test_mixture_host import make_mixture

EPS, TAU = 0.3, 0.25
MODES = (1, 3, 4, 5, 8)                          # the branches of the logsumexp sum order (glabc_device.h mix_log_prob)
GFS = (0.3, 0.5, 0.8, 1.0)


def make_case(d, N, K, n, T, gf, num, y_kind, seed, prior="gauss", lanes=0, spl=None, pad=0, hist_pad=0, outside=False):
    return dict(d=d, N=N, K=K, n=n, T=T, gf=gf, num=num, y_kind=y_kind, seed=seed, prior=prior, lanes=lanes,
                spl=spl or (7 if T % 7 else 5), pad=pad, hist_pad=hist_pad, outside=outside,
                chain0=((N + 1) << 33) + d * 1000003)                   # above 2^32: both Philox counter words in use


def case_id(c):
    return "d%d-N%d-K%d-gf%g-num%d-%s-%s%s" % (c["d"], c["N"], c["K"], c["gf"], c["num"], c["y_kind"], c["prior"],
                                               "-lanes%d" % c["lanes"] if c["lanes"] else "")


def y_obs(c):
    return y_obs_of(c["d"], c["y_kind"])


def lean(c):
    return all(abs(np.float32(v)) >= np.float32(2.0 ** -6) for v in y_obs(c))


def mixture(c):
    d, K = c["d"], c["K"]
    if c["outside"]:
        # a Uniform(-2, 2)^d prior and a narrow mode at 3.5: its candidates have prior -inf, weight 0; with 40 % of the mass there
        # one iteration in a hundred draws all N = 5 candidates from it
        assert K == 4
        loc = np.array([[1.5] * d, [-1.5] * d, [0.2] * d, [3.5] * d])
        scale = np.array([[0.5] * d, [0.6] * d, [0.9] * d, [0.2] * d])
        return distribution.GaussianMixture(K, d, loc=loc, scale=scale, weights=[0.25, 0.2, 0.15, 0.4])
    return make_mixture(K, d, spread=1.5)                              # centres at -1.5 / 0 / 1.5 per coordinate


def model_object(c):
    m = AbsGaussModel(EPS, y_obs(c))
    d = c["d"]
    if c["prior"] == "uniform":
        m._prior = lambda: make_dist(("uniform", [-2.0] * d, [2.0] * d))
    return m


def descriptors(c):
    """(model, mixture, mala, filler): filler is the DiagGaussian the checker's step runs with (mala_mix_ref.assemble)"""
    d = c["d"]
    filler = make_dist(("gauss", [0.05 * j for j in range(d)], [1.1] * d)).descriptor()
    mala = A.Mala(TAU, TAU ** 2, EPS ** 2, int(c["num"]), 0)           # GLMALA.py:43,90: Python floats
    return model_object(c).descriptor(), mixture(c).descriptor(), mala, filler


def inputs(c):
    rng = np.random.default_rng(c["seed"])
    theta0 = (1.2 * rng.standard_normal((c["n"], c["d"]))).astype(np.float32)
    y0 = (np.abs(theta0) + 0.2236068 * rng.standard_normal((c["n"], c["d"]))).astype(np.float32)
    return theta0, y0


_REF = {}


def reference(oracle, c):
    """(arrays, stats, times each mode was drawn) of a case, computed once; lanes / launch cuts / strides do not enter"""
    key = tuple((k, repr(c[k])) for k in sorted(c) if k not in ("lanes", "spl", "pad", "hist_pad"))
    if key not in _REF:
        model, mix, mala, filler = descriptors(c)
        theta0, y0 = inputs(c)
        prov, stats = ref.MixProvider(mix), ref.new_stats()
        r = ref.assemble(oracle, model, mala, prov, filler, theta0, y0, seed=c["seed"], chain0=c["chain0"], T=c["T"], N=c["N"],
                         gf=c["gf"], stats=stats)
        for a in r.values():
            a.setflags(write=False)
        _REF[key] = (r, stats, prov.mode_counts)
    return _REF[key]


def _sweep():
    out = []
    for d in (1, 2, 3, 4):
        for N in range(1, 17):
            for v, y_kind in enumerate(("away", "zero")):
                T = 8 + (N + d + v) % 5
                c = make_case(d, N, K=MODES[(N + d + 2 * v) % 5], n=65, T=T, gf=GFS[(N + v) % 4], num=2 + (3 * N + d + v) % 8,
                              y_kind=y_kind, seed=7000 + 100 * d + 2 * N + v, spl=3 if T % 3 else 5, pad=(N % 3) * 3,
                              hist_pad=(d - 1) * 2)
                out += [dict(c, lanes=l) for l in ((1, 2) if d == 2 else (0,))]
    return out


SWEEP = _sweep()

# one per theta_dim: both branches meet in one wavefront in one iteration; theta_dim 2 at both launch geometries; the Uniform prior
# with a mode outside its support
DEEP = [make_case(1, 5, 3, 130, 60, 0.5, 9, "zero", 11, pad=3),
        make_case(2, 5, 4, 130, 60, 0.5, 7, "away", 12, lanes=1, hist_pad=2),
        make_case(2, 5, 4, 130, 60, 0.5, 7, "away", 12, lanes=2, pad=1),
        make_case(3, 5, 5, 130, 60, 0.5, 5, "away", 13, pad=2, hist_pad=1),
        make_case(4, 5, 8, 130, 60, 0.5, 6, "zero", 14),
        make_case(2, 5, 4, 130, 60, 0.5, 8, "zero", 15, prior="uniform", outside=True, pad=5),
        make_case(3, 5, 4, 130, 60, 0.5, 4, "away", 16, prior="uniform", outside=True)]
