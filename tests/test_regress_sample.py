"""glabcmcmc_amd.regression end to end on the GPU: on the rows ``rejection.sample`` returns for the built-in g-and-k Model and for a
CompiledModel with y_dim != theta_dim, and on the weighted particles of ``smc.sample``.

The Gram of ``adjust(path="auto")`` is the restatement's (tests/regress_ref.py) bit for bit on the same arrays, so alpha, beta and the
covariance equal ``fit`` of the restatement's Gram exactly, and the adjusted theta is the restatement's apply bit for bit.
``path="generic"`` on the same arrays agrees within the bounds of tests/test_regress_host.py: the Gram within the addition bound, B
within FIT_TOLERANCE cond(G) 2^-52 ||B||.
"""
import math

import numpy as np
import pytest
import torch

import regress_ref as R
from glabcmcmc_amd import regression, rejection, smc
from glabcmcmc_amd.compiled import CompiledModel
from glabcmcmc_amd.examples.GK import GK_set
from glabcmcmc_amd.examples.Mixture import Mixture_set
from helpers import make_dist
from test_regress_host import EPS, FIT_TOLERANCE
from test_rtc import NONLINEAR

pytestmark = pytest.mark.gpu

SEED = 0x5EEDC0FFEE123457


def check_against_restatement(model, draws, a, theta_dim, y_dim):
    """the bit checks of one ``adjust(path="auto")`` result `a` on a Rejection -> (the restatement's Gram, row weights, design)"""
    n = draws.theta.shape[0]
    theta, y, dis = draws.theta.cpu().numpy().T, draws.y.cpu().numpy().T, draws.distance.cpu().numpy()
    y_obs = model.y_obs.numpy().reshape(-1).astype(np.float64)
    assert a.delta == float(dis.max())
    want, _ = R.weighted_gram(theta, y, dis, None, n, y_obs, a.delta, R.EPANECHNIKOV)
    assert R.same_bits(a.gram, want)
    f = regression.fit(want, theta_dim, y_dim)
    assert np.array_equal(a.alpha, f.alpha) and np.array_equal(a.beta, f.beta) and np.array_equal(a.covariance, f.covariance)
    assert a.ess == f.ess and np.array_equal(a.mean, a.alpha)
    assert a.theta.shape == (n, theta_dim) and a.theta.dtype == torch.float32 and a.theta.is_cuda
    assert R.same_bits(a.theta.cpu().numpy().T, R.regression_apply(theta, y, n, y_obs, f.beta))
    w = R.row_weights(dis, None, n, a.delta, R.EPANECHNIKOV)
    # two float64 sums of the same n positive numbers in different orders, each within (n - 1) 2^-53 of the exact sum
    assert np.allclose(a.weights.cpu().numpy(), w / w.sum(), rtol=2 * n * EPS, atol=0)
    return want, w, R.design(theta, y, n, y_obs)


def check_generic(model, draws, a, want, w, z, theta_dim, y_dim):
    g = regression.adjust(model, (draws.theta.cpu(), draws.y.cpu(), draws.distance.cpu()), path="generic")
    assert (np.abs(g.gram - want) <= R.addition_bound(R.row_terms(z, w), w)).all()
    x = z[:, :1 + y_dim] * np.sqrt(w)[:, None]
    cond = np.linalg.cond(x.T @ x)
    assert np.linalg.norm(g.beta - a.beta) <= FIT_TOLERANCE * cond * EPS * np.linalg.norm(a.beta)
    assert not g.theta.is_cuda and np.abs(g.theta.numpy() - a.theta.cpu().numpy()).max() <= 1e-5 * np.abs(a.theta.cpu().numpy()).max()
    assert math.isclose(g.outside_prior, a.outside_prior, abs_tol=2.0 / draws.theta.shape[0])


def test_gk_end_to_end(hip):
    model = GK_set(0.5)
    draws = rejection.sample(model, 1 << 18, kernel="hard", quantile=0.05, seed=SEED)
    assert draws.theta.is_cuda and draws.theta.shape[0] > 13000
    before = draws.theta.clone()
    a = regression.adjust(model, draws, path="auto")
    assert torch.equal(draws.theta, before)                          # not in place
    want, w, z = check_against_restatement(model, draws, a, 4, 8)
    check_generic(model, draws, a, want, w, z, 4, 8)
    wt = torch.from_numpy(w / w.sum())
    raw = draws.theta[:, 0].double().cpu()
    adj = a.theta[:, 0].double().cpu()
    raw_sd = math.sqrt(float((wt * (raw - (wt * raw).sum()) ** 2).sum()))
    adj_sd = math.sqrt(float((wt * (adj - (wt * adj).sum()) ** 2).sum()))
    print("sd of A: raw %.3f, adjusted %.3f; outside the prior %.3f; ess %.0f" % (raw_sd, adj_sd, a.outside_prior, a.ess))
    assert adj_sd < raw_sd
    assert math.isclose(adj_sd ** 2, a.covariance[0, 0], rel_tol=1e-4)   # the Gram's residual covariance is the adjusted draws'
    assert 0.0 < a.outside_prior < 1.0
    # a quantile of the kept distances as delta, and terms / combine / fit / apply by hand on two shards
    b = regression.adjust(model, draws, quantile=0.5)
    assert b.delta < a.delta and int((b.weights > 0).sum()) <= draws.theta.shape[0] // 2 + 1
    n, half = draws.theta.shape[0], 5000
    parts = [regression.terms(draws.theta[s], draws.y[s], draws.distance[s], y_obs=model.y_obs, delta=a.delta)
             for s in (slice(0, half), slice(half, n))]
    whole = regression.combine(parts)
    assert (np.abs(whole - a.gram) <= R.addition_bound(R.row_terms(z, w), w)).all()


def test_population_weights_enter_the_gram(hip):
    model = Mixture_set(0.05)
    pop = smc.sample(model, 1024, kernel="hard", epsilon=0.3, seed=SEED)
    assert pop.theta.shape == (1024, 2)
    a = regression.adjust(model, pop, kernel="uniform", delta=math.inf)
    theta, y = pop.theta.cpu().numpy().T, pop.y.cpu().numpy().T
    weight = pop.weights.to(torch.float32).cpu().numpy()
    y_obs = model.y_obs.numpy().reshape(-1).astype(np.float64)
    want, _ = R.weighted_gram(theta, y, pop.distance.cpu().numpy(), weight, 1024, y_obs, math.inf, R.UNIFORM)
    assert R.same_bits(a.gram, want)
    plain, _ = R.weighted_gram(theta, y, None, None, 1024, y_obs, math.inf, R.UNIFORM)
    assert not np.array_equal(plain, want)
    assert a.ess <= float(pop.ess) * (1 + 1e-6)
    assert math.isclose(a.ess, 1.0 / float((pop.weights.double() ** 2).sum()), rel_tol=1e-5)
    assert a.theta.shape == (1024, 2) and torch.isfinite(a.theta).all()


def test_compiled_model_rows(hip):
    model = CompiledModel(3, 2, NONLINEAR, make_dist(("gauss", [0.0, 0.5, 0.0], [1.5, 1.0, 2.0])), [0.9, 0.6], 0.15, noise_dim=4)
    draws = rejection.sample(model, 1 << 16, kernel="hard", quantile=0.1, seed=SEED, path="fused")
    assert draws.theta.shape[1] == 3 and draws.y.shape[1] == 2 and draws.theta.is_cuda
    a = regression.adjust(model, draws)
    want, w, z = check_against_restatement(model, draws, a, 3, 2)
    check_generic(model, draws, a, want, w, z, 3, 2)
