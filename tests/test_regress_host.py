"""ABC regression adjustment on the host: the NumPy restatement of glabc_weighted_gram (tests/regress_ref.py) against an independent
computation, ``regression.fit`` against numpy.linalg.lstsq, a linear-Gaussian Model whose adjusted draws are exact posterior draws,
and the edges of ``fit`` / ``combine``.  Everything here runs ``path="generic"`` on CPU tensors: no GPU.

Tolerances.
  * Gram against X^T diag(w) X: per statistic (number of additions) 2^-53 sum |term| (regress_ref.addition_bound), the bound of a
    float64 sum of those terms in any order.
  * B of ``fit`` against lstsq on the sqrt(w)-scaled design: FIT_TOLERANCE cond(G) 2^-52 ||B||, G the weighted Gram of the design
    (1, y - y_obs) -- both solvers are backward stable, so each is within a modest multiple of cond 2^-52 of the exact B; ``fit``
    centres first, which costs at most the conditioning of G itself.  The g-and-k inputs have cond(G) <= 10^4 (asserted).
  * Known answer: 5 standard errors, one fixed seed.
"""
import math

import numpy as np
import pytest
import torch

import regress_ref as R
from glabcmcmc_amd import distribution, regression, rejection
from glabcmcmc_amd.examples.GK import GK_set

FIT_TOLERANCE = 100.0           # units of cond(G) 2^-52 ||B||; at most 1000
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def gk_rows():
    """g-and-k prior draws on the CPU, the nearest 5 %: theta (n, 4), y (n, 8), distance (n,), the Model"""
    torch.manual_seed(11)
    model = GK_set(0.5)
    theta = 10.0 * torch.rand(1 << 15, 4)
    y = model.generate_samples(theta)
    dis = model.discrepancy(y)
    keep = torch.nonzero(dis <= torch.quantile(dis, 0.05)).view(-1)
    return theta[keep].contiguous(), y[keep].contiguous(), dis[keep].contiguous(), model


def restated(theta, y, dis, weight, y_obs, delta, kind):
    n = theta.shape[0]
    return R.weighted_gram(theta.numpy().T, y.numpy().T, None if dis is None else dis.numpy(), weight, n, y_obs, delta, kind)


@pytest.mark.parametrize("kind", [R.EPANECHNIKOV, R.UNIFORM])
def test_restatement_equals_matrix_product(gk_rows, kind):
    theta, y, dis, model = gk_rows
    n = theta.shape[0]
    y_obs = model.y_obs.numpy().reshape(-1).astype(np.float64)
    delta = float(dis.max())
    weight = np.linspace(0.5, 1.5, n).astype(np.float32)
    g, partial = restated(theta, y, dis, weight, y_obs, delta, kind)
    assert partial.shape == ((n + 1023) // 1024, R.n_stats(4, 8)) and g.shape == (R.n_stats(4, 8),)
    w = R.row_weights(dis.numpy(), weight, n, delta, kind)
    z = R.design(theta.numpy().T, y.numpy().T, n, y_obs)
    m = z.T @ (w[:, None] * z)                                      # the independent computation: BLAS, its own order
    want = np.concatenate([m[np.triu_indices(13)], [w @ w]])
    bound = R.addition_bound(R.row_terms(z, w), w)
    err = np.abs(g - want)
    print("largest error / bound: %.3g" % (err / bound).max())
    assert (err <= bound).all(), (err / bound).max()
    # the generic path of the module: torch's sums of the same terms
    got = regression.terms(theta, y, dis, torch.from_numpy(weight), y_obs=model.y_obs, delta=delta,
                           kernel="epanechnikov" if kind == R.EPANECHNIKOV else "uniform", path="generic")
    assert (np.abs(got - g) <= bound).all()


def test_fit_equals_lstsq(gk_rows):
    theta, y, dis, model = gk_rows
    n = theta.shape[0]
    y_obs = model.y_obs.numpy().reshape(-1).astype(np.float64)
    delta = float(dis.max())
    g, _ = restated(theta, y, dis, None, y_obs, delta, R.EPANECHNIKOV)
    f = regression.fit(g, 4, 8)
    w = R.row_weights(dis.numpy(), None, n, delta, R.EPANECHNIKOV)
    x = R.design(theta.numpy().T, y.numpy().T, n, y_obs)[:, :9]
    sw = np.sqrt(w)[:, None]
    coef = np.linalg.lstsq(sw * x, sw * theta.numpy().astype(np.float64), rcond=None)[0]
    cond = np.linalg.cond((sw * x).T @ (sw * x))
    print("cond(G) = %.3g" % cond)
    assert cond <= 1e4
    tol = FIT_TOLERANCE * cond * EPS * np.linalg.norm(coef[1:])
    print("|B - lstsq| = %.3g, tolerance %.3g" % (np.linalg.norm(f.beta - coef[1:]), tol))
    assert np.linalg.norm(f.beta - coef[1:]) <= tol
    assert np.linalg.norm(f.alpha - coef[0]) <= FIT_TOLERANCE * cond * EPS * np.linalg.norm(coef)
    assert np.array_equal(f.mean, f.alpha)
    resid = theta.numpy().astype(np.float64) - x @ coef
    cov = (w[:, None] * resid).T @ resid / w.sum()
    assert np.allclose(f.covariance, cov, rtol=0, atol=FIT_TOLERANCE * cond * EPS * np.abs(np.cov(theta.numpy().T)).max())
    assert math.isclose(f.ess, w.sum() ** 2 / (w * w).sum(), rel_tol=1e-12)


# ---- known answer: theta ~ N(0, I), y = theta + 0.5 noise.  The posterior is N(y_obs / 1.25, 0.2 I) and the regression of theta on y
# is exactly linear with B = 0.8 I and Gaussian residuals independent of y: the adjusted draws are exact posterior draws
class LinearGaussian:
    theta_dim = y_dim = 2
    epsilon = 0.1

    def __init__(self):
        self.y_obs = torch.tensor([[1.0, -0.5]])

    def generate_samples(self, theta, num_samples=1):
        return theta + 0.5 * torch.randn_like(theta)

    def discrepancy(self, y):
        return ((y.reshape(-1, 2) - self.y_obs) ** 2).sum(1).sqrt()

    def prior_log_prob(self, samples):
        return -math.log(2 * math.pi) - 0.5 * (samples.reshape(-1, 2) ** 2).sum(1)


@pytest.fixture(scope="module")
def linear_draws():
    torch.manual_seed(2026)
    model = LinearGaussian()
    prior = distribution.DiagGaussian(2, torch.zeros(2), torch.zeros(2))
    return model, rejection.sample(model, 65536, kernel="hard", quantile=1.0, path="generic", prior=prior)


def test_known_answer_uniform(linear_draws):
    model, draws = linear_draws
    n = draws.theta.shape[0]
    assert n == 65536
    a = regression.adjust(model, draws, kernel="uniform", delta=math.inf, path="generic")
    post_mean, post_var = model.y_obs.numpy().reshape(-1) / 1.25, 0.2
    th = a.theta.double().numpy()
    z_mean = (th.mean(0) - post_mean) / math.sqrt(post_var / n)
    z_var = (th.var(0) - post_var) / (post_var * math.sqrt(2.0 / n))
    print("mean: %s standard errors, variance: %s" % (z_mean.round(2), z_var.round(2)))
    assert (np.abs(z_mean) <= 5).all() and (np.abs(z_var) <= 5).all()
    assert np.abs(a.beta - 0.8 * np.eye(2)).max() <= 0.02
    assert (np.abs(a.mean - post_mean) <= 5 * math.sqrt(post_var / n)).all()
    assert np.abs(a.covariance - post_var * np.eye(2)).max() <= 5 * post_var * math.sqrt(2.0 / n)
    assert math.isclose(a.ess, n, rel_tol=1e-12) and a.outside_prior == 0.0 and a.delta == math.inf
    assert math.isclose(float(a.weights.sum()), 1.0, rel_tol=1e-12)


def test_known_answer_epanechnikov(linear_draws):
    model, draws = linear_draws
    a = regression.adjust(model, draws, quantile=0.2, path="generic")
    assert 0.19 * 65536 < int((a.weights > 0).sum()) <= 0.2 * 65536 + 1
    post_mean = model.y_obs.numpy().reshape(-1) / 1.25
    wm = (a.weights[:, None] * a.theta.double()).sum(0).numpy()
    z = (wm - post_mean) / math.sqrt(0.2 / a.ess)
    print("weighted mean: %s standard errors, ess %.0f" % (z.round(2), a.ess))
    assert (np.abs(z) <= 5).all()
    assert np.allclose(wm, a.mean, rtol=0, atol=1e-6)               # the Gram's mean is the adjusted draws' weighted mean


# ---- edges of fit and combine
def small_rows(n=300, seed=3):
    rng = np.random.default_rng(seed)
    theta = rng.standard_normal((n, 2)).astype(np.float32)
    y = (theta @ np.array([[1.0, 0.3, 0.0], [0.2, 1.0, 0.5]]) + 0.3 * rng.standard_normal((n, 3))).astype(np.float32)
    return torch.from_numpy(theta), torch.from_numpy(y), np.array([0.1, -0.2, 0.3])


def test_fit_refuses_constant_column_and_ridge_lets_it_through():
    theta, y, y_obs = small_rows()
    y[:, 1] = 0.75
    g = regression.terms(theta, y, y_obs=y_obs, path="generic")
    with pytest.raises(ValueError, match="condition number"):
        regression.fit(g, 2, 3)
    f = regression.fit(g, 2, 3, ridge=1e-6)
    assert np.isfinite(f.beta).all() and abs(f.beta[1]).max() < 1e-3


def test_fit_refuses_too_few_weighted_rows():
    theta, y, y_obs = small_rows(n=5)
    g = regression.terms(theta, y, y_obs=y_obs, path="generic")
    with pytest.raises(ValueError, match="too few weighted rows"):
        regression.fit(g, 2, 3)
    with pytest.raises(ValueError, match="no row carries weight"):
        regression.fit(np.zeros(R.n_stats(2, 3)), 2, 3)


def test_combine_of_ragged_shards():
    theta, y, y_obs = small_rows(n=2500)
    dis = torch.from_numpy(np.random.default_rng(5).uniform(0.0, 1.2, 2500).astype(np.float32))
    cuts = [(0, 1), (1, 1300), (1300, 2500)]
    shards = [R.weighted_gram(theta[a:b].numpy().T, y[a:b].numpy().T, dis[a:b].numpy(), None, b - a, y_obs, 1.0, R.EPANECHNIKOV)[0]
              for a, b in cuts]
    whole, _ = R.weighted_gram(theta.numpy().T, y.numpy().T, dis.numpy(), None, 2500, y_obs, 1.0, R.EPANECHNIKOV)
    w = R.row_weights(dis.numpy(), None, 2500, 1.0, R.EPANECHNIKOV)
    bound = R.addition_bound(R.row_terms(R.design(theta.numpy().T, y.numpy().T, 2500, y_obs), w), w)
    got = regression.combine(shards)
    assert (np.abs(got - whole) <= bound).all()
    assert R.same_bits(got, regression.combine(shards))            # deterministic for a given split
    with pytest.raises(ValueError):
        regression.combine([])


def test_zero_weight_row_with_nan_changes_nothing():
    theta, y, y_obs = small_rows(n=700)
    dis = torch.from_numpy(np.random.default_rng(6).uniform(0.0, 0.9, 700).astype(np.float32))
    clean_ref, _ = R.weighted_gram(theta.numpy().T, y.numpy().T, dis.numpy(), None, 700, y_obs, 1.0, R.EPANECHNIKOV)
    clean = regression.terms(theta, y, dis, y_obs=y_obs, delta=1.0, path="generic")
    theta, dis = theta.clone(), dis.clone()
    theta[17, 0], dis[17] = math.nan, 2.0                           # outside delta: weight 0
    theta[400, 1], dis[400] = math.nan, math.nan                    # a NaN distance: weight 0
    clean_ref2, _ = R.weighted_gram(np.delete(theta.numpy(), [17, 400], 0).T, np.delete(y.numpy(), [17, 400], 0).T,
                                    np.delete(dis.numpy(), [17, 400]), None, 698, y_obs, 1.0, R.EPANECHNIKOV)
    ref, _ = R.weighted_gram(theta.numpy().T, y.numpy().T, dis.numpy(), None, 700, y_obs, 1.0, R.EPANECHNIKOV)
    got = regression.terms(theta, y, dis, y_obs=y_obs, delta=1.0, path="generic")
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    assert np.allclose(ref, clean_ref2, rtol=1e-12) and np.allclose(got, ref, rtol=1e-12)
    assert not np.array_equal(clean, got) and np.isfinite(clean_ref).all()


def test_arguments():
    theta, y, y_obs = small_rows(n=50)
    with pytest.raises(ValueError, match="kernel"):
        regression.terms(theta, y, y_obs=y_obs, kernel="gauss", path="generic")
    with pytest.raises(ValueError, match="delta"):
        regression.terms(theta, y, y_obs=y_obs, delta=0.0, path="generic")
    with pytest.raises(ValueError, match="path"):
        regression.terms(theta, y, y_obs=y_obs, path="eager")
    with pytest.raises(ValueError, match="fused"):
        regression.terms(theta, y, y_obs=y_obs, path="fused")
    with pytest.raises(ValueError, match="beta"):
        regression.apply(theta, y, np.zeros((2, 3)), y_obs=y_obs, path="generic")
    out = regression.apply(theta, y, np.zeros((3, 2)), y_obs=y_obs, path="generic")
    assert torch.equal(out, theta)
    beta = np.random.default_rng(0).standard_normal((3, 2))
    assert R.same_bits(regression.apply(theta, y, beta, y_obs=y_obs, path="generic").numpy().T,
                       R.regression_apply(theta.numpy().T, y.numpy().T, 50, y_obs, beta))


# ---- the committed resource report
def test_resource_report_shows_no_private_segment():
    """profiles/regress_kernel_resources.txt: every gram_kernel<2..16>, the finishing kernel and all 64 apply_kernel<TD, YD> without a
    private segment or a spilled vector register"""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "regress_kernel_resources.txt")).read()
    kernels = re.split(r"^Function Name: ", text.split("# apply_kernel<TD, YD>")[0], flags=re.M)[1:]
    assert sorted(int(re.search(r"gram_kernelILi(\d+)E", k).group(1)) for k in kernels if "gram_kernelI" in k) == list(range(2, 17))
    assert sum("gram_finish_kernel" in k for k in kernels) == 1
    for k in kernels:
        field = lambda name: int(re.search(r"%s: (\d+)" % re.escape(name), k).group(1))          # noqa: E731
        assert field("ScratchSize [bytes/lane]") == 0 and field("VGPRs Spill") == 0 and "Dynamic Stack: False" in k, k.splitlines()[0]
    rows = [line.split() for line in text.splitlines() if line.startswith("apply_kernel ")]
    assert sorted((int(r[1]), int(r[2])) for r in rows) == [(t, y) for t in range(1, 9) for y in range(1, 9)]
    assert all(r[5:8] == ["0", "0", "0"] for r in rows)              # private segment, spilled scalars, spilled vectors
