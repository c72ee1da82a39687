"""The full-covariance perturbation kernel of ABC-SMC on the CPU: the refusals of glabc_smc_draws_full as csrc/glabc_check.h answers
them under g++, the compiler's resource report of its kernels, the restatement (tests/smc_full_ref.py) against plain float64
arithmetic, the ValueErrors and RuntimeErrors of ``smc.sample(perturbation="full")``, and the law and the cost of the generic path
on CPU tensors with the callback twin of the correlated linear Model (glabcmcmc_amd/examples/Correlated_smc.py).

Law check.  The particles of the last generation are independent given the previous one, so the standard error of a
self-normalised estimate of E f is sqrt(sum w_i^2 (f_i - mean)^2); the weighted mean and every entry of the weighted covariance are
held to 5 of them against the closed-form Gaussian posterior.  Cost: under bandwidth="beaumont" the full kernel's run simulates at
most half of what the diagonal kernel's run simulates (a NumPy restatement of both kernels gave 3.6 times fewer in three seeds).
"""
import os
import re

import numpy as np
import pytest
import torch

import smc_full_ref as F
import smc_ref as S
from glabcmcmc_amd import _capi, smc
from glabcmcmc_amd.examples import Correlated_smc
from glabcmcmc_amd.examples.Mixture import Mixture_set
from test_arg_checks import check_table

OK, NULL, DIM, KIND, ARG = 0, -1, -2, -3, -4
SEED = 20261021
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------- the refusals (csrc/glabc_check.h)
def test_check_smc_draws_full(tmp_path_factory):
    """check_smc_draws' refusals in their order, the factor's two between the population's dimension and the range of draws"""
    prelude = ("static const int64_t IDS[4] = {3, 1, 3, 1ll << 40}; static uint8_t ACC[4]; static int64_t CUM[4] = {1, 2, 3, 4}; "
               "static float CH[36]; for (int j = 0; j < 36; ++j) CH[j] = 0.25f; "
               "glabc_kde k; std::memset(&k, 0, sizeof k); k.dim = 3; k.n_samples = 4; k.x = b.f; k.log_w = b.f; k.cum_q = CUM; "
               "for (int j = 0; j < 8; ++j) k.bandwidth[j] = 0.5f; ")
    call = "check_smc_draws_full(&b.m, %s, %s, 0, nullptr, %s, 65, b.f, b.f, b.f, b.f, ACC)"

    def row(want, spoil="", k="&k", chol="CH", n="65"):
        return (prelude + spoil, call % (k, chol, n), want)
    check_table(tmp_path_factory, "smc_draws_full", [
        row(OK), row(OK, "make_gk(b); k.dim = 4; "), row(OK, "CH[1] = -3.0f; CH[3] = 0.0f; CH[4] = -0.0f; "),          # off the diagonal: any finite value
        row(OK, "CH[6] = NaN; CH[7] = -1.0f; "),                                                      # past dim (dim + 1) / 2: not read
        row(OK, "b.m.theta_dim = b.m.y_dim = b.m.prior.dim = k.dim = 8; "), row(OK, "b.m.theta_dim = b.m.y_dim = b.m.prior.dim = k.dim = 1; CH[1] = NaN; "),
        row(NULL, chol="nullptr"), row(NULL, k="nullptr", chol="nullptr"),
        row(ARG, "CH[0] = 0.0f; "), row(ARG, "CH[2] = -0.25f; "), row(ARG, "CH[5] = NaN; "), row(ARG, "CH[5] = INFINITY; "),
        row(ARG, "CH[1] = NaN; "), row(ARG, "CH[4] = -INFINITY; "), row(ARG, "b.m.theta_dim = b.m.y_dim = b.m.prior.dim = k.dim = 8; CH[35] = 0.0f; "),
        # the Model and the population come first ...
        row(DIM, "b.m.theta_dim = 0; ", chol="nullptr"), row(KIND, "b.m.sim_kind = GLABC_SIM_USER; CH[0] = 0.0f; "),
        row(ARG, "k.bandwidth[0] = 0.0f; ", chol="nullptr"), row(NULL, "k.cum_q = nullptr; CH[0] = 0.0f; "), row(DIM, "k.dim = 2; ", chol="nullptr"),
        # ... and the range of draws last
        row(NULL, chol="nullptr", n="-1"), row(ARG, "CH[0] = -1.0f; ", n="-1"), row(ARG, n="-1"),
    ])
    check_table(tmp_path_factory, "chol", [
        ("static float CH[3] = {1.0f, -2.0f, 1e-30f}; ", "check_chol(CH, 2)", OK), ("", "check_chol(nullptr, 1)", NULL),
        ("static float CH[3] = {1.0f, 0.0f, 0.0f}; ", "check_chol(CH, 2)", ARG), ("static float CH[3] = {1.0f, 0.0f, 0.0f}; ", "check_chol(CH, 1)", OK),
    ])


def test_entry_points_are_bound_and_exported():
    names = ("glabc_kde_sample_full", "glabc_smc_draws_full", "glabc_rtc_smc_draws_full")
    assert set(names) <= set(_capi.ENTRY_POINTS) and _capi.VERSION == 301 and _capi.STREAM_LAYOUT == 2
    assert [len(_capi.ENTRY_POINTS[n][1]) for n in names] == [7, 14, 15]
    header = open(os.path.join(ROOT, "include", "glabc.h")).read()
    assert "int glabc_kde_sample_full(const glabc_kde* kde, const float* chol, int64_t n, uint64_t seed, int64_t row0" in header
    assert "int glabc_smc_draws_full(const glabc_model* model, const glabc_kde* population, const float* chol, uint64_t seed" in header
    assert "int glabc_rtc_smc_draws_full(const glabc_rtc_program* program, const glabc_model* model, const glabc_kde* population, const float* chol" in header
    lib = _capi.lib()
    assert lib.glabc_smc_draws_full(None, None, None, 0, 0, None, 0, 0, None, None, None, None, None, None) == NULL
    assert lib.glabc_rtc_smc_draws_full(None, None, None, None, 0, 0, None, 0, 0, None, None, None, None, None, None) == NULL
    assert lib.glabc_kde_sample_full(None, None, 0, 0, 0, None, None) == NULL
    m, k = Mixture_set(0.05).descriptor(), _capi.Kde()
    assert lib.glabc_smc_draws_full(m, k, None, 0, 0, None, 0, 0, 8, None, None, None, None, None) == DIM                 # an empty population


def test_resource_report_shows_no_private_segment():
    """profiles/smc_full_kernel_resources.txt: nine instantiations of smc_draws_kernel<D, YD, true>, none with a private segment or a spill"""
    text = open(os.path.join(ROOT, "profiles", "smc_full_kernel_resources.txt")).read()
    kernels = re.split(r"^Function Name: ", text, flags=re.M)[1:]
    assert len(kernels) == 9
    shapes = sorted(tuple(int(x) for x in re.search(r"smc_draws_kernelILi(\d)ELi(\d)ELb1E", k).groups()) for k in kernels)
    assert shapes == sorted([(d, d) for d in range(1, 9)] + [(4, 8)])
    for k in kernels:
        field = lambda name: int(re.search(r"%s: (\d+)" % re.escape(name), k).group(1))          # noqa: E731
        assert field("ScratchSize [bytes/lane]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0
        assert field("Occupancy [waves/SIMD]") >= 8 and field("LDS Size [bytes/block]") == 0


# ---------------------------------------------------------------------------------- the restatement
def population(d, n=60, seed=3, offset=0.0):
    rng = np.random.default_rng(seed)
    X = (offset + rng.standard_normal((n, d))).astype(np.float32)
    w = rng.random(n).astype(np.float32)
    w[::7] = 0.0
    scales = 0.5 + rng.random(d)
    return S.HostPopulation(X, w, bw=scales.astype(np.float32)), F.dense_factor(scales, seed=seed)


@pytest.mark.parametrize("d", [1, 2, 5, 8])
def test_restated_theta_is_x_plus_L_z_to_float32_rounding(d):
    pop, L = population(d)
    ids = np.concatenate([np.arange(300), [2 ** 32 - 1, 2 ** 40 + 3]])
    j, nrm = F.ancestors_and_normals(pop, SEED, ids)
    assert (pop.weights[j] > 0).all() and np.unique(j).size > 20 and abs(nrm.mean()) < 0.2 and abs(nrm.std() - 1.0) < 0.1
    theta = F.theta_rows(pop, L, SEED, ids)
    exact = pop.X[j].astype(np.float64) + nrm.astype(np.float64) @ L.astype(np.float64).T
    # d products and d - 1 sums of magnitude <= sum_e |nrm_e L_de|, one more sum with x: (d + 1) roundings of 2^-24 relative each
    bound = (d + 1) * 2.0 ** -24 * (np.abs(pop.X[j]) + np.abs(nrm).astype(np.float64) @ np.abs(L).astype(np.float64).T)
    assert (np.abs(theta - exact) <= bound).all()
    # a diagonal factor gives oracle_kde_sample's rows under bandwidth = diag(L), bit for bit
    diag = np.diag(pop.bandwidth).astype(np.float32)
    assert np.array_equal(F.theta_rows(pop, diag, SEED, ids).view(np.uint32), S.kde_rows(pop, SEED, ids).view(np.uint32))
    # a draw depends on (population, L, seed, id) alone
    some = np.array([299, 0, 77, 77, 2 ** 40 + 3])
    assert np.array_equal(F.theta_rows(pop, L, SEED, some), theta[[299, 0, 77, 77, 301]])
    assert not np.array_equal(F.theta_rows(pop, L, SEED + 1, some), theta[[299, 0, 77, 77, 301]])


def test_restated_draw_follows_smc_ref_behind_theta():
    model = Mixture_set(0.05).descriptor()
    pop, _ = population(2)
    ids = np.arange(40, 140)
    diag = np.diag(pop.bandwidth).astype(np.float32)
    for a, b in zip(F.restate(model, pop, diag, SEED, ids), S.restate(model, pop, SEED, ids)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("d", [1, 2, 4, 8])
def test_restated_density_against_the_multivariate_normal_formula(d):
    pop, L = population(d, n=40, offset=3.0)
    rng = np.random.default_rng(d)
    theta = 3.0 + 1.5 * rng.standard_normal((25, d))
    w = pop.weights.astype(np.float64) / pop.weights.astype(np.float64).sum()
    cov = L.astype(np.float64) @ L.astype(np.float64).T
    inv, logdet = np.linalg.inv(cov), np.linalg.slogdet(cov)[1]
    want = np.empty(25)
    for i in range(25):
        diff = theta[i] - pop.X.astype(np.float64)
        dens = np.exp(-0.5 * np.einsum("sd,de,se->s", diff, inv, diff) - 0.5 * logdet - 0.5 * d * np.log(2 * np.pi))
        want[i] = np.log((w * dens).sum())
    assert np.allclose(F.log_q(theta, pop.X, pop.weights, L), want, rtol=0, atol=1e-10)
    # ... and the generic path's torch density is the same function
    mix = smc._FullMixture(torch.from_numpy(pop.X), torch.from_numpy(w), L)
    assert np.allclose(mix.log_prob(torch.from_numpy(theta)).numpy(), want, rtol=0, atol=1e-9)


def test_the_closed_form_posterior_of_the_correlated_model():
    mean, cov = F.correlated_posterior()
    m2, c2 = Correlated_smc.analytic()
    assert np.allclose(mean, m2) and np.allclose(cov, c2)
    assert abs(cov[0, 1] / np.sqrt(cov[0, 0] * cov[1, 1]) + 0.980) < 5e-4 and np.allclose(mean, [0.5, 0.5], atol=1e-3)


# ---------------------------------------------------------------------------------- the host layer
def test_full_factor():
    rng = np.random.default_rng(0)
    x = torch.from_numpy((rng.standard_normal((500, 3)) @ np.array([[1.0, 0.9, 0.0], [0.0, 0.3, 0.5], [0.0, 0.0, 0.2]])).astype(np.float32))
    w = torch.from_numpy(rng.random(500))
    w = w / w.sum()
    L = smc.full_factor(x, w, "beaumont")
    assert L.dtype == np.float32 and L.shape == (3, 3) and not np.triu(L, 1).any() and (np.diagonal(L) > 0).all()
    xd, wd = x.double().numpy(), w.numpy()
    mean = wd @ xd
    cov = (wd[:, None] * (xd - mean)).T @ (xd - mean) / (1.0 - (wd * wd).sum())
    assert np.allclose(L.astype(np.float64) @ L.astype(np.float64).T, 2.0 * cov, rtol=1e-5, atol=1e-7)
    # diag(L L^T) is the diagonal rule's bandwidth^2: rule factor times the unbiased weighted std
    assert np.allclose(smc._marginal_scales(L), np.sqrt(2.0 * np.diagonal(cov)), rtol=1e-6)
    silverman = smc.full_factor(x, w, "silverman")
    assert np.allclose(silverman, L * (smc.rule_factor("silverman", 500, 3) / np.sqrt(2.0)), rtol=1e-6)
    fixed = np.array([[2.0, 0.6], [0.6, 1.0]])
    assert np.allclose(smc.full_factor(x[:, :2], w, fixed), np.linalg.cholesky(fixed).astype(np.float32))
    packed = smc.pack_cholesky(L, 3)
    assert list(packed) == [L[0, 0], L[1, 0], L[1, 1], L[2, 0], L[2, 1], L[2, 2]] and np.array_equal(F.pack(L), np.float32(list(packed)))
    for bad, dim in ((np.eye(2), 3), (np.array([[1.0, 0.5], [0.0, 1.0]]), 2), (np.diag([1.0, 0.0]), 2), (np.diag([1.0, np.nan]), 2),
                     (np.diag([1.0, -1.0]), 2), ("L", 2), (np.ones(3), 2)):          # shape, upper triangle, diagonal, not a matrix
        with pytest.raises(ValueError, match="cholesky"):
            smc.pack_cholesky(bad, dim)


def test_argument_errors():
    model, gen = Correlated_smc.Callback(), dict(path="generic", prior=Correlated_smc.prior(), perturbation="full")
    T = lambda **kw: smc.sample(model, 64, **dict(gen, **kw))          # noqa: E731
    with pytest.raises(ValueError, match='perturbation is "diagonal" or "full"'):
        T(perturbation="local")
    with pytest.raises(ValueError, match='perturbation is "diagonal" or "full"'):
        T(perturbation=None)
    for bad in (0.3, [0.3, 0.2], torch.tensor([0.3, 0.2]), "sheather", np.eye(3), np.array([[1.0, 2.0], [2.0, 1.0]]),          # a float, vectors, ..., not SPD
                np.array([[1.0, 0.5], [0.2, 1.0]]), np.array([[1.0, np.nan], [np.nan, 1.0]]), np.zeros((2, 2)), None):
        with pytest.raises(ValueError, match='with perturbation="full", bandwidth is'):
            T(bandwidth=bad)
    # the same values stay what they were under the diagonal kernel
    p = smc.sample(model, 64, kernel="hard", epsilon=2.0, path="generic", prior=Correlated_smc.prior(), bandwidth=[0.3, 0.2])
    assert p.generations[-1]["bandwidth"] == [float(np.float32(0.3)), float(np.float32(0.2))] and "cholesky" not in p.generations[-1]


def test_a_degenerate_population_is_refused():
    x = torch.zeros(64, 2)
    x[:, 0] = torch.arange(64.0)                                           # a constant coordinate
    w = torch.full((64,), 1.0 / 64, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="the population is degenerate.*smallest eigenvalue"):
        smc.full_factor(x, w, "silverman")
    one = torch.ones(64, 2)                                                # one distinct particle
    with pytest.raises(RuntimeError, match="the population is degenerate"):
        smc.full_factor(one, w, "beaumont")
    with pytest.raises(RuntimeError, match="the population is degenerate"):
        smc.full_factor(torch.full((64, 2), float("nan")), w, "beaumont")

    class Flat(Correlated_smc.Callback):                                   # every simulation lands on the data: theta_2 never moves
        def generate_samples(self, theta, num_samples=1):
            return self.y_obs.expand(theta.reshape(-1, 2).shape[0], 2).clone()

    class Line:
        def forward(self, n):
            return torch.stack([torch.randn(n), torch.ones(n)], dim=1), torch.zeros(n)

        def log_prob(self, theta):
            return torch.zeros(theta.shape[0])
    with pytest.raises(RuntimeError, match="the population is degenerate"):
        smc.sample(Flat(), 64, kernel="model", path="generic", prior=Line(), perturbation="full")


def test_diagonal_is_the_call_without_the_argument():
    model, kw = Correlated_smc.Callback(), dict(kernel="hard", epsilon=0.5, path="generic", prior=Correlated_smc.prior(), bandwidth="beaumont")
    torch.manual_seed(SEED)
    a = smc.sample(model, 256, **kw)
    torch.manual_seed(SEED)
    b = smc.sample(model, 256, perturbation="diagonal", **kw)
    assert a.generations == b.generations and all("cholesky" not in g for g in a.generations)
    for x, y in ((a.theta, b.theta), (a.y, b.y), (a.distance, b.distance), (a.weights, b.weights)):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------- the law and the cost, generic path
def test_generic_full_kernel_samples_the_correlated_posterior_in_half_the_simulations():
    N = 2000
    model, kw = Correlated_smc.Callback(), dict(kernel="model", bandwidth="beaumont", path="generic", prior=Correlated_smc.prior())
    torch.manual_seed(SEED)
    full = smc.sample(model, N, perturbation="full", **kw)
    torch.manual_seed(SEED)
    diag = smc.sample(model, N, **kw)
    mean, cov = F.correlated_posterior()
    for name, p in (("full", full), ("diagonal", diag)):
        assert p.theta.shape == (N, 2) and not p.theta.is_cuda and abs(float(p.weights.sum()) - 1.0) < 1e-12 and p.epsilon == 0.05
        m, c, se_m, se_c = F.weighted_moments(p.theta.numpy(), p.weights.numpy())
        sims = sum(g["n_draws"] for g in p.generations)
        print("%s: %d simulations, %d generations, ess %.0f; mean %r (%r SE), covariance %r (%r SE)"
              % (name, sims, len(p.generations), p.ess, m, (m - mean) / se_m, c.tolist(), ((c - cov) / se_c).tolist()))
        assert (np.abs(m - mean) <= 5.0 * se_m).all() and (np.abs(c - cov) <= 5.0 * se_c).all()
    for g in full.generations[1:]:
        L = np.float32(g["cholesky"])
        assert L.shape == (2, 2) and L[0, 1] == 0 and np.allclose(g["bandwidth"], np.sqrt((np.float64(L) ** 2).sum(axis=1)))
        assert L[1, 0] < 0                                                 # the population is anticorrelated from generation 0 on
    assert full.generations[0]["bandwidth"] is None and "cholesky" not in full.generations[0]
    sims = {k: sum(g["n_draws"] for g in p.generations) for k, p in (("full", full), ("diagonal", diag))}
    assert 2 * sims["full"] <= sims["diagonal"], sims
    assert full.ess > N / 4
