"""glabcmcmc_amd.rejection and glabcmcmc_amd.smc on a CompiledModel, through the run-time compiled draw kernels (glabc_rtc_abc_draws /
glabc_rtc_smc_draws), on the GPU.

A CompiledModel that restates Mixture_set(0.05) and Mixture_set itself give identical results on the same seed in every public
function (the sweep, the selection, the first-N-by-id rule and the regeneration are one code for both entry points); smc.sample on a
CompiledModel does not depend on how the sweep is cut; on NONLINEAR the weighted particles of ABC-SMC and the draws of
rejection.sample(kernel="model") have the same means of theta and theta^2 (5 standard errors of the difference, the weighted side's
from its ESS); and a draws program whose self-check disagrees is never handed out.  Two programs are compiled, once each.
"""
import warnings

import numpy as np
import pytest
import torch

from glabcmcmc_amd import rejection, smc
from glabcmcmc_amd.compiled import CompiledModel, SimulatorSelfCheckError
from glabcmcmc_amd.examples.Mixture import Mixture_set
from helpers import make_dist
from test_rtc import NONLINEAR, mixture_source

pytestmark = pytest.mark.gpu

SEED = 0x123456789ABCDEF1


@pytest.fixture(scope="module")
def pair():
    """Mixture_set(0.05) and its restatement as a CompiledModel: the same prior object, y_obs, epsilon and float32 noise scale"""
    builtin = Mixture_set(0.05)
    d = builtin.descriptor()
    compiled = CompiledModel(2, 2, mixture_source([d.noise.p2[0], d.noise.p2[1]]), builtin._prior(), [d.y_obs[0], d.y_obs[1]], 0.05)
    return builtin, compiled


@pytest.fixture(scope="module")
def nonlinear():
    return CompiledModel(3, 2, NONLINEAR, make_dist(("gauss", [0.0, 0.5, 0.0], [1.5, 1.0, 2.0])), [0.9, 0.6], 0.15, noise_dim=4)


def assert_same_rejection(a, b):
    assert a.epsilon == b.epsilon and a.n_draws == b.n_draws and a.ids.numel() > 0
    for x, y in ((a.theta, b.theta), (a.y, b.y), (a.distance, b.distance), (a.ids, b.ids)):
        assert x.shape == y.shape and torch.equal(x, y)


def assert_same_population(a, b):
    assert a.generations == b.generations and a.epsilon == b.epsilon and a.ess == b.ess
    for x, y in ((a.theta, b.theta), (a.y, b.y), (a.distance, b.distance), (a.weights, b.weights)):
        assert torch.equal(x, y)


def test_rejection_equals_the_builtin_model(hip, pair):
    builtin, compiled = pair
    assert rejection._path(compiled, "auto", 0.05).program is not None and rejection._path(builtin, "auto", 0.05).program is None
    for kw in (dict(kernel="model"), dict(kernel="model", epsilon=0.3), dict(kernel="hard", n_accept=100), dict(kernel="hard", quantile=0.01),
               dict(kernel="hard", epsilon=0.2)):
        for path in ("auto", "fused"):
            assert_same_rejection(rejection.sample(compiled, 50000, seed=SEED, path=path, **kw), rejection.sample(builtin, 50000, seed=SEED, **kw))
    a, b = rejection.calibrate_epsilon(compiled, 50000, 0.02, seed=SEED), rejection.calibrate_epsilon(builtin, 50000, 0.02, seed=SEED)
    assert a == b and a > 0.0
    for kernel, n_draws in (("hard", None), ("model", 200000)):
        ta, ya = rejection.initial_state(compiled, 64, kernel=kernel, n_draws=n_draws, seed=SEED)
        tb, yb = rejection.initial_state(builtin, 64, kernel=kernel, n_draws=n_draws, seed=SEED)
        assert ta.shape == (64, 2) and torch.equal(ta, tb) and torch.equal(ya, yb)
    ids = torch.tensor([2 ** 40 + 7, 3, 3, 2 ** 32], dtype=torch.int64)
    da, db = rejection.draws(compiled, 4, seed=SEED, ids=ids), rejection.draws(builtin, 4, seed=SEED, ids=ids)
    for x, y in zip(da, db):
        assert torch.equal(x, y)


@pytest.mark.parametrize("kw", [dict(kernel="model"), dict(kernel="hard", epsilon=0.3), dict(kernel="hard", epsilons=[0.6, 0.3, 0.15]),
                                dict(kernel="model", bandwidth="beaumont", quantile=0.3)], ids=["model", "hard", "ladder", "beaumont"])
def test_smc_equals_the_builtin_model(hip, pair, kw):
    builtin, compiled = pair
    a, b = smc.sample(compiled, 512, seed=SEED, **kw), smc.sample(builtin, 512, seed=SEED, **kw)
    assert_same_population(a, b)
    assert len(a.generations) >= 2 and a.theta.is_cuda


def test_smc_draws_equal_the_builtin_model(hip, pair):
    builtin, compiled = pair
    p = smc.sample(builtin, 256, kernel="hard", epsilon=0.5, seed=SEED)
    kde = smc._Rule("silverman", device=p.theta.device).fit(p.theta, p.weights.to(torch.float32))
    for x, y in zip(smc.draws(compiled, kde, 300, seed=SEED, row0=2 ** 32 - 5), smc.draws(builtin, kde, 300, seed=SEED, row0=2 ** 32 - 5)):
        assert torch.equal(x, y)


def test_smc_on_a_compiled_model_does_not_depend_on_the_launch_size(hip, nonlinear, monkeypatch):
    a = smc.sample(nonlinear, 512, kernel="model", seed=SEED)
    monkeypatch.setattr(smc, "MIN_LAUNCH", 1)
    monkeypatch.setattr(rejection, "MAX_LAUNCH", 777)
    b = smc.sample(nonlinear, 512, kernel="model", seed=SEED)
    assert_same_population(a, b)
    assert a.epsilon == 0.15 and abs(float(a.weights.sum()) - 1.0) < 1e-12
    c = smc.sample(nonlinear, 512, kernel="model", seed=SEED + 1)
    assert not torch.equal(a.theta, c.theta)


def test_smc_and_rejection_agree_in_law_on_nonlinear(hip, nonlinear):
    p = smc.sample(nonlinear, 4096, kernel="model", seed=SEED)
    r = rejection.sample(nonlinear, 1 << 19, kernel="model", seed=SEED + 1)
    m = r.ids.numel()
    assert m > 200 and p.ess > 200                                     # enough on both sides for the comparison to mean something
    w = p.weights.double().cpu().numpy()
    for power in (1, 2):
        f, g = p.theta.double().cpu().numpy() ** power, r.theta.double().cpu().numpy() ** power
        mu_w = (w[:, None] * f).sum(axis=0)
        var_w = (w[:, None] * (f - mu_w) ** 2).sum(axis=0)
        se = np.sqrt(var_w / p.ess + g.var(axis=0, ddof=1) / m)
        z = (mu_w - g.mean(axis=0)) / se
        print("theta^%d: SMC %s, rejection %s, z %s (ESS %.0f, %d accepted)" % (power, mu_w, g.mean(axis=0), z, p.ess, m))
        assert (np.abs(z) <= 5.0).all(), (power, mu_w, g.mean(axis=0), se)


def test_a_disagreeing_self_check_hands_no_program_out(hip, monkeypatch):
    cm = CompiledModel(3, 2, NONLINEAR, make_dist(("gauss", [0.0, 0.5, 0.0], [1.5, 1.0, 2.0])), [0.9, 0.6], 0.15, noise_dim=4)
    composed = CompiledModel.composed_draws

    def wrong(self, *args, **kw):
        out = composed(self, *args, **kw)
        out["y"] = out["y"] + 1.0
        return out

    monkeypatch.setattr(CompiledModel, "composed_draws", wrong)
    with pytest.raises(SimulatorSelfCheckError, match="disagrees with the composition"):
        cm.draws_program()
    with pytest.raises(SimulatorSelfCheckError):                            # the verdict sticks
        cm.draws_program()
    assert (CompiledModel.DRAWS,) not in cm._programs and (CompiledModel.DRAWS,) not in cm._checked
    with pytest.raises(SimulatorSelfCheckError):
        rejection.sample(cm, 1000, kernel="hard", n_accept=10, seed=SEED, path="fused")
    with pytest.raises(SimulatorSelfCheckError):
        smc.sample(cm, 64, kernel="hard", epsilon=1.0, seed=SEED, path="fused")
    # "auto" warns and goes generic: as before this path existed, prior= requirement included
    with pytest.warns(RuntimeWarning, match="generic path"):
        with pytest.raises(ValueError, match="prior="):
            rejection.sample(cm, 1000, kernel="hard", n_accept=10, seed=SEED)
    with pytest.warns(RuntimeWarning, match="generic path"):
        r = rejection.sample(cm, 1000, kernel="hard", n_accept=10, seed=SEED, prior=cm.prior)
    assert r.ids.numel() == 10 and r.n_draws == 1000
    monkeypatch.undo()
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)                                     # the verdict is this object's: a fresh one checks and runs fused
        fresh = CompiledModel(3, 2, NONLINEAR, cm.prior, [0.9, 0.6], 0.15, noise_dim=4)
        assert rejection.sample(fresh, 1000, kernel="hard", n_accept=10, seed=SEED).ids.numel() == 10
