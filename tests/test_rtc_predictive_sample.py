"""glabcmcmc_amd.predictive on a CompiledModel, through the run-time compiled predictive kernel (glabc_rtc_predictive_counts /
glabc_rtc_predictive_draws), on the GPU, end to end.

check under "auto" on a GPU history is the fused path; it equals summary(combine(terms(...))) over two chain shards times two row
slices; range=None equals the explicit exact range; simulate in its three layouts holds the draws that check counts; a predictive
program whose self-check disagrees is never handed out -- "auto" warns and runs the generic path, "fused" raises.

Law (derived, not tuned): EDGE1 is y = theta^2 + 0.5 eps.  On a constant history theta = 1, 1024 chains x 64 rows, the N = 65 536
draws are independent y = 1 + 0.5 z.  P(y >= 1) = 1/2, binomial standard error 0.5 / 256; the mass of [0.5, 1.5] is
erf(1 / sqrt 2) = 0.6827, standard error sqrt(0.6827 x 0.3173 / 65 536); both within 5 standard errors.
"""
import math

import numpy as np
import pytest
import torch

from glabcmcmc_amd import diagnostics, predictive
from glabcmcmc_amd.compiled import CompiledModel, SimulatorSelfCheckError
from helpers import make_dist
from test_rtc import NONLINEAR
from test_rtc_draws_shapes import EDGE1

pytestmark = pytest.mark.gpu

SEED = 0x123456789ABCDEF1


def nonlinear_model():
    return CompiledModel(3, 2, NONLINEAR, make_dist(("gauss", [0.0, 0.5, 0.0], [1.5, 1.0, 2.0])), [0.9, 0.6], 0.15, noise_dim=4)


@pytest.fixture(scope="module")
def nonlinear():
    return nonlinear_model()


@pytest.fixture(scope="module")
def rows():
    """a (T, C, D) history on the GPU: 11 rows of 130 chains"""
    g = torch.Generator().manual_seed(5)
    return (torch.tensor([0.0, 0.5, 0.0]) + torch.tensor([1.5, 1.0, 2.0]) * torch.randn(11, 130, 3, generator=g)).cuda()


def assert_same_check(a, b):
    assert a.n == b.n and a.within_epsilon == b.within_epsilon
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_auto_is_the_fused_path_and_the_tables_add_over_shards(hip, nonlinear, rows):
    assert predictive._path(nonlinear, rows, "auto").program is not None
    assert predictive._path(nonlinear, rows.cpu(), "auto") is None
    auto = predictive.check(nonlinear, rows, bins=7, seed=SEED)
    fused = predictive.check(nonlinear, rows, bins=7, seed=SEED, path="fused")
    assert_same_check(auto, fused)
    assert auto.n == 1430 and (auto.y_counts.sum(axis=1) == 1430).all() and auto.distance_counts.sum() == 1430
    assert not auto.y_outside.any() and not auto.distance_outside.any()
    # range=None is the explicit exact range, found in a pass of its own
    lim = np.concatenate([auto.y_edges[:, [0, -1]], auto.distance_edges[None, [0, -1]]])
    assert_same_check(predictive.check(nonlinear, rows, bins=7, range=lim, seed=SEED), auto)
    # shards of chains and slices of rows count the very draws of the whole job
    whole = predictive.terms(nonlinear, rows, bins=7, range=lim, seed=SEED)
    parts = [predictive.terms(nonlinear, rows[r0:r1, c0:c1], bins=7, range=lim, seed=SEED, chain0=c0, n_chains_total=130, row0=r0)
             for r0, r1 in ((0, 4), (4, 11)) for c0, c1 in ((0, 50), (50, 130))]
    both = predictive.combine(parts)
    assert both.n == whole.n == 1430 and np.array_equal(both.counts, whole.counts) and np.array_equal(both.tails, whole.tails)
    assert_same_check(predictive.summary(both), auto)
    # another seed: other draws; the chain-major layout: the same
    assert not np.array_equal(predictive.check(nonlinear, rows, bins=7, range=lim, seed=SEED + 1).tails, auto.tails)
    assert_same_check(predictive.check(nonlinear, rows.permute(0, 2, 1).contiguous(), bins=7, seed=SEED, layout="chain_major"), auto)


def test_simulate_in_every_layout_holds_the_draws_check_counts(hip, nonlinear, rows):
    c = predictive.check(nonlinear, rows, bins=7, seed=SEED)
    y, dis = predictive.simulate(nonlinear, rows, seed=SEED)
    assert y.is_cuda and tuple(y.shape) == (11, 130, 2) and tuple(dis.shape) == (11, 130)
    h = diagnostics.histogram(y, 7)
    assert np.array_equal(h.counts, c.y_counts) and np.array_equal(h.edges, c.y_edges)
    assert np.array_equal(diagnostics.histogram(dis.reshape(11, 130, 1), 7).counts[0], c.distance_counts)
    ycm, dcm = predictive.simulate(nonlinear, rows.permute(0, 2, 1).contiguous(), seed=SEED, layout="chain_major")
    assert tuple(ycm.shape) == (11, 2, 130) and torch.equal(ycm.permute(0, 2, 1), y) and torch.equal(dcm, dis)
    y1, d1 = predictive.simulate(nonlinear, rows[:, 5], seed=SEED, chain0=5, n_chains_total=130)
    assert tuple(y1.shape) == (11, 2) and tuple(d1.shape) == (11,) and torch.equal(y1, y[:, 5]) and torch.equal(d1, dis[:, 5])
    # the distances are the Model's own of the simulated rows
    assert torch.equal(nonlinear.discrepancy(y.reshape(-1, 2)).reshape(11, 130), dis)


def test_a_disagreeing_self_check_hands_no_program_out(hip, rows, monkeypatch):
    cm = nonlinear_model()
    composed = CompiledModel.composed_predictive

    def wrong(self, *args, **kw):
        y, dis = composed(self, *args, **kw)
        return y + 1.0, dis

    monkeypatch.setattr(CompiledModel, "composed_predictive", wrong)
    with pytest.raises(SimulatorSelfCheckError, match="disagrees with the composition"):
        cm.predictive_program()
    with pytest.raises(SimulatorSelfCheckError):                            # the verdict sticks
        cm.predictive_program()
    assert (CompiledModel.PREDICTIVE,) not in cm._programs and (CompiledModel.PREDICTIVE,) not in cm._checked
    with pytest.raises(SimulatorSelfCheckError):
        predictive.check(cm, rows, bins=7, seed=SEED, path="fused")
    with pytest.raises(SimulatorSelfCheckError):
        predictive.simulate(cm, rows, seed=SEED)
    with pytest.warns(RuntimeWarning, match="generic path"):
        c = predictive.check(cm, rows, bins=7, seed=SEED)
    assert c.n == 1430 and c.distance_counts is not None and (c.y_counts.sum(axis=1) == 1430).all()


def test_law_of_the_predictive_draws_of_a_user_simulator(hip):
    Model = CompiledModel(1, 1, EDGE1, make_dist(("gauss", [0.0], [1.0])), [1.0], 0.3, noise_dim=1)
    n = 65536
    history = torch.ones(64, 1024, 1, device="cuda")
    c = predictive.check(Model, history, bins=1, range=[(0.5, 1.5), (0.0, 10.0)], thresholds=[1.0, 0.3], seed=2026)
    assert c.n == n and (c.tails.sum(axis=1) == n).all() and not c.tails[:, 3].any()
    mass = c.y_counts[0, 0] / n
    p = math.erf(1.0 / math.sqrt(2.0))
    print("p_upper %r (0.5 +- %.4f), mass %r (%.4f +- %.4f)" % (c.p_upper.tolist(), 0.5 / 256, mass, p, math.sqrt(p * (1 - p) / n)))
    assert abs(c.p_upper[0] - 0.5) <= 5 * 0.5 / 256
    assert abs(mass - p) <= 5 * math.sqrt(p * (1.0 - p) / n)
