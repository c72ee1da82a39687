"""glabcmcmc_amd.coverage on the GPU: does the diagnostic separate a sound tolerance from a loose one on the project's own example?

Mixture_set (y = |theta| + N(0, 0.05 I), prior N(0, I), D = 2), n = 2^17 table draws, 512 prior-predictive tests, fixed seeds, 10 bins.
The rank histogram pooled over the two coordinates is held to the 99.9 % point of chi^2(9), 27.88: below it at epsilon = 0.1 and at
epsilon = +inf (the posterior is then the prior, which is calibrated too), above it at epsilon = 1.0, where the over-wide posterior
piles the ranks up on both sides of the middle and the 90 % interval covers more often than at 0.1.

The seed was chosen on the CPU first: the restatement (tests/coverage_ref.py) at these very sizes, n = 2^17 and 512 tests, gives under
SEED  chi2 = 3.27 (hard, 0.1), 16.55 (hard, +inf), 135.24 (hard, 1.0), 3.58 (model, 0.1), 42.07 (model, 1.0) and coverage(0.9) = 0.889
at 0.1 against 0.970 at 1.0.  The fused path computes the same integers (tests/test_coverage_shapes.py), so these are the figures
this test sees.

quantile = 0.01: every test keeps its floor(0.01 (n - 1)) + 1 nearest draws and the ties of the last, and the tolerances are
torch.sort's order statistic of the composed distances (glabc_abc_draws, then glabc_model_discrepancy with y_obs swapped).
"""
import copy
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from glabcmcmc_amd import coverage, rejection
from glabcmcmc_amd.examples.Mixture import Mixture_set
from helpers import bits, host

pytestmark = pytest.mark.gpu

SEED = 20261021
N, R = 1 << 17, 512
BOUND = 27.88                              # the 99.9 % point of chi^2(9)


@functools.lru_cache(maxsize=None)
def checked(kernel, eps):
    return coverage.check(Mixture_set(0.05), R, N, kernel=kernel, epsilon=eps, seed=SEED)


def test_rank_histogram_separates_a_sound_tolerance_from_a_loose_one(hip):
    tight, prior, loose = checked("hard", 0.1), checked("hard", math.inf), checked("hard", 1.0)
    for name, c in (("0.1", tight), ("inf", prior), ("1.0", loose)):
        print("hard %s: chi2 %.2f, coverage %r, empty %d, median kept %.0f" % (name, c.chi2(10).value, c.coverage().pooled.tolist(), c.n_empty,
                                                                              float(c.ess.nanmedian())))
    assert tight.chi2(10).dof == 9 and tight.n_empty == prior.n_empty == loose.n_empty == 0
    assert tight.chi2(10).value < BOUND and prior.chi2(10).value < BOUND
    assert loose.chi2(10).value > BOUND
    assert float(loose.coverage(0.9).pooled[0]) > float(tight.coverage(0.9).pooled[0])
    assert prior.mass.tolist() == [N] * R and int(tight.rank_histogram(10).sum()) == 2 * R
    assert torch.equal(tight.mass2, tight.mass) and (tight.below <= tight.mass[:, None]).all()


def test_model_kernel_agrees_with_the_hard_kernel(hip):
    for eps in (0.1, 1.0):
        hard, model = checked("hard", eps), checked("model", eps)
        print("epsilon %g: chi2 hard %.2f, model %.2f, median ess %.1f" % (eps, hard.chi2(10).value, model.chi2(10).value, float(model.ess.nanmedian())))
        assert (model.ess[~model.empty] <= N).all() and model.unit == 65536 and (model.mass <= 65536 * N).all()
        assert (model.chi2(10).value < BOUND) == (hard.chi2(10).value < BOUND)
    assert checked("model", 0.1).chi2(10).value < BOUND < checked("model", 1.0).chi2(10).value


def test_quantile_keeps_the_rank_and_its_ties(hip):
    q, rank = 0.01, int(math.floor(0.01 * (N - 1)))
    c = coverage.check(Mixture_set(0.05), R, N, kernel="hard", quantile=q, seed=SEED)
    assert (c.widths > 0).all() and torch.isfinite(c.widths).all() and c.n_empty == 0
    # one float below each tolerance fewer than rank + 1 draws are kept: the tolerance IS the distance of that rank, and what is kept
    # beyond rank + 1 are its ties
    under = coverage.check(Mixture_set(0.05), R, N, kernel="hard", epsilon=torch.nextafter(c.widths, torch.zeros(())), seed=SEED)
    ties = c.mass - under.mass - 1
    assert (under.mass <= rank).all() and (c.mass >= rank + 1).all() and (ties >= 0).all()
    assert (c.mass - (rank + 1) <= ties).all()
    print("rank %d: kept %d .. %d, tests with ties %d" % (rank, int(c.mass.min()), int(c.mass.max()), int((ties > 0).sum())))
    assert int(c.mass.min()) == rank + 1                                # ties are rare: most tests keep exactly rank + 1
    assert c.chi2(10).value < BOUND                                     # a 1 % tolerance is sound here
    # the same tolerances in several launches per sweep
    old, rejection.MAX_LAUNCH = rejection.MAX_LAUNCH, 50000
    try:
        c2 = coverage.check(Mixture_set(0.05), R, N, kernel="hard", quantile=q, seed=SEED)
    finally:
        rejection.MAX_LAUNCH = old
    assert torch.equal(c2.widths, c.widths) and torch.equal(c2.mass, c.mass) and torch.equal(c2.below, c.below)


def test_quantile_tolerances_equal_torch_sort_of_the_composed_distances(hip):
    n, nt = 1 << 14, 64
    model = Mixture_set(0.05)
    desc = model.descriptor()
    tests = rejection.draws(model, nt, seed=SEED ^ coverage.COVERAGE_TEST_KEY, want=("theta", "y"))
    y = rejection.draws(model, n, seed=SEED, want=("y",)).y.contiguous()
    ys, dis = host(tests.y), torch.empty(n, device="cuda")
    for q in (0.0, 0.01, 0.5, 1.0):
        rank = int(math.floor(q * (n - 1)))
        c = coverage.check(model, nt, n, kernel="hard", quantile=q, seed=SEED)
        want = np.empty(nt, np.float32)
        for r in range(nt):
            swapped = copy.copy(desc)
            swapped.y_obs = type(desc.y_obs)(*([float(v) for v in ys[r]] + [0.0] * 6))
            assert hip.glabc_model_discrepancy(C.byref(swapped), y.data_ptr(), n, dis.data_ptr(), None) == 0
            want[r] = float(torch.sort(dis).values[rank])
        assert np.array_equal(bits(c.widths.numpy()), bits(want)), q
        assert (c.mass >= rank + 1).all() and int(c.mass.min()) == rank + 1
    # the local test: pseudo-observations near y_obs, from another seed than the table's
    near = rejection.sample(model, 1 << 16, kernel="hard", n_accept=nt, seed=SEED + 1)
    local = coverage.check(model, nt, n, kernel="hard", quantile=0.01, tests=near, seed=SEED)
    assert local.mass.shape == (nt,) and (local.mass >= int(0.01 * (n - 1)) + 1).all()
