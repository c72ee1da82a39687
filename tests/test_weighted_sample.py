"""One law check of glabcmcmc_amd.weighted on the GPU: the credible intervals of an ABC-SMC population against those of a plain
rejection sample of the same target."""
import math
from fractions import Fraction

import numpy as np
import pytest

from glabcmcmc_amd import rejection, smc, weighted
from glabcmcmc_amd.examples.Mixture import Mixture_set

pytestmark = pytest.mark.gpu

SEED = 0x5EEDC0FFEE123457
Z = 5.0


def test_interval_of_a_population_is_the_rejection_samples(hip):
    """``smc.sample(Mixture_set(0.05), 4096, kernel="model")`` and ``rejection.sample(kernel="model")`` draw from the same ABC
    posterior, the first with weights.  For each end p of the equal-tailed intervals of probability 0.5, 0.9 and 0.95 the weighted
    quantile t = q_smc(p) is compared with the rejection sample on the probability scale, which needs no density estimate.

    Margin.  With F the posterior's distribution function, F(q_smc(p)) - p has standard deviation sqrt(p (1 - p) / ESS), ESS the
    population's Kish effective sample size (an inverted empirical distribution function of ESS effective draws), and the rejection
    sample's empirical F_rej(t) at a fixed t has standard deviation sqrt(F (1 - F) / n_rej), n_rej the accepted draws; the two
    samples are independent, so
        F_rej(q_smc(p)) - p      has standard deviation      s = sqrt(p (1 - p) (1 / ESS + 1 / n_rej))
    and the allowed difference is Z = 5 of them plus the two empirical functions' own steps, the largest normalised weight of the
    population and 1 / n_rej.  ESS and n_rej are read off the two samples in the test.  Equivalently: q_smc(p) lies between the
    rejection sample's quantiles at p - margin and p + margin.  A wrong weighted quantile -- weights ignored, a rank off by the
    share of one mode -- misses by tenths on this bimodal posterior; the margins are a few hundredths.

    Observed: ESS 3210, n_rej 2382, |F_rej(q_smc(p)) - p| / s at most 1.77 over the 12 comparisons, margins 0.024 to
    0.062."""
    model = Mixture_set(0.05)
    pop = smc.sample(model, 4096, kernel="model", seed=SEED)
    rej = rejection.sample(model, 1 << 21, kernel="model", seed=SEED + 1)
    m, scale = weighted.quantize(pop.weights)
    total, sum_sq = int(m.sum()), sum(int(v) ** 2 for v in m.tolist())
    ess = total * total / sum_sq
    summary = weighted.summary(pop)
    assert summary["M"] == total and summary["scale"] == scale and math.isclose(summary["ess"], ess, rel_tol=1e-12)
    assert math.isclose(ess, float(pop.ess), rel_tol=1e-3)           # float32 weights against the sampler's float64 ones
    n_rej = rej.theta.shape[0]
    assert n_rej > 1000 and ess > 1000
    theta = np.sort(rej.theta.cpu().numpy().astype(np.float64), axis=0)
    step = float(pop.weights.max()) + 1.0 / n_rej
    worst = 0.0
    for prob in (0.5, 0.9, 0.95):
        lower, upper = weighted.interval(pop, prob)
        assert lower.shape == upper.shape == (2,) and (lower < upper).all()
        for p, ends in (((1.0 - prob) / 2.0, lower), ((1.0 + prob) / 2.0, upper)):
            s = math.sqrt(p * (1.0 - p) * (1.0 / ess + 1.0 / n_rej))
            for j in range(2):
                f_rej = np.searchsorted(theta[:, j], ends[j], side="right") / n_rej
                print("prob %.2f p %.3f coordinate %d: q_smc %.4f, F_rej %.4f, (F_rej - p) / s %.2f, margin %.4f"
                      % (prob, p, j, ends[j], f_rej, (f_rej - p) / s, Z * s + step))
                worst = max(worst, abs(f_rej - p) / s)
                assert abs(f_rej - p) <= Z * s + step
    print("ess %.0f of 4096, %d accepted rejection draws, worst |F_rej - p| / s %.2f" % (ess, n_rej, worst))
    # the unit-weight path on the rejection sample is numpy's inverted empirical distribution function
    lower, upper = weighted.interval(rej, 0.9)
    rank = lambda p: max(math.ceil(Fraction(p) * n_rej), 1) - 1      # noqa: E731
    assert np.array_equal(lower, theta[rank((1.0 - 0.9) / 2.0)]) and np.array_equal(upper, theta[rank((1.0 + 0.9) / 2.0)])
