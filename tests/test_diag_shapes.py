"""glabc_autocov (csrc/glabc_diag.hip) at every shape at which its kernels take another path, bit for bit against the NumPy
restatement of its specification (tests/diag_ref.py), and glabcmcmc_amd/diagnostics.py against the restatement's formulas.

The kernels hold 20 lags per work-item, unroll time by 20 rows and put 4 lag blocks in a workgroup of 64 chains, so the grid has
rows and lags on both sides of 20, 40 and 80 next to the powers of two, one row, a ragged last workgroup (63, 65, 321 chains)
and padding columns that hold NaN.  cases() is not the full cross product: test_grid_covers_every_pair checks that every value
of an axis meets at least two values of every other axis.

Tolerances.  glabc_autocov: none, equal bits (NaN matching NaN).  rhat / ess / tau / mcse / sd / mean: rtol 1e-9 -- the
per-chain numbers are bit-equal, only the sums over chains differ in order, at most M 2^-53 relative each, about 2e-11 after the
pair sums; `truncated` must be equal, and before anything runs on the GPU the restatement's examined |P_j| are asserted to
exceed 1e-6, so that the Geyer cut cannot flip on a rounding difference.
"""
import functools

import numpy as np
import pytest
import torch

import diag_ref as R
from helpers import assert_untouched, assert_written, bits64, canary_f64, dev, host

ERR_NULL, ERR_DIM, ERR_ARG = -1, -2, -4          # glabc_status, include/glabc.h

DIMS = (1, 2, 3, 8)
CHAINS = (1, 63, 64, 65, 321)
PADS = (0, 17)
ROWS = (1, 2, 19, 20, 21, 31, 32, 33, 40, 41, 64, 65, 97)
LAGS = (0, 1, 19, 20, 21, 31, 32, 33, 39, 40, 63, 64, 79, 80)          # and n_rows - 1
GUARD = 7                                         # canary elements on either side of an output
RTOL = 1e-9


def lags_of(n_rows):
    return sorted({k for k in LAGS if k <= n_rows - 1} | {n_rows - 1})


@functools.lru_cache(maxsize=None)
def cases():
    """(theta_dim, n_chains, pad, n_rows, max_lag): two chain counts per (theta_dim, n_rows), the padding alternating"""
    out = []
    for di, d in enumerate(DIMS):
        for ri, n_rows in enumerate(ROWS):
            for s in (0, 2):
                ci = (di + ri + s) % len(CHAINS)
                pad = PADS[(ri + ci + s // 2) % 2]
                out += [(d, CHAINS[ci], pad, n_rows, k) for k in lags_of(n_rows)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(n_rows, d, n_chains):
    """the restatement at every lag, computed once: acov_k does not depend on max_lag"""
    mean, acov = R.autocov(R.diag_history(n_rows, d, n_chains), n_rows - 1)
    mean.setflags(write=False)
    acov.setflags(write=False)
    return mean, acov


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((bits64(a) == bits64(b)) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------------------------- CPU: the grid and the inputs
def test_grid_covers_every_pair():
    axes = ("theta_dim", "chains", "pad", "n_rows", "max_lag")
    rows = cases()
    assert {c[0] for c in rows} == set(DIMS) and {c[1] for c in rows} == set(CHAINS) and {c[2] for c in rows} == set(PADS)
    assert {c[3] for c in rows} == set(ROWS) and {c[4] for c in rows} >= set(LAGS)
    for a in range(5):
        for b in range(5):
            if a == b:
                continue
            for v in {c[a] for c in rows}:
                met = {c[b] for c in rows if c[a] == v}
                need = 2
                if axes[b] == "max_lag" and axes[a] == "n_rows":
                    need = min(2, len(lags_of(v)))              # one row has the lag 0 alone
                if axes[a] == "max_lag" and axes[b] == "n_rows":
                    need = min(2, sum(1 for n in ROWS if v in lags_of(n)))
                assert len(met) >= need, (axes[a], v, axes[b], met)


def test_inputs_are_what_the_tests_assume():
    hist = R.diag_history(97, 3, 321)
    assert hist.dtype == np.float32 and hist.shape == (97, 3, 321)
    still = (np.diff(hist, axis=0) == 0).all(axis=1).mean()
    assert 0.2 < still < 0.4                                           # rejected steps
    mean, acov = reference(97, 3, 321)
    assert np.abs(mean).max() > 40 and (acov[0] > 0).all()           # centring matters: |mean| >> sd
    sd = np.sqrt(acov[0]).mean(axis=1)
    assert sd[0] < sd[1] < sd[2] and 3 < sd[2] / sd[0] < 12           # coordinate scales 2^-1 .. 2^1.5


# ---------------------------------------------------------------------------------- GPU: glabc_autocov
def guarded(size):
    """a device buffer of `size` float64 canaries between two guard bands -> (tensor, pointer to the middle)"""
    t = dev(canary_f64(GUARD + size + GUARD))
    return t, t.data_ptr() + 8 * GUARD


def split_guards(t, size):
    a = host(t)
    return a[:GUARD], a[GUARD:GUARD + size], a[GUARD + size:]


def hip_autocov(hip, hist, max_lag, n=None, expect=0):
    """-> (mean [d][n], acov [max_lag + 1][d][n]) from glabc_autocov, outputs between guard bands"""
    n_rows, d, stride = hist.shape
    n = stride if n is None else n
    mean_t, mean_p = guarded(d * n)
    acov_t, acov_p = guarded((max_lag + 1) * d * n)
    h = dev(np.array(hist))
    assert hip.glabc_autocov(h.data_ptr(), n_rows, d, n, stride, max_lag, mean_p, acov_p, None) == expect
    lo, mean, hi = split_guards(mean_t, d * n)
    lo2, acov, hi2 = split_guards(acov_t, (max_lag + 1) * d * n)
    assert_untouched(lo, hi, lo2, hi2)
    if expect == 0 and n > 0:
        assert_written(mean, acov)
    else:
        assert_untouched(mean, acov)
    return mean.reshape(d, n), acov.reshape(max_lag + 1, d, n)


@pytest.mark.gpu
@pytest.mark.parametrize("d", DIMS)
def test_autocov_matches_the_restatement_bit_for_bit(hip, d):
    n_cases = 0
    for _, n, pad, n_rows, max_lag in (c for c in cases() if c[0] == d):
        hist = R.diag_history(n_rows, d, n)
        ref_mean, ref_acov = reference(n_rows, d, n)
        mean, acov = hip_autocov(hip, R.padded(hist, pad) if pad else hist, max_lag, n)
        assert same_bits(mean, ref_mean), ("mean", d, n, pad, n_rows, max_lag)
        bad = ~((bits64(acov) == bits64(ref_acov[:max_lag + 1])) | (np.isnan(acov) & np.isnan(ref_acov[:max_lag + 1])))
        assert not bad.any(), ("acov", d, n, pad, n_rows, max_lag, "first differing (lag, coordinate, chain):", np.argwhere(bad)[0])
        n_cases += 1
    assert n_cases >= 2 * len(ROWS)
    # two calls give equal bits
    hist = R.diag_history(97, d, 321)
    a, b = hip_autocov(hip, hist, 96), hip_autocov(hip, hist, 96)
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows, max_lag", [(1, 0), (33, 32), (97, 96)])
def test_constant_chain_is_exact(hip, n_rows, max_lag):
    hist = np.array(R.diag_history(n_rows, 2, 65))
    hist[:, 0, 7] = np.float32(50.3)                                  # one coordinate of chain 7 never moves
    hist[:, :, 64] = np.float32(-1e-3)                                # all of chain 64
    mean, acov = hip_autocov(hip, hist, max_lag)
    assert mean[0, 7] == np.float32(50.3) and (mean[:, 64] == np.float32(-1e-3)).all()
    assert (bits64(acov[:, 0, 7]) == 0).all() and (bits64(acov[:, :, 64]) == 0).all()          # +0.0 exactly
    ref_mean, ref_acov = R.autocov(hist, max_lag)
    assert same_bits(mean, ref_mean) and same_bits(acov, ref_acov)


@pytest.mark.gpu
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("n_rows, row, max_lag", [(97, 0, 96), (97, 48, 48), (33, 32, 32), (41, 20, 20)])
def test_nan_or_inf_stays_in_its_own_chain(hip, value, n_rows, row, max_lag):
    """One NaN or infinity makes the chain's mean non-finite, so every centred value is NaN or infinite and every lag whose
    pairs include that row is NaN: all lags here (row <= ... <= max_lag puts the row in a pair of each)"""
    clean = R.diag_history(n_rows, 3, 65)
    hist = np.array(clean)
    hist[row, 1, 9] = value
    mean, acov = hip_autocov(hip, hist, max_lag)
    assert not np.isfinite(mean[1, 9]) and np.isnan(acov[:, 1, 9]).all()
    ref_mean, ref_acov = R.autocov(hist, max_lag)
    assert same_bits(mean, ref_mean) and same_bits(acov, ref_acov)
    clean_mean, clean_acov = reference(n_rows, 3, 65)
    keep = np.ones((3, 65), bool)
    keep[1, 9] = False
    assert (bits64(mean)[keep] == bits64(clean_mean)[keep]).all()
    assert (bits64(acov)[:, keep] == bits64(clean_acov[:max_lag + 1])[:, keep]).all()


@pytest.mark.gpu
def test_autocov_refusals(hip):
    n_rows, d, n = 40, 3, 70
    hist = dev(np.array(R.diag_history(n_rows, d, n)))
    mean_t, mp = guarded(d * n)
    acov_t, ap = guarded(40 * d * n)
    h = hist.data_ptr()
    for rc, args in ((ERR_NULL, (None, n_rows, d, n, n, 8, mp, ap)), (ERR_NULL, (h, n_rows, d, n, n, 8, None, ap)),
                     (ERR_NULL, (h, n_rows, d, n, n, 8, mp, None)), (ERR_NULL, (None, n_rows, 0, n, n, 8, mp, ap)),
                     (ERR_DIM, (h, n_rows, 0, n, n, 8, mp, ap)), (ERR_DIM, (h, n_rows, 9, n, n, 8, mp, ap)),
                     (ERR_DIM, (h, n_rows, -1, n, n, 8, mp, ap)),
                     (ERR_ARG, (h, 0, d, n, n, 0, mp, ap)), (ERR_ARG, (h, -3, d, n, n, 0, mp, ap)),
                     (ERR_ARG, (h, n_rows, d, -1, n, 8, mp, ap)), (ERR_ARG, (h, n_rows, d, n, n - 1, 8, mp, ap)),
                     (ERR_ARG, (h, n_rows, d, n, n, -1, mp, ap)), (ERR_ARG, (h, n_rows, d, n, n, n_rows, mp, ap)),
                     (ERR_ARG, (h, 1, d, n, n, 1, mp, ap)), (ERR_ARG, (h, 5000, d, n, n, 4097, mp, ap)),
                     (0, (h, n_rows, d, 0, n, 8, mp, ap)), (0, (h, n_rows, d, 0, 0, 8, mp, ap))):
        assert hip.glabc_autocov(*args, None) == rc, args
        assert_untouched(host(mean_t), host(acov_t))


# ---------------------------------------------------------------------------------- GPU: diagnostics.py
def assert_no_marginal_pair(examined):
    for per_coordinate in examined:
        assert (np.abs(np.asarray(per_coordinate)) > 1e-6).all(), per_coordinate


def assert_summary_close(got, want):
    for key in ("mean", "sd", "mcse", "rhat", "ess", "tau"):
        np.testing.assert_allclose(got[key], want[key], rtol=RTOL, atol=0, err_msg=key)
    assert np.array_equal(got["truncated"], want["truncated"])


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [50.0, 0.0])
@pytest.mark.parametrize("n_rows", [64, 97])
@pytest.mark.parametrize("m_chains", [1, 64, 321])
def test_rhat_ess_summary_match_the_restatement(hip, m_chains, n_rows, offset):
    from glabcmcmc_amd import diagnostics as D
    hist = R.diag_history(n_rows, 3, m_chains, offset)
    rows = torch.from_numpy(np.array(hist.transpose(0, 2, 1), order="C"))          # (T, C, D)
    for max_lag in (16, 33):
        ref = R.ess(hist, max_lag)
        assert_no_marginal_pair(ref["examined"])                                    # on the CPU, before the GPU is asked
        got = D.ess(rows, max_lag)
        assert got.max_lag == max_lag
        np.testing.assert_allclose(got.tau, ref["tau"], rtol=RTOL, atol=0)
        np.testing.assert_allclose(got.ess, ref["ess"], rtol=RTOL, atol=0)
        assert np.array_equal(got.truncated, ref["truncated"])
        assert_summary_close(D.summary(rows, max_lag), R.summary(hist, max_lag))
    for split in (True, False):
        np.testing.assert_allclose(D.rhat(rows, split=split), R.rhat(hist, split=split), rtol=RTOL, atol=0)
    # the Terms of the history answer as the history does, and so do the combined Terms of its shards
    t = D.terms(rows, 33)
    assert (t.M, t.n, t.half_n) == (m_chains, n_rows, n_rows // 2)
    assert np.array_equal(D.ess(t).tau, D.ess(rows, 33).tau) and np.array_equal(D.rhat(t), D.rhat(rows))
    np.testing.assert_allclose(D.ess(t, 16).tau, R.ess(hist, 16)["tau"], rtol=RTOL, atol=0)
    if m_chains > 1:
        cut = m_chains // 3 + 1
        both = D.combine([D.terms(rows[:, :cut], 33), D.terms(rows[:, cut:], 33)])
        np.testing.assert_allclose(D.ess(both).tau, ref["tau"], rtol=RTOL, atol=0)
        np.testing.assert_allclose(D.rhat(both), R.rhat(hist), rtol=RTOL, atol=0)


@pytest.mark.gpu
def test_every_layout_gives_equal_bits(hip):
    from glabcmcmc_amd import diagnostics as D
    hist = R.diag_history(97, 3, 65)                                                # chain-major (T, D, C)
    ref_mean, ref_acov = reference(97, 3, 65)
    rows = np.array(hist.transpose(0, 2, 1), order="C")                             # (T, C, D), its own memory
    view = dev(np.array(hist)).permute(0, 2, 1)                                     # (T, C, D) view of a chain-major device buffer
    outs = [D.autocovariance(hist, 40, layout="chain_major"), D.autocovariance(torch.from_numpy(np.array(hist)), 40, layout="chain_major"),
            D.autocovariance(rows, 40), D.autocovariance(torch.from_numpy(rows), 40), D.autocovariance(view, 40),
            D.autocovariance(torch.from_numpy(rows.astype(np.float64)), 40)]        # float64 holding float32 values
    for mean, acov in outs:
        assert mean.is_cuda and acov.is_cuda and mean.dtype == acov.dtype == torch.float64
        assert mean.shape == (3, 65) and acov.shape == (41, 3, 65)
        assert same_bits(host(mean), ref_mean) and same_bits(host(acov), ref_acov[:41])
    one_mean, one_acov = D.autocovariance(rows[:, 5], 40)                           # (T, D): a single chain
    assert same_bits(host(one_mean), ref_mean[:, 5:6]) and same_bits(host(one_acov), ref_acov[:41, :, 5:6])
    want = D.summary(rows, 33)
    for other in (D.summary(hist, 33, layout="chain_major"), D.summary(view, 33)):
        for key in want:
            assert np.array_equal(bits64(want[key]) if want[key].dtype != bool else want[key],
                                  bits64(other[key]) if other[key].dtype != bool else other[key]), key


@pytest.mark.gpu
def test_summary_of_a_sampler_run_in_place(hip):
    import glabcmcmc_amd as g
    from glabcmcmc_amd import diagnostics as D
    from glabcmcmc_amd.examples.Mixture import Mixture_set
    m = Mixture_set(0.3)
    lp = g.DiagGaussian(2, loc=torch.zeros(1, 2), log_scale=torch.log(torch.tensor([0.35, 0.35])))
    ip = g.DiagGaussian(2, torch.tensor([0.0, 0.0]), torch.tensor([0.0, 0.0]))
    chains, iters = 256, 200
    out = g.GLMCMC(m, iters, torch.zeros(chains, 2), torch.zeros(chains, 2) + 0.1, lp, None, 0.7, ip, 5, seed=11, return_device=True,
                   verbose=False)
    assert out.is_cuda and out.shape == (iters, chains, 2)
    hist = np.ascontiguousarray(out.cpu().numpy().transpose(0, 2, 1))              # the host copy, chain-major
    want = R.summary(hist, iters - 1)                                               # the default max_lag: min(n - 1, 256)
    assert_no_marginal_pair(R.ess(hist, iters - 1)["examined"])
    history_bytes = out.numel() * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    got = D.summary(out)
    grown = torch.cuda.max_memory_allocated() - before
    print("summary of %d bytes of history: peak device memory grew by %d bytes" % (history_bytes, grown))
    assert grown < history_bytes
    assert_summary_close(got, want)
    assert np.isfinite(got["ess"]).all() and (got["rhat"] > 0.9).all()
