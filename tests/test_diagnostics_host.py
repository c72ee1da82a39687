"""Chain diagnostics on the CPU: the restatement the GPU tests trust (tests/diag_ref.py) against an FFT and against an AR(1)
process's known autocorrelation time, and the parts of glabcmcmc_amd/diagnostics.py that need no device -- combine / pack, the
Geyer sequence, every ValueError -- plus glabc_autocov's refusals as csrc/glabc_check.h answers them under g++.
"""
import numpy as np
import pytest

import diag_ref as R
from glabcmcmc_amd import diagnostics as D
from test_arg_checks import check_table

OK, NULL, DIM, ARG = 0, -1, -2, -4


# ---------------------------------------------------------------------------------- the restatement against an FFT
@pytest.mark.parametrize("n_rows, d, n_chains", [(97, 2, 65), (400, 1, 8), (512, 3, 5)])
def test_restatement_matches_fft(n_rows, d, n_chains):
    """Autocovariances of the same centred data through np.fft (zero-padded to >= 2T points, at most 1024): the FFT's error at
    1024 points is about 10 log2(1024) 2^-53 = 1e-14 relative to acov_0, the bound is 1e-12 acov_0 per chain"""
    hist = R.diag_history(n_rows, d, n_chains)
    max_lag = n_rows - 1
    mean, acov = R.autocov(hist, max_lag)
    u = hist.astype(np.float64) - mean                                  # the restatement's own centring
    size = 1 << int(np.ceil(np.log2(2 * n_rows)))
    assert 2 * n_rows <= size <= 1024
    f = np.fft.rfft(u, n=size, axis=0)
    fft_acov = np.fft.irfft(f * np.conj(f), n=size, axis=0)[:n_rows] / n_rows
    err = np.abs(acov - fft_acov).max(axis=0)
    assert (acov[0] > 0).all()
    print("largest |restatement - fft| / acov_0: %.3g" % (err / acov[0]).max())
    assert (err <= 1e-12 * acov[0]).all()


def ar1_history(m_chains=256, n_rows=400, phi=0.5, seed=20261019):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((n_rows, m_chains))
    x = np.empty((n_rows, m_chains))
    x[0] = z[0] / np.sqrt(1.0 - phi ** 2)
    for t in range(1, n_rows):
        x[t] = phi * x[t - 1] + z[t]
    return np.ascontiguousarray(x.astype(np.float32)[:, None, :])


AR1_TAU_TOL = 2 * 0.0796


def test_restatement_finds_ar1_autocorrelation_time():
    """AR(1) with phi = 0.5 has tau = (1 + phi) / (1 - phi) = 3.  On this fixed input (seed 20261019, M = 256 chains of n = 400)
    the restatement gives tau = 2.92040 at max_lag 32, 64 and 128 alike (the sequence stops at the sixth pair): an error of
    0.0796, measured on the CPU (x86-64, NumPy float64).  The tolerance is twice that.  R-hat of these chains is 1.0043."""
    hist = ar1_history()
    for max_lag in (32, 64, 128):
        e = R.ess(hist, max_lag)
        print("max_lag %d: tau %.6f, error %.4g" % (max_lag, e["tau"][0], abs(e["tau"][0] - 3.0)))
        assert abs(e["tau"][0] - 3.0) <= AR1_TAU_TOL
        assert not e["truncated"][0]
        assert e["ess"][0] == pytest.approx(256 * 400 / e["tau"][0], rel=1e-15)
    assert abs(R.rhat(hist)[0] - 1.0) < 0.01


# ---------------------------------------------------------------------------------- combine
def ref_terms(hist, max_lag):
    """diagnostics.Terms of a shard, built from the restatement's per-chain numbers"""
    n_rows, d, m = hist.shape
    mean, acov = R.autocov(hist, max_lag)
    half = n_rows // 2
    hm, hs, ha = np.zeros((2, d)), np.zeros((2, d)), np.zeros((2, d))
    for i, rows in enumerate((hist[:half], hist[n_rows - half:])):
        pm, pa = R.autocov(rows, 0)
        hm[i], hs[i], ha[i] = pm.sum(1), (pm * pm).sum(1), pa[0].sum(1)
    return D.Terms(m, n_rows, mean.sum(1), (mean * mean).sum(1), acov.sum(2), half, hm, hs, ha)


def assert_terms_close(a, b, rtol):
    assert (a.M, a.n, a.half_n) == (b.M, b.n, b.half_n)
    for name in ("sum_mean", "sum_mean_sq", "sum_acov", "half_sum_mean", "half_sum_mean_sq", "half_sum_acov0"):
        x, y = np.asarray(getattr(a, name)), np.asarray(getattr(b, name))
        assert x.shape == y.shape, name
        assert np.all(np.abs(x - y) <= rtol * np.abs(y)), (name, np.abs(x - y).max())


@pytest.mark.parametrize("shards", [(64, 65), (100, 1, 156)])
def test_combine_of_shards_is_the_whole(shards):
    """A handful of double additions in another order: 1e-13 relative"""
    m, max_lag = sum(shards), 16
    hist = R.diag_history(64, 3, m)
    whole = ref_terms(hist, max_lag)
    parts, at = [], 0
    for k in shards:
        parts.append(ref_terms(hist[:, :, at:at + k], max_lag))
        at += k
    got = D.combine(parts)
    assert_terms_close(got, whole, 1e-13)
    # the packed vector is what ranks all-reduce: its sum over shards unpacks to the same Terms
    packed = sum(D.pack(p) for p in parts)
    assert_terms_close(D.unpack(packed, whole.n, whole.half_n, 3), whole, 1e-13)
    # ... and the formulas read the combined Terms as they read the whole's
    assert np.allclose(D.rhat(got), D.rhat(whole), rtol=1e-12, atol=0)
    assert np.allclose(D.ess(got).tau, D.ess(whole).tau, rtol=1e-12, atol=0)
    assert np.allclose(D.rhat(whole), R.rhat(hist), rtol=1e-11, atol=0)
    ref = R.ess(hist, max_lag)
    assert np.allclose(D.ess(whole).tau, ref["tau"], rtol=1e-9, atol=0) and np.array_equal(D.ess(whole).truncated, ref["truncated"])


def test_combine_refuses_shards_that_do_not_match():
    a = ref_terms(R.diag_history(64, 2, 5), 8)
    with pytest.raises(ValueError):
        D.combine([a, ref_terms(R.diag_history(64, 2, 5), 9)])
    with pytest.raises(ValueError):
        D.combine([a, ref_terms(R.diag_history(65, 2, 5), 8)])
    with pytest.raises(ValueError):
        D.combine([])


# ---------------------------------------------------------------------------------- the Geyer sequence by hand
def test_geyer_sequence_on_hand_written_rho():
    # a negative pair at j = 1: only P_0 = 1.5 counts
    tau, trunc = D.geyer_tau([1.0, 0.5, -0.25, 0.125, 0.5, 0.5])
    assert tau == -1.0 + 2.0 * 1.5 and not trunc
    # the monotone clamp: P = 1.5, 0.25, 0.5 -> 0.25, then a negative pair
    tau, trunc = D.geyer_tau([1.0, 0.5, 0.125, 0.125, 0.25, 0.25, -0.5, 0.25])
    assert tau == -1.0 + 2.0 * (1.5 + 0.25 + 0.25) and not trunc
    # no negative pair within max_lag: truncated, an upper bound on ESS
    tau, trunc = D.geyer_tau([1.0, 0.5, 0.25, 0.125])
    assert tau == -1.0 + 2.0 * (1.5 + 0.375) and trunc
    # max_lag even: lag 4 has no partner and is not read
    tau, trunc = D.geyer_tau([1.0, 0.5, 0.25, 0.125, 1e9])
    assert tau == -1.0 + 2.0 * (1.5 + 0.375) and trunc
    tau, trunc = D.geyer_tau([1.0, 0.5, 0.25, 0.125, -1e9])
    assert tau == -1.0 + 2.0 * (1.5 + 0.375) and trunc
    # max_lag = 1 and 2: P_0 alone, never cut
    for rho in ([1.0, -3.0], [1.0, -3.0, 7.0]):
        tau, trunc = D.geyer_tau(rho)
        assert tau == -1.0 + 2.0 * -2.0 and trunc
    # a pair sum of exactly zero is not negative
    tau, trunc = D.geyer_tau([1.0, 0.5, 0.25, -0.25, -0.5, 0.25])
    assert tau == -1.0 + 2.0 * 1.5 and not trunc
    # per coordinate, and the restatement agrees
    rho = np.array([[1.0, 0.5, -0.25, 0.125, 0.5, 0.5], [1.0, 0.5, 0.125, 0.125, 0.25, 0.25]]).T
    tau, trunc = D.geyer_tau(rho)
    assert tau.tolist() == [2.0, -1.0 + 2.0 * (1.5 + 0.25 + 0.25)] and trunc.tolist() == [False, True]
    for j in range(2):
        assert R.geyer(rho[:, j])[:2] == (tau[j], trunc[j])
    with pytest.raises(ValueError):
        D.geyer_tau([1.0])


def test_constant_chains_give_nan_without_an_exception():
    t = D.Terms(4, 10, np.array([8.0]), np.array([16.0]), np.zeros((4, 1)), 5, np.full((2, 1), 8.0), np.full((2, 1), 16.0),
                np.zeros((2, 1)))
    assert np.isnan(D.rhat(t)).all() and np.isnan(D.rhat(t, split=False)).all()
    e = D.ess(t)
    assert np.isnan(e.ess).all() and np.isnan(e.tau).all()


# ---------------------------------------------------------------------------------- argument errors, no GPU needed
def test_argument_errors_come_before_any_device(monkeypatch):
    from glabcmcmc_amd import engine

    def no_device(*a, **k):
        raise AssertionError("an argument error must be raised before the device is asked for")
    monkeypatch.setattr(engine, "require_device", no_device)
    ok = np.zeros((10, 3, 2), np.float32)
    for bad in (np.zeros(5, np.float32), np.zeros((5, 2, 2, 2), np.float32)):          # a wrong rank
        for call in (lambda h: D.autocovariance(h, 0), lambda h: D.terms(h, 0), D.rhat, D.ess, D.summary):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError):
        D.autocovariance(np.zeros((5, 2), np.float32), 0, layout="chain_major")      # chain-major is (T, D, C)
    with pytest.raises(ValueError):
        D.terms(ok, 0, layout="columns")
    with pytest.raises(ValueError):
        D.terms(np.zeros((10, 3, 9), np.float32), 0)                                  # more than GLABC_MAX_DIM coordinates
    for max_lag in (-1, 10, 4097, 2.5):                                               # out of range: n - 1 = 9
        for call in (D.autocovariance, D.terms):
            with pytest.raises(ValueError):
                call(ok, max_lag)
    for max_lag in (0, 10):                                                           # ESS needs a pair of lags
        with pytest.raises(ValueError):
            D.ess(ok, max_lag)
        with pytest.raises(ValueError):
            D.summary(ok, max_lag)
    with pytest.raises(ValueError):
        D.terms(np.zeros((5000, 1, 1), np.float32), 4097)                             # GLABC_MAX_LAG
    for n in (1, 2, 3):                                                               # split-R-hat needs two halves of two rows
        with pytest.raises(ValueError):
            D.rhat(np.zeros((n, 3, 2), np.float32))
        with pytest.raises(ValueError):
            D.summary(np.zeros((n, 3, 2), np.float32))
    with pytest.raises(ValueError):
        D.rhat(np.zeros((1, 3, 2), np.float32), split=False)
    with pytest.raises(ValueError):
        D.ess(np.zeros((1, 3, 2), np.float32))
    with pytest.raises(ValueError):
        D.terms(ok, 2, first_half_rows=11)


def test_no_cpu_fallback():
    """Without a GPU the module raises; it never computes on the host"""
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            D.ess(np.zeros((10, 3, 2), np.float32))


def test_module_is_exported_and_bound():
    import glabcmcmc_amd
    from glabcmcmc_amd import _capi
    assert glabcmcmc_amd.diagnostics is D and "diagnostics" in glabcmcmc_amd.__all__
    assert "glabc_autocov" in _capi.ENTRY_POINTS and D.MAX_LAG == 4096


# ---------------------------------------------------------------------------------- glabc_autocov's refusals (csrc/glabc_check.h)
def test_check_autocov(tmp_path_factory):
    call = "check_autocov(%s, %s, %s, %s, %s, %s, %s, %s)"
    base = dict(h="b.f", rows="97", d="3", n="65", stride="65", lag="64", mean="b.d", acov="b.d")

    def row(want, **kw):
        a = dict(base, **kw)
        return ("", call % (a["h"], a["rows"], a["d"], a["n"], a["stride"], a["lag"], a["mean"], a["acov"]), want)
    check_table(tmp_path_factory, "autocov", [
        row(OK), row(OK, lag="0"), row(OK, lag="96"), row(OK, rows="1", lag="0"), row(OK, stride="82"), row(OK, n="0", stride="0"),
        row(OK, d="1"), row(OK, d="8"), row(OK, rows="5000", lag="4096"),
        row(NULL, h="nullptr"), row(NULL, mean="nullptr"), row(NULL, acov="nullptr"),
        row(NULL, h="nullptr", d="0"),                                   # a null pointer is reported first
        row(DIM, d="0"), row(DIM, d="9"), row(DIM, d="-1"), row(DIM, d="9", rows="0"),
        row(ARG, rows="0", lag="0"), row(ARG, rows="-5"), row(ARG, n="-1"), row(ARG, stride="64"), row(ARG, lag="-1"),
        row(ARG, lag="97"), row(ARG, rows="1", lag="1"), row(ARG, rows="5000", lag="4097"), row(ARG, rows="100000", lag="99999"),
    ])


# ---------------------------------------------------------------------------------- the committed resource report
def test_resource_report_shows_no_private_segment():
    """profiles/diag_kernel_resources.txt: both kernels without a private segment or a spilled register, and autocov_kernel
    within the 128 VGPRs (AGPRs included) that four wavefronts per SIMD allow"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "profiles", "diag_kernel_resources.txt")).read()
    kernels = re.split(r"^Function Name: ", text, flags=re.M)[1:]
    assert len(kernels) == 2 and "mean_kernel" in kernels[0] and "autocov_kernel" in kernels[1]
    for k in kernels:
        field = lambda name: int(re.search(r"%s: (\d+)" % re.escape(name), k).group(1))          # noqa: E731
        assert field("ScratchSize [bytes/lane]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0
        assert field("VGPRs") + field("AGPRs") <= 128 and field("Occupancy [waves/SIMD]") >= 4
