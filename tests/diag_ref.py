"""Chain diagnostics restated in NumPy float64 loops, vectorised over chains only: the numerical specification of
glabc_autocov (include/glabc.h) in exactly its order, and the R-hat / ESS formulas of glabcmcmc_amd/diagnostics.py computed
from a history.  Shares no code with csrc/ or with diagnostics.py; tests/test_diagnostics_host.py checks it against an FFT and
against an AR(1) process's known autocorrelation time, tests/test_diag_shapes.py holds the kernels and the module to it.

Histories here are chain-major float32 [n_rows][d][stride], as the samplers write them.
"""
import functools

import numpy as np


# ---------------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def diag_history(n_rows, d, n_chains, offset=50.0, seed=0):
    """float32 [n_rows][d][n_chains], read-only.  AR(1) per chain and coordinate, phi per chain in 0.2 .. 0.8; coordinate scales
    2^-1 .. 2^1.5; per-chain offsets up to +-offset (so that centring matters in float32 data); about 30 % of the rows repeat
    the row before (rejected steps); rounded to float32 once"""
    rng = np.random.default_rng([seed, n_rows, d, n_chains, int(offset)])
    phi = rng.uniform(0.2, 0.8, (n_chains, 1))
    scale = 2.0 ** (np.linspace(-1.0, 1.5, d) if d > 1 else np.array([0.5]))
    off = rng.uniform(-offset, offset, (n_chains, d))
    z = rng.standard_normal((n_rows, n_chains, d))
    keep = rng.random((n_rows, n_chains, 1)) >= 0.3
    x = np.empty_like(z)
    x[0] = z[0] / np.sqrt(1.0 - phi ** 2)
    for t in range(1, n_rows):
        x[t] = np.where(keep[t], phi * x[t - 1] + z[t], x[t - 1])
    hist = np.ascontiguousarray((off + scale * x).astype(np.float32).transpose(0, 2, 1))
    hist.setflags(write=False)
    return hist


def padded(hist, pad):
    """the same chains with `pad` columns of NaN behind them (stride = n_chains + pad)"""
    n_rows, d, n = hist.shape
    out = np.full((n_rows, d, n + pad), np.nan, np.float32)
    out[:, :, :n] = hist
    return out


# ---------------------------------------------------------------------------------- section 1: glabc_autocov
def autocov(hist, max_lag, n_chains=None):
    """-> (mean [d][n], acov [max_lag + 1][d][n]) float64; columns n_chains .. stride - 1 are never read"""
    n_rows, d, stride = hist.shape
    n = stride if n_chains is None else n_chains
    assert 0 <= max_lag <= n_rows - 1
    with np.errstate(all="ignore"):
        x = np.asarray(hist)[:, :, :n].astype(np.float64)
        s = np.zeros((d, n))
        for t in range(n_rows):
            s = s + x[t]
        m = s / float(n_rows)
        u = x - m
        acov = np.empty((max_lag + 1, d, n))
        for k in range(max_lag + 1):
            a = np.zeros((d, n))
            for t in range(k, n_rows):
                a = a + u[t] * u[t - k]
            acov[k] = a / float(n_rows)
    return m, acov


# ---------------------------------------------------------------------------------- section 3: the formulas
def _within_between(mean, acov0, n):
    """mean, acov0: [d][M] per chain -> (W, var+) [d]"""
    m_chains = mean.shape[1]
    w = (acov0 * (n / (n - 1.0))).mean(axis=1)
    b_over_n = mean.var(axis=1, ddof=1) if m_chains > 1 else np.zeros(mean.shape[0])
    return w, (n - 1.0) / n * w + b_over_n


def rhat(hist, split=True):
    n_rows = hist.shape[0]
    if split:
        h = n_rows // 2
        hist = np.concatenate([hist[:h], hist[n_rows - h:]], axis=2)          # 2M half-chains of length h
        n_rows = h
    mean, acov = autocov(hist, 0)
    w, var = _within_between(mean, acov[0], n_rows)
    with np.errstate(all="ignore"):
        return np.where(w == 0.0, np.nan, np.sqrt(var / w))


def geyer(rho):
    """rho [K + 1] of one coordinate -> (tau, truncated, examined pair sums before the clamp)"""
    max_lag = len(rho) - 1
    total, prev, truncated, examined = 0.0, None, True, []
    j = 0
    while 2 * j + 1 <= max_lag:
        p = rho[2 * j] + rho[2 * j + 1]
        examined.append(p)
        if j >= 1:
            if p < 0.0:
                truncated = False
                break
            p = min(p, prev)
        total += p
        prev = p
        j += 1
    return -1.0 + 2.0 * total, truncated, examined


def ess(hist, max_lag):
    """-> dict(ess, tau [d], truncated [d] bool, examined: per coordinate the pair sums the sequence looked at, var = var+)"""
    n_rows, d, m_chains = hist.shape
    mean, acov = autocov(hist, max_lag)
    w, var = _within_between(mean, acov[0], n_rows)
    tau, trunc, examined = np.empty(d), np.empty(d, bool), []
    with np.errstate(all="ignore"):
        for j in range(d):
            rho = 1.0 - (w[j] - n_rows / (n_rows - 1.0) * acov[:, j].mean(axis=1)) / var[j]
            rho[0] = 1.0
            if w[j] == 0.0:
                rho[:] = np.nan
            tau[j], trunc[j], ex = geyer(rho)
            examined.append(ex)
        return {"ess": m_chains * n_rows / tau, "tau": tau, "truncated": trunc, "examined": examined, "var": var,
                "mean": mean.mean(axis=1)}


def summary(hist, max_lag):
    e = ess(hist, max_lag)
    with np.errstate(all="ignore"):
        sd = np.sqrt(e["var"])
        return {"mean": e["mean"], "sd": sd, "mcse": sd / np.sqrt(e["ess"]), "rhat": rhat(hist, split=True), "ess": e["ess"],
                "tau": e["tau"], "truncated": e["truncated"]}
