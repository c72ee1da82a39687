"""regression -- local-linear regression adjustment of ABC draws (Beaumont, Zhang and Balding 2002).

Keep the draws within a loose tolerance ``delta``, fit theta = alpha + B^T (y - y_obs) + e by least squares with kernel weights in
the distance (Epanechnikov: 1 - (d / delta)^2), and move every kept draw to theta - B^T (y - y_obs): what theta would have been had
the simulation hit the data, to first order.  Where a simulation is dear this buys from a loose tolerance what plain rejection needs
a far tighter one for.  The adjustment can leave the prior's support: ``Adjusted.outside_prior`` is the weighted share that did.

Three steps, each usable on its own:

``terms``    the weighted Gram of a shard of rows: with z = (1, y - y_obs, theta) and P = 1 + y_dim + theta_dim, the packed upper
             triangle of sum_r w_r z_r z_r^T and, last, sum_r w_r^2 -- Q = P (P + 1) / 2 + 1 float64 numbers (154 at most).
             ``glabc_weighted_gram`` (include/glabc.h, csrc/glabc_regress.hip) reads the float32 arrays in place, with no float64
             design matrix, in a summation order the header states and tests/regress_ref.py reproduces bit for bit.
``combine``  adds the Grams of shards in list order, in float64: deterministic for a given split, and equal to the one-shot Gram up
             to rounding (the kernel's segments restart at every shard, so the bits differ from the one-shot Gram's).
``fit``      NumPy float64 on the host: centre, solve the y_dim x y_dim system -> alpha, B, the residual covariance and Kish's
             effective sample size, all from the Gram alone.
``apply``    ``glabc_regression_apply``: the row-wise correction with the fitted B.

A sharded job all-reduces the Q doubles of ``terms``; every rank then fits and applies the same B.

``path="auto"`` takes the kernels for CUDA tensors and plain torch float64 for CPU tensors; ``path="generic"`` is the same
arithmetic in plain torch float64 wherever the tensors live (what callback Models and CPU results of
``rejection.sample(path="generic")`` get); ``path="fused"`` insists on the kernels.  The generic path's sums are torch's, in no
stated order: it agrees with the kernels to rounding, not to the bit.

Layout.  ``rejection.sample`` returns theta and y as (n, D) views of dimension-major buffers; those are read in place.  Any other
float32 layout is first copied to a dimension-major float32 buffer (4 bytes per value).
"""
import ctypes as C
import math
from collections import namedtuple

import numpy as np
import torch

from . import _capi, rejection

KINDS = {"epanechnikov": 0, "uniform": 1}          # GLABC_GRAM_EPANECHNIKOV, GLABC_GRAM_UNIFORM
SEGMENT = 1024                                      # GLABC_GRAM_SEGMENT
MAX_DIM = 8                                         # GLABC_MAX_DIM

Fit = namedtuple("Fit", "alpha beta mean covariance ess")
Adjusted = namedtuple("Adjusted", "theta weights alpha beta mean covariance ess delta outside_prior gram")


def n_stats(theta_dim, y_dim):
    """Q: the length of a Gram"""
    p = 1 + y_dim + theta_dim
    return p * (p + 1) // 2 + 1


def workspace_size(n, theta_dim, y_dim):
    """doubles of workspace ``glabc_weighted_gram`` needs for n rows"""
    return (n + SEGMENT - 1) // SEGMENT * n_stats(theta_dim, y_dim)


# ---------------------------------------------------------------------------------- arguments
def _kind(kernel):
    if kernel not in KINDS:
        raise ValueError('kernel is "epanechnikov" or "uniform", got %r' % (kernel,))
    return KINDS[kernel]


def _delta(delta):
    try:
        d = float(delta)
    except (TypeError, ValueError):
        raise ValueError("delta must be a number, got %r" % (delta,)) from None
    if not d > 0.0:
        raise ValueError("delta must be > 0 (inf is legal), got %r" % (delta,))
    return d


def _rows(theta, y, distance, weights):
    if not (torch.is_tensor(theta) and torch.is_tensor(y)) or theta.dim() != 2 or y.dim() != 2 or theta.shape[0] != y.shape[0]:
        raise ValueError("theta is an (n, theta_dim) tensor and y an (n, y_dim) tensor of the same n")
    n, d, yd = theta.shape[0], theta.shape[1], y.shape[1]
    if not (1 <= d <= MAX_DIM and 1 <= yd <= MAX_DIM):
        raise ValueError("theta_dim and y_dim are 1 .. %d, got %d and %d" % (MAX_DIM, d, yd))
    for name, v in (("distance", distance), ("weights", weights)):
        if v is not None and (not torch.is_tensor(v) or v.reshape(-1).shape[0] != n):
            raise ValueError("%s holds one number per row (%d), got %r" % (name, n, None if not torch.is_tensor(v) else tuple(v.shape)))
    return n, d, yd


def _y_obs(y_obs, yd):
    v = np.asarray(y_obs.detach().cpu().numpy() if torch.is_tensor(y_obs) else y_obs, np.float64).reshape(-1)
    if v.shape[0] != yd:
        raise ValueError("y_obs has %d entries, y has %d columns" % (v.shape[0], yd))
    return np.ascontiguousarray(v)


def _fused(path, *tensors):
    """The one place that decides what a call runs: True for the kernels"""
    if path not in ("auto", "fused", "generic"):
        raise ValueError('path is "auto", "fused" or "generic", got %r' % (path,))
    cuda = all(t.is_cuda for t in tensors if t is not None)
    if path == "fused" and not cuda:
        raise ValueError('path="fused" needs CUDA tensors')
    return path != "generic" and cuda


def _dimension_major(x):
    """(n, D) -> (float32 tensor whose storage is read, stride between coordinates): in place where column j of x is contiguous
    (what rejection.sample returns), else a [D][n] copy"""
    n, d = x.shape
    if x.dtype == torch.float32 and (n <= 1 or x.stride(0) == 1) and (d == 1 or x.stride(1) >= max(n, 1)):
        return x, (x.stride(1) if d > 1 else max(n, 1))
    t = x.to(torch.float32).t().contiguous()
    return t, max(n, 1)


def _vector(v, dev):
    return None if v is None else v.reshape(-1).to(device=dev, dtype=torch.float32).contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------- the Gram
def _gram_generic(theta, y, distance, weights, y_obs, delta, kind):
    """the specification's terms in torch float64; the sums are torch's"""
    dev = theta.device
    n = theta.shape[0]
    if distance is None:
        k = torch.ones(n, dtype=torch.float64, device=dev)
    else:
        d = distance.reshape(-1).to(device=dev, dtype=torch.float32).double()
        k = _kernel_weights(d, None, delta, kind)
    w = k if weights is None else k * weights.reshape(-1).to(device=dev, dtype=torch.float32).double()
    keep = torch.nonzero(w != 0.0).view(-1)                          # a row of weight 0 contributes nothing, whatever it holds
    w = w[keep]
    z = torch.cat([torch.ones(keep.numel(), 1, dtype=torch.float64, device=dev),
                   y[keep].to(torch.float32).double() - torch.as_tensor(y_obs, device=dev), theta[keep].to(torch.float32).double()], dim=1)
    m = z.t() @ (w[:, None] * z)
    iu = torch.triu_indices(z.shape[1], z.shape[1])
    return np.concatenate([m[iu[0], iu[1]].cpu().numpy(), [float((w * w).sum())]])


def terms(theta, y, distance=None, weights=None, *, y_obs, delta=math.inf, kernel="epanechnikov", path="auto"):
    """The Gram of a shard of rows -> float64 NumPy array [Q] (module docstring).  theta (n, theta_dim), y (n, y_dim); distance and
    weights (n,) or None: without a distance every row has kernel weight 1, and `weights` (an ``smc.Population``'s) multiply the
    kernel weights.  n == 0 gives Q zeros."""
    n, d, yd = _rows(theta, y, distance, weights)
    kind, delta, y_obs = _kind(kernel), _delta(delta), _y_obs(y_obs, yd)
    if not _fused(path, theta, y, distance, weights):
        return _gram_generic(theta, y, distance, weights, y_obs, delta, kind)
    if n == 0:
        return np.zeros(n_stats(d, yd))
    dev = theta.device
    th, stride_t = _dimension_major(theta)
    ys, stride_y = _dimension_major(y)
    dis, w = _vector(distance, dev), _vector(weights, dev)
    gram = torch.empty(n_stats(d, yd), dtype=torch.float64, device=dev)
    work = torch.empty(workspace_size(n, d, yd), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _capi.check(_capi.lib().glabc_weighted_gram(th.data_ptr(), stride_t, d, ys.data_ptr(), stride_y, yd, _ptr(dis), _ptr(w), n,
                                                    y_obs.ctypes.data, delta, kind, gram.data_ptr(), work.data_ptr(),
                                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "glabc_weighted_gram")
    return gram.cpu().numpy()


def combine(list_of_grams):
    """The Gram of the union of shards: float64 sums in list order.  Deterministic for a given split; equal to the one-shot Gram of
    all rows up to rounding, not to the bit"""
    grams = [np.asarray(g, np.float64) for g in list_of_grams]
    if not grams or any(g.shape != grams[0].shape or g.ndim != 1 for g in grams):
        raise ValueError("combine takes a non-empty list of Grams of one shape")
    total = np.zeros_like(grams[0])
    for g in grams:
        total = total + g
    return total


def unpack(gram, theta_dim, y_dim):
    """-> (the symmetric P x P matrix sum w z z^T, sum w^2)"""
    p = 1 + y_dim + theta_dim
    g = np.asarray(gram, np.float64)
    if g.shape != (n_stats(theta_dim, y_dim),):
        raise ValueError("a Gram of theta_dim %d and y_dim %d has %d entries, got shape %r" % (theta_dim, y_dim, n_stats(theta_dim, y_dim), g.shape))
    m = np.zeros((p, p))
    m[np.triu_indices(p)] = g[:-1]
    return m + np.triu(m, 1).T, float(g[-1])


def fit(gram, theta_dim, y_dim, ridge=0.0):
    """Weighted least squares of theta on (1, y - y_obs) from the Gram alone -> Fit(alpha [D], beta [YD][D], mean [D] (= alpha: the
    fitted theta at y = y_obs), covariance [D][D] (the weighted residual covariance), ess (W^2 / sum w^2)).  Centre, then solve
    (C_yy + ridge * mean(diag C_yy) * I) B = C_y,theta.  ValueError, naming the condition number, where C_yy is singular to working
    precision (condition number above 2^52, or a y column whose variance is within ess * 2^-52 of its second moment: constant) and where fewer than P = 1 + y_dim + theta_dim rows carry weight as Kish's effective sample size
    counts them."""
    if not (isinstance(ridge, (int, float)) and ridge >= 0.0):
        raise ValueError("ridge must be a number >= 0, got %r" % (ridge,))
    m, sum_w2 = unpack(gram, theta_dim, y_dim)
    p, yd = m.shape[0], y_dim
    total = m[0, 0]
    if not total > 0.0 or not sum_w2 > 0.0:
        raise ValueError("no row carries weight (sum of weights %r): widen delta" % (total,))
    ess = total * total / sum_w2
    if ess < p:
        raise ValueError("too few weighted rows: the effective sample size %.3g is below the %d columns of the fit" % (ess, p))
    second = m[1:, 1:] / total
    first = m[0, 1:] / total
    c = second - np.outer(first, first)
    cyy, cyt, ctt = c[:yd, :yd], c[:yd, yd:], c[yd:, yd:]
    a = cyy + ridge * np.mean(np.diag(cyy)) * np.eye(yd)
    eps = np.finfo(np.float64).eps
    try:
        cond = float(np.linalg.cond(a))
    except np.linalg.LinAlgError:
        cond = math.inf
    # a variance within the worst-case rounding error of its second moment, a sum of about `ess` terms: a constant column
    flat = np.diag(a) <= ess * eps * np.diag(second)[:yd]
    if flat.any() or not np.isfinite(cond) or cond > 1.0 / eps:
        raise ValueError("the y - y_obs columns are collinear to working precision (condition number %.3g%s): drop the column or pass ridge > 0"
                         % (cond, ", constant column %s" % np.nonzero(flat)[0].tolist() if flat.any() else ""))
    beta = np.linalg.solve(a, cyt)
    alpha = first[yd:] - beta.T @ first[:yd]
    cov = ctt - beta.T @ cyt - cyt.T @ beta + beta.T @ cyy @ beta
    return Fit(alpha, beta, alpha.copy(), 0.5 * (cov + cov.T), ess)


# ---------------------------------------------------------------------------------- the correction
def apply(theta, y, beta, *, y_obs, path="auto", out=None):
    """theta - B^T (y - y_obs) for every row -> float32 (n, theta_dim).  beta [y_dim][theta_dim] as ``fit`` returns it.  out: None
    (a new tensor) or `theta` itself (in place, fused path on rows that are read in place)."""
    n, d, yd = _rows(theta, y, None, None)
    y_obs = _y_obs(y_obs, yd)
    beta = np.ascontiguousarray(np.asarray(beta, np.float64))
    if beta.shape != (yd, d):
        raise ValueError("beta is [y_dim][theta_dim] = %r, got %r" % ((yd, d), beta.shape))
    if out is not None and out is not theta:
        raise ValueError("out is None or theta itself")
    if not _fused(path, theta, y):
        dy = y.to(torch.float32).double() - torch.as_tensor(y_obs, device=y.device)
        a = theta.to(torch.float32).double()
        for k in range(yd):                                          # k ascending, one rounded product and difference each
            a = a - torch.as_tensor(beta[k], device=theta.device)[None, :] * dy[:, k:k + 1]
        a = a.to(torch.float32)
        if out is None:
            return a
        theta.copy_(a)
        return theta
    dev = theta.device
    th, stride_t = _dimension_major(theta)
    ys, stride_y = _dimension_major(y)
    if out is not None and th is not theta:
        raise ValueError("in place needs float32 rows in the dimension-major layout of rejection.sample")
    res = th if out is not None else torch.empty(d, max(n, 1), dtype=torch.float32, device=dev)
    stride_o = stride_t if out is not None else max(n, 1)
    if n:
        with torch.cuda.device(dev):
            _capi.check(_capi.lib().glabc_regression_apply(th.data_ptr(), stride_t, d, ys.data_ptr(), stride_y, yd, n, y_obs.ctypes.data,
                                                           beta.ctypes.data, res.data_ptr(), stride_o,
                                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "glabc_regression_apply")
    return theta if out is not None else res[:, :n].t()


# ---------------------------------------------------------------------------------- the whole step
def _draws(ABCset, draws, weights):
    """-> theta, y, distance, weights of a Rejection, a Population or a (theta, y[, distance]) tuple"""
    if hasattr(draws, "theta") and hasattr(draws, "y") and hasattr(draws, "distance"):
        theta, y, dis = draws.theta, draws.y, draws.distance
        own = getattr(draws, "weights", None)
        if own is not None:
            own = torch.as_tensor(own)
            weights = own if weights is None else own.to(torch.float64) * torch.as_tensor(weights).to(own.device, torch.float64)
    elif isinstance(draws, (tuple, list)) and len(draws) in (2, 3):
        theta, y = draws[0], draws[1]
        dis = draws[2] if len(draws) == 3 else None
    else:
        raise ValueError("draws is a rejection.Rejection, an smc.Population or a (theta, y[, distance]) tuple, got %r" % (type(draws),))
    if dis is None:
        dis = ABCset.discrepancy(y).reshape(-1)
    if weights is not None:
        weights = torch.as_tensor(weights).reshape(-1).to(theta.device)
    return theta, y, dis.reshape(-1).to(theta.device), weights


def _pick_delta(dis, delta, quantile):
    if delta is not None and quantile is not None:
        raise ValueError("adjust takes delta or quantile, not both")
    if delta is not None:
        return _delta(delta)
    d = dis.to(torch.float32)
    n_valid = int((~torch.isnan(d)).sum())
    if n_valid == 0:
        raise ValueError("no row has a distance")
    if quantile is None:
        return float(d[~torch.isnan(d)].max())                       # the largest kept distance
    q = float(quantile) if isinstance(quantile, (int, float, np.floating, np.integer)) and not isinstance(quantile, bool) else math.nan
    if not 0.0 <= q <= 1.0:
        raise ValueError("quantile must be a number in [0, 1], got %r" % (quantile,))
    rank = int(math.floor(q * (n_valid - 1)))                        # rejection's rule; NaNs sort last
    if d.is_cuda:
        return _delta(rejection._select_rank(d.contiguous(), rank))  # exact and sort-free: diagnostics.select over key counts
    return _delta(float(torch.kthvalue(d[~torch.isnan(d)], rank + 1).values))


def _kernel_weights(dis, weights, delta, kind):
    """w_r of the specification, in its operations: float64 (n,)"""
    d = dis.to(torch.float32).double()
    # a tensor divisor: torch divides by a Python number as a product with its reciprocal, which is not the specification's d / delta
    u = d / torch.tensor([delta], dtype=torch.float64, device=d.device)
    inside = d <= delta                                              # a NaN distance fails the comparison
    k = torch.where(inside, 1.0 - u * u if kind == KINDS["epanechnikov"] else torch.ones_like(d), torch.zeros_like(d))
    return k if weights is None else k * weights.to(torch.float32).double()


def adjust(ABCset, draws, *, delta=None, quantile=None, kernel="epanechnikov", weights=None, ridge=0.0, path="auto"):
    """Regression-adjust kept draws -> Adjusted(theta (n, D) float32, weights (n,) float64 summing to 1, alpha, beta, mean,
    covariance, ess, delta, outside_prior, gram).  draws: a ``rejection.Rejection``, an ``smc.Population`` (its weights multiply
    the kernel weights) or a (theta, y[, distance]) tuple (a missing distance is ``ABCset.discrepancy(y)``).  delta: the largest kept
    distance by default, or the `quantile` of the kept distances.  Every row is corrected, whatever its weight; rows of weight 0
    (beyond delta) take no part in the fit or in ``outside_prior``, the weighted share of adjusted draws that
    ``ABCset.prior_log_prob`` puts at -inf.  mean, covariance and ess come from the Gram alone (``fit``)."""
    theta, y, dis, weights = _draws(ABCset, draws, weights)
    n, d, yd = _rows(theta, y, dis, weights)
    kind = _kind(kernel)
    if n == 0:
        raise ValueError("no draws to adjust")
    delta = _pick_delta(dis, delta, quantile)
    gram = terms(theta, y, dis, weights, y_obs=ABCset.y_obs, delta=delta, kernel=kernel, path=path)
    f = fit(gram, d, yd, ridge)
    adjusted = apply(theta, y, f.beta, y_obs=ABCset.y_obs, path=path)
    w = _kernel_weights(dis, weights, delta, kind)
    w = w / w.sum()
    log_prior = ABCset.prior_log_prob(adjusted.contiguous()).reshape(-1).to(w.device)
    outside = float(w[torch.isinf(log_prior) & (log_prior < 0)].sum())
    return Adjusted(adjusted, w, f.alpha, f.beta, f.mean, f.covariance, f.ess, delta, outside, gram)
