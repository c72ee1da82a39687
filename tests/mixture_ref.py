"""GaussianMixture as include/glabc.h specifies it, restated in numpy float64 for the tests.

Written from the specification's text, not from the kernels: the constants a mixture is made of, ``log_prob`` (the per-mode
terms, torch.sum's float64 order over the coordinates and over the modes, max + log(sum exp)), the draw of a mode and of a
variate, the row-wise ``forward`` and the candidates of a sampler iteration.  Elementary functions, uniforms, Philox and a
candidate's proposal normals come from the CPU checker's exports (oracle_lib); the two pieces restated here for speed --
Philox4x32-10 and the float64 row-sum order, both vectorised over rows -- are held to the checker's own exports by
tests/test_mixture_host.py.  numpy's elementwise + - * are IEEE double operations and never contract into fma.
"""
import ctypes as C

import numpy as np

import oracle_lib

SLOT_MIX = 0x10000000            # GLABC_SLOT_MIX


def rowsum_f64(x):
    """torch.sum's float64 association over the LAST axis (fewer than 16 terms): under four terms in sequence; else four
    partials of every fourth term, then a scalar takes the n % 4 tail in order followed by the four partials in order"""
    x = np.asarray(x, np.float64)
    n = x.shape[-1]
    assert 1 <= n < 16
    if n < 4:
        s = x[..., 0]
        for i in range(1, n):
            s = s + x[..., i]
        return s
    nv = n // 4
    acc = [x[..., k] for k in range(4)]
    for v in range(1, nv):
        for k in range(4):
            acc[k] = acc[k] + x[..., 4 * v + k]
    fa = np.zeros(x.shape[:-1], np.float64)
    for i in range(4 * nv, n):
        fa = fa + x[..., i]
    for k in range(4):
        fa = fa + acc[k]
    return fa


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on uint32 arrays (broadcast) -> four uint32 arrays"""
    M0, M1, W0, W1, mask = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    c = [np.asarray(v, np.uint64) & np.uint64(mask) for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & mask, int(k1) & mask
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(mask), p1 >> np.uint64(32), p1 & np.uint64(mask)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & mask, (k1 + W1) & mask
    return [v.astype(np.uint32) for v in c]


def _f64_fn(name, x):
    x = np.ascontiguousarray(x, np.float64)
    out = np.empty_like(x)
    getattr(oracle_lib.load(), name)(x.ctypes.data, x.size, out.ctypes.data)
    return out


def glabc_exp(x):
    return _f64_fn("oracle_exp_v", x)


def glabc_log(x):
    return _f64_fn("oracle_log_v", x)


def uniform_f64(a, b):
    """glabc_uniform_f64 of two uint32 words"""
    a, b = np.ascontiguousarray(a, np.uint32), np.ascontiguousarray(b, np.uint32)
    u, upos, u64 = np.empty(a.size, np.float32), np.empty(a.size, np.float32), np.empty(a.size, np.float64)
    oracle_lib.load().oracle_uniforms_v(a.ctypes.data, b.ctypes.data, a.size, u.ctypes.data, upos.ctypes.data, u64.ctypes.data)
    return u64.reshape(a.shape)


def normal_pair(a, b):
    """glabc_normal_pair of two uint32 words -> (z0, z1) float32"""
    a, b = np.ascontiguousarray(a, np.uint32), np.ascontiguousarray(b, np.uint32)
    z0, z1 = np.empty(a.size, np.float32), np.empty(a.size, np.float32)
    oracle_lib.load().oracle_normal_pair_v(a.ctypes.data, b.ctypes.data, a.size, z0.ctypes.data, z1.ctypes.data)
    return z0.reshape(a.shape), z1.reshape(a.shape)


class MixtureRef:
    """A mixture given by its float64 constants (the fields of glabc_mixture)."""

    def __init__(self, loc, scale, inv_scale, log_weight, cum_weight, sum_log_scale, c0):
        self.loc, self.scale, self.inv_scale = (np.array(a, np.float64) for a in (loc, scale, inv_scale))
        self.log_weight, self.cum_weight, self.sum_log_scale = (np.array(a, np.float64) for a in (log_weight, cum_weight, sum_log_scale))
        self.c0 = float(c0)
        self.K, self.d = self.loc.shape

    @classmethod
    def from_descriptor(cls, m):
        K, d = m.n_modes, m.dim
        tab = lambda t: np.array([[t[k][q] for q in range(d)] for k in range(K)], np.float64)        # noqa: E731
        vec = lambda t: np.array([t[k] for k in range(K)], np.float64)                               # noqa: E731
        return cls(tab(m.loc), tab(m.scale), tab(m.inv_scale), vec(m.log_weight), vec(m.cum_weight), vec(m.sum_log_scale), m.c0)

    def log_prob(self, z):
        """z[n][d] float64 -> float64[n]"""
        z = np.asarray(z, np.float64).reshape(-1, self.d)
        t = np.empty((z.shape[0], self.K), np.float64)
        for k in range(self.K):
            e = (z - self.loc[k]) * self.inv_scale[k]
            S = rowsum_f64(e * e)
            t[:, k] = ((self.c0 + self.log_weight[k]) - 0.5 * S) - self.sum_log_scale[k]
        m = t.max(axis=1)
        m = np.where(np.isinf(m), 0.0, m)
        return m + glabc_log(rowsum_f64(glabc_exp(t - m[:, None])))

    def log_prob_f32(self, theta):
        """log_prob of float32 states: (float) log_prob((double) theta)"""
        return self.log_prob(np.asarray(theta, np.float32).astype(np.float64)).astype(np.float32)

    def mode(self, u):
        """the first k with u < cum_weight[k], else K - 1"""
        u = np.asarray(u, np.float64)
        mode = np.full(u.shape, self.K - 1, np.int64)
        for k in range(self.K - 1, -1, -1):
            mode = np.where(u < self.cum_weight[k], k, mode)
        return mode

    def draw(self, u, eps):
        """(mode uniforms [n], float32 normals [n][d]) -> (z float64 [n][d], log_p float64 [n], mode [n])"""
        k = self.mode(u)
        z = np.asarray(eps, np.float32).astype(np.float64) * self.scale[k] + self.loc[k]
        return z, self.log_prob(z), k

    def forward_rows(self, n, seed, row0):
        """glabc_mixture_forward: row id = row0 + r, counter (id lo, id hi, 0, b); the mode uniform from words 0-1 of block 0,
        the normals from words 2-3 of block 0, then blocks 1 and up"""
        ids = np.uint64(row0) + np.arange(n, dtype=np.uint64)
        lo, hi = (ids & np.uint64(0xFFFFFFFF)), (ids >> np.uint64(32))
        nb = (self.d + 2 + 3) // 4
        words = []
        for b in range(nb):
            words += philox4x32_10(lo, hi, 0, b, seed & 0xFFFFFFFF, seed >> 32)
        u = uniform_f64(words[0], words[1])
        eps = np.empty((n, 2 * ((self.d + 1) // 2)), np.float32)
        for i in range((self.d + 1) // 2):
            eps[:, 2 * i], eps[:, 2 * i + 1] = normal_pair(words[2 + 2 * i], words[3 + 2 * i])
        return self.draw(u, eps[:, :self.d])

    def candidates(self, seed, chain_ids, step, n_prop, y_dim):
        """forward inside a sampler for every candidate j < n_prop of the chains at iteration `step`: the mode uniform from the
        block at counter (chain lo, chain hi, step, SLOT_MIX + j), the normals the candidate's ordinary proposal normals.
        -> theta' float32 [n_prop][n][d], log q' float32 [n_prop][n]"""
        L = oracle_lib.load()
        chain_ids = np.asarray(chain_ids, np.uint64)
        n, d = len(chain_ids), self.d
        eps = np.empty((n_prop, n, d), np.float32)
        u2, r, z = np.empty(2, np.float32), np.empty(1, np.float64), np.empty(n_prop * (d + y_dim), np.float32)
        for i, cid in enumerate(chain_ids):
            L.oracle_step_draws(C.c_uint64(int(seed)), C.c_uint64(int(cid)), int(step), n_prop, d, y_dim, u2.ctypes.data, r.ctypes.data,
                                z.ctypes.data)
            eps[:, i, :] = z.reshape(n_prop, d + y_dim)[:, :d]
        lo, hi = (chain_ids & np.uint64(0xFFFFFFFF)), (chain_ids >> np.uint64(32))
        theta = np.empty((n_prop, n, d), np.float32)
        log_q = np.empty((n_prop, n), np.float32)
        for j in range(n_prop):
            w = philox4x32_10(lo, hi, step, SLOT_MIX + j, seed & 0xFFFFFFFF, seed >> 32)
            zz, lp, _ = self.draw(uniform_f64(w[0], w[1]), eps[j])
            theta[j], log_q[j] = zz.astype(np.float32), lp.astype(np.float32)
        return theta, log_q
