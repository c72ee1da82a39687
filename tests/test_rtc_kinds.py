"""Every kind of run-time compiled program at every launch entry point (csrc/glabc_rtc.hip), on the GPU.

One program of each of the five kinds -- sampler, mixture, draws, predictive, weighted predictive -- around a two-line simulator with
a discrepancy of its own, theta_dim = y_dim = noise_dim = 2, batch size 2, 64 chains or draws.  A program keeps its kernels in one
array indexed by its kind's slot enumeration and one packer of its kind, so the kind is what stands between an entry point and a
kernel of another argument block: each of the eight launch entry points takes its own kind (GLABC_OK, with the very arguments the
others are refused with -- the kind is their only defect) and answers every other kind with GLABC_ERR_KIND, every buffer it could
have written still holding its canary.  The two row kernels stand in a slot the program's table announces: glabc_rtc_simulate and
glabc_rtc_model_rows give the same bits on all five programs, and glabc_rtc_hooks the same three flags."""
import ctypes as C

import numpy as np
import pytest
import torch

from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import distribution, engine
from glabcmcmc_amd.compiled import CompiledModel
from glabcmcmc_amd.kernel_density import KernelDensity

pytestmark = pytest.mark.gpu

ERR_KIND = -3
D, N, BATCH, SEED, BINS = 2, 64, 2, 20240229, 7
KINDS = ("sampler", "mixture", "draws", "predictive", "weighted_predictive")
SOURCE = """
GLABC_SIMULATOR void glabc_user_simulate(const float* theta, const float* eps, float* y)
{
    y[0] = fabsf(theta[0]) + 0.25f * eps[0];
    y[1] = theta[0] * theta[1] + 0.5f * eps[1];
}
#define GLABC_USER_DISCREPANCY 1
GLABC_SIMULATOR float glabc_user_discrepancy(const float* y, const float* y_obs)
{
    return fabsf(y[0] - y_obs[0]) + 0.5f * fabsf(y[1] - y_obs[1]);
}
"""
CANARY = 0x7FC0BEEF                                               # a NaN with a payload of its own


@pytest.fixture(scope="module")
def programs(hip):
    src, out = SOURCE.encode(), {}

    def compiled(name, *args):
        handle, log = C.c_void_p(), C.create_string_buffer(1 << 14)
        assert getattr(hip, name)(*args, C.byref(handle), log, len(log)) == 0, log.value.decode()
        return handle

    out["sampler"] = compiled("glabc_rtc_compile", src, A.ALGO_GLMCMC, D, D, D, BATCH)
    out["mixture"] = compiled("glabc_rtc_compile_mix", src, A.ALGO_GLMCMC, D, D, D, BATCH)
    out["draws"] = compiled("glabc_rtc_compile_draws", src, D, D, D)
    out["predictive"] = compiled("glabc_rtc_compile_predictive", src, D, D, D)
    out["weighted_predictive"] = compiled("glabc_rtc_compile_weighted_predictive", src, D, D, D)
    assert tuple(out) == KINDS
    yield out
    for handle in out.values():
        hip.glabc_rtc_release(handle)


@pytest.fixture(scope="module")
def model():
    prior = distribution.DiagGaussian(D, torch.zeros(D), torch.zeros(D))
    return CompiledModel(theta_dim=D, y_dim=D, simulator_source=SOURCE, prior=prior, y_obs=[1.0, 0.5], epsilon=0.7).descriptor()


def canary(*shape, dtype=torch.float32):
    words = {torch.float32: torch.int32, torch.int32: torch.int32, torch.uint8: torch.uint8, torch.int64: torch.int64}[dtype]
    value = {torch.int32: CANARY, torch.uint8: 0xA5, torch.int64: (CANARY << 32) | CANARY}[words]
    return torch.full(shape, value, dtype=words, device="cuda").view(dtype)


def untouched(tensors):
    torch.cuda.synchronize()
    for t in tensors:
        fresh = canary(*t.shape, dtype=t.dtype)
        assert torch.equal(t.view(torch.uint8), fresh.view(torch.uint8))


class Calls:
    """The eight launch entry points with valid arguments of the programs' dimensions: call(program) -> (status, the device buffers the
    launch may write)"""

    def __init__(self, hip, m):
        self.hip, self.m = hip, m
        g = torch.Generator().manual_seed(SEED)
        self.theta0, self.y0 = torch.randn(N, D, generator=g), torch.randn(N, D, generator=g)
        self.local = distribution.DiagGaussian(D, torch.zeros(D), torch.log(torch.full((D,), 0.3))).descriptor()
        self.glob = distribution.DiagGaussian(D, torch.zeros(D), torch.zeros(D)).descriptor()
        self.mix = distribution.GaussianMixture(2, D, loc=np.array([[-1.0, 0.0], [1.0, 0.5]]), scale=np.ones((2, D)),
                                                weights=[1.0, 2.0]).descriptor()
        self.population = KernelDensity("silverman", device=torch.device("cuda", torch.cuda.current_device())).fit(
            torch.randn(48, D, generator=g).cuda())
        self.pop = self.population.descriptor()
        self.chol = (C.c_float * 3)(0.5, 0.1, 0.4)
        self.hist = torch.randn(1, D, N, generator=g).cuda()              # one history row of 64 chains; the 64 weighted draws
        self.w = (1.0 + torch.rand(N, generator=g)).cuda()
        self.lo, self.hi, self.thr = np.full(D + 1, -4.0), np.full(D + 1, 4.0), np.zeros(D + 1, np.float32)

    def _steps(self, entry, glob):
        def call(program):
            chains = engine.ChainBatch(self.theta0, self.y0, torch.device("cuda", torch.cuda.current_device()))
            state = [chains.theta, chains.y, chains.log_w, chains.flags, chains.n_moves]
            before = [t.clone() for t in state]
            hist = canary(1, D, N)
            r = A.Run()
            r.seed, r.step0, r.n_steps, r.batch_size, r.global_frequency = SEED, 1, 1, BATCH, 0.5
            r.history, r.hist_stride = hist.data_ptr(), N
            cs = chains.struct()
            rc = getattr(self.hip, entry)(program, C.byref(self.m), C.byref(self.local), C.byref(glob), C.byref(cs), C.byref(r), None)
            if rc != 0:                                                # a refused launch leaves the chains' state as it was
                torch.cuda.synchronize()
                for t, b in zip(state, before):
                    assert torch.equal(t.view(torch.uint8), b.view(torch.uint8))
            return rc, [hist]
        return call

    def _draws(self, entry):
        def call(program):
            theta, y, dis, lp, acc = canary(D, N), canary(D, N), canary(N), canary(N), canary(N, dtype=torch.uint8)
            m, pop = C.byref(self.m), C.byref(self.pop)
            if entry == "glabc_rtc_abc_draws":
                rc = self.hip.glabc_rtc_abc_draws(program, m, SEED, 0, None, N, N, theta.data_ptr(), y.data_ptr(), dis.data_ptr(), acc.data_ptr(),
                                                  None)
                return rc, [theta, y, dis, acc]
            if entry == "glabc_rtc_smc_draws":
                rc = self.hip.glabc_rtc_smc_draws(program, m, pop, SEED, 0, None, N, N, theta.data_ptr(), y.data_ptr(), dis.data_ptr(),
                                                  lp.data_ptr(), acc.data_ptr(), None)
            else:
                rc = self.hip.glabc_rtc_smc_draws_full(program, m, pop, self.chol, SEED, 0, None, N, N, theta.data_ptr(), y.data_ptr(),
                                                       dis.data_ptr(), lp.data_ptr(), acc.data_ptr(), None)
            return rc, [theta, y, dis, lp, acc]
        return call

    def _tables(self):
        return canary(D + 1, BINS + 3, dtype=torch.int64), canary(D + 1, 4, dtype=torch.int64), canary(D + 1, 2, dtype=torch.int32)

    def predictive_draws(self, program):
        y, dis = canary(1, D, N), canary(1, N)
        rc = self.hip.glabc_rtc_predictive_draws(program, C.byref(self.m), self.hist.data_ptr(), 1, D, N, N, SEED, 0, N, y.data_ptr(), N,
                                                 dis.data_ptr(), N, None)
        return rc, [y, dis]

    def predictive_counts(self, program):
        counts, tails, extremes = self._tables()
        rc = self.hip.glabc_rtc_predictive_counts(program, C.byref(self.m), self.hist.data_ptr(), 1, D, N, N, SEED, 0, N, BINS, self.lo.ctypes.data,
                                                  self.hi.ctypes.data, self.thr.ctypes.data, counts.data_ptr(), tails.data_ptr(),
                                                  extremes.data_ptr(), None)
        return rc, [counts, tails, extremes]

    def weighted_predictive_counts(self, program):
        counts, tails, extremes = self._tables()
        rc = self.hip.glabc_rtc_weighted_predictive_counts(program, C.byref(self.m), self.hist.data_ptr(), N, D, self.w.data_ptr(), N, 0.5, SEED, 0,
                                                           BINS, self.lo.ctypes.data, self.hi.ctypes.data, self.thr.ctypes.data,
                                                           counts.data_ptr(), tails.data_ptr(), extremes.data_ptr(), None)
        return rc, [counts, tails, extremes]

    def all(self):
        """entry point -> (the kind it launches, call)"""
        return {"glabc_rtc_steps": ("sampler", self._steps("glabc_rtc_steps", self.glob)),
                "glabc_rtc_mix_steps": ("mixture", self._steps("glabc_rtc_mix_steps", self.mix)),
                "glabc_rtc_abc_draws": ("draws", self._draws("glabc_rtc_abc_draws")),
                "glabc_rtc_smc_draws": ("draws", self._draws("glabc_rtc_smc_draws")),
                "glabc_rtc_smc_draws_full": ("draws", self._draws("glabc_rtc_smc_draws_full")),
                "glabc_rtc_predictive_draws": ("predictive", self.predictive_draws),
                "glabc_rtc_predictive_counts": ("predictive", self.predictive_counts),
                "glabc_rtc_weighted_predictive_counts": ("weighted_predictive", self.weighted_predictive_counts)}


def test_each_entry_point_takes_its_own_kind_and_refuses_every_other(hip, programs, model):
    for entry, (own, call) in Calls(hip, model).all().items():
        rc, written = call(programs[own])
        torch.cuda.synchronize()
        assert rc == 0, (entry, own, rc)                               # the arguments are valid: below, the kind is the only defect
        for t in written:                                              # ... and the launch ran: no buffer is all canary
            assert not torch.equal(t.view(torch.uint8), canary(*t.shape, dtype=t.dtype).view(torch.uint8)), entry
        for kind in KINDS:
            if kind != own:
                rc, written = call(programs[kind])
                assert rc == ERR_KIND, (entry, kind, rc)
                untouched(written)


def test_row_kernels_and_hooks_are_the_same_on_every_kind(hip, programs, model):
    g = torch.Generator().manual_seed(SEED + 1)
    theta, eps = torch.randn(N, D, generator=g).cuda(), torch.randn(N, D, generator=g).cuda()
    ys, rows, flags = [], [], []
    for kind in KINDS:
        p = programs[kind]
        y = canary(N, D)
        assert hip.glabc_rtc_simulate(p, theta.data_ptr(), eps.data_ptr(), N, y.data_ptr(), None) == 0, kind
        ys.append(y)
        for what in (A.RTC_DISCREPANCY, A.RTC_LOG_KERNEL):
            out = canary(N)
            assert hip.glabc_rtc_model_rows(p, C.byref(model), what, ys[0].data_ptr(), N, out.data_ptr(), None) == 0, (kind, what)
            rows.append(out)
        up, ud, uk = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
        assert hip.glabc_rtc_hooks(p, C.byref(up), C.byref(ud), C.byref(uk)) == 0
        flags.append((up.value, ud.value, uk.value))
    torch.cuda.synchronize()
    assert flags == [(0, 1, 0)] * len(KINDS)
    # the sampler program's rows are what the source says (float32, one rounding per operation, no contraction) ...
    t, e = theta.cpu().numpy(), eps.cpu().numpy()
    want = np.stack([np.abs(t[:, 0]) + np.float32(0.25) * e[:, 0], t[:, 0] * t[:, 1] + np.float32(0.5) * e[:, 1]], axis=1)
    assert np.array_equal(ys[0].cpu().numpy().view(np.uint32), want.astype(np.float32).view(np.uint32))
    yo = np.array([1.0, 0.5], np.float32)
    dis = np.abs(want[:, 0] - yo[0]) + np.float32(0.5) * np.abs(want[:, 1] - yo[1])
    assert np.array_equal(rows[0].cpu().numpy().view(np.uint32), dis.astype(np.float32).view(np.uint32))
    assert bool(torch.isfinite(rows[1]).all()) and bool((rows[1] != rows[0]).any())
    # ... and every other kind gives the same bits
    for k, kind in enumerate(KINDS):
        assert torch.equal(ys[k].view(torch.int32), ys[0].view(torch.int32)), kind
        assert torch.equal(rows[2 * k].view(torch.int32), rows[0].view(torch.int32)), kind
        assert torch.equal(rows[2 * k + 1].view(torch.int32), rows[1].view(torch.int32)), kind
