"""CompiledModel -- a user's simulator inside the fused kernel (run-time compilation, ``glabc_rtc_compile``).

The reference's Model is a Python object whose ``generate_samples`` may be anything (examples/Mixture.py:13-26).  Python
cannot run inside a GPU kernel, so such a Model goes through the split-phase path (``generic.py``, ~10^8.9 chain-steps/s).
If the simulator can be written as a few lines of C, ``CompiledModel`` compiles the library's own sampler code around it
(hiprtc, a second or so per configuration, cached) and the samplers run it at the speed of the built-in Models
(~10^10.3 chain-steps/s):

    SIM = '''
    GLABC_SIMULATOR void glabc_user_simulate(const float* theta, const float* eps, float* y)
    {   /* theta[GLABC_THETA_DIM], eps[GLABC_NOISE_DIM] standard normals -> y[GLABC_Y_DIM] */
        for (int j = 0; j < GLABC_Y_DIM; ++j) y[j] = fabsf(theta[j]) + 0.2236068f * eps[j];
    }'''
    model = CompiledModel(theta_dim=2, y_dim=2, simulator_source=SIM, prior=DiagGaussian(2, zeros, zeros),
                          y_obs=[1.5, 1.5], epsilon=0.05)
    MCMCRunner(model).run_glmcmc(...)

The rest of the Model defaults to what the reference's example uses: a ``DiagGaussian`` / ``Uniform`` prior, the Euclidean
discrepancy to ``y_obs`` and the Gaussian ABC kernel of width ``epsilon`` (examples/Mixture.py:28-45) -- and each of them can be
user source too: the same string may define, announced by a ``#define`` each,

    #define GLABC_USER_PRIOR 1
    GLABC_SIMULATOR float glabc_user_prior_log_prob(const float* theta) { ... }               /* Mixture.py:28-31 */
    #define GLABC_USER_DISCREPANCY 1
    GLABC_SIMULATOR float glabc_user_discrepancy(const float* y, const float* y_obs) { ... }  /* Mixture.py:33-36 */
    #define GLABC_USER_KERNEL 1
    GLABC_SIMULATOR float glabc_user_log_kernel(float dis, float scale) { ... }               /* Mixture.py:38-45 */

which the fused kernel then calls in place of the descriptor's forms (``prior`` stays a required argument: with a user prior it
only says where the self-check starts its chains).

GLMCMC with ``batch_size`` 1..16 runs a register kernel compiled for that batch size (``glabc_rtc_compile``); with 17..4096 it runs
the lane-group kernel of the built-in Models (8 to 64 lanes of a wavefront share a chain's proposals), compiled once per Model
for every such batch size (``glabc_rtc_compile_wide``).  Every program is checked against the split-phase path before it is
handed out -- the wide one once per batch size, at the lane count the library launches for it.  GLMCMC's ``path="auto"`` keeps a
Model with a user prior on the split-phase path above 16 proposals (only that path redraws the prior's ``7 log(1e-10)``
sentinel), and falls back to it with a warning where the wide program fails to compile or fails its check.  The object also
implements the full duck-typed protocol (``generate_samples`` through the compiled simulator on rows, ``prior_log_prob`` /
``discrepancy`` / ``calculate_log_kernel`` through the row-wise kernels), so it works with every sampler, the split-phase
path included.

A ``distribution.Gamma`` as the Model's prior and / or as the importance / global proposal runs fused too: the samplers then ask for
a program compiled with ``GLABC_RTC_GAMMA`` (``program(..., gamma=True)``, a program of its own in the cache), which holds the
Gamma kernels next to the generic ones, and its self-check runs them -- with the caller's proposal, positive start states.

A ``distribution.GaussianMixture`` as the importance / global proposal runs fused as well, at any ``theta_dim``: the samplers ask for
a mixture program (``program(..., mixture=True)``: ``glabc_rtc_compile_mix`` up to 16 proposals, ``glabc_rtc_compile_wide_mix`` once per
Model above), launched by ``glabc_rtc_mix_steps``.  Its self-check runs it against ``glabc_propose_mix`` -> the compiled row callbacks
-> ``glabc_select`` on the same Philox streams, with the caller's mixture.

``rejection`` and ``smc`` run fused on a ``CompiledModel`` as well: ``draws_program()`` compiles the two draw kernels of
``glabc_abc_draws`` / ``glabc_smc_draws`` around the source (``glabc_rtc_compile_draws``; a program of its own in the cache, no sampler
kernel in it) and checks them, bit for bit, against the composition of entry points that specifies a draw (include/glabc.h) before
it is handed out.  A user prior (``GLABC_USER_PRIOR``) and a Gamma prior have no draws program: theta is drawn from a DiagGaussian
or Uniform descriptor prior there.

``predictive`` runs fused on a ``CompiledModel`` too: ``predictive_program()`` compiles ``predictive_kernel`` of
``glabc_predictive_counts`` / ``glabc_predictive_draws`` around the source (``glabc_rtc_compile_predictive``; a program of its own in the
cache) and checks it, bit for bit, against the composition of entry points that specifies a predictive draw before it is handed
out.  Any prior will do, a user prior included: theta comes from the history.  ``predictive.check_weighted`` has a program of its
own again: ``weighted_predictive_program()`` compiles ``weighted_predictive_kernel`` of ``glabc_weighted_predictive_counts`` around
the source (``glabc_rtc_compile_weighted_predictive``) and holds its tables to integer sums of the quantised weights over the draws
of the predictive program before it is handed out.

Use + - * / fmaf sqrtf fabsf and the ``glabc_*`` functions of include/glabc_numerics.h (``glabc_expf``,
``glabc_logf``, ``glabc_sincos2pi`` ...) for results that a CPU build of the same source reproduces bit for bit.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _capi, distribution, engine
from .distribution import _fill, _launch_rowwise


class SimulatorCompileError(RuntimeError):
    pass


class SimulatorSelfCheckError(RuntimeError):
    pass


class CompiledModel:
    def __init__(self, theta_dim, y_dim, simulator_source, prior, y_obs, epsilon, noise_dim=None):
        self.theta_dim, self.y_dim = int(theta_dim), int(y_dim)
        self.noise_dim = int(y_dim if noise_dim is None else noise_dim)
        self.simulator_source = str(simulator_source)
        self.prior = prior
        self.y_obs = torch.as_tensor(y_obs, dtype=torch.float32).reshape(1, -1)
        if self.y_obs.shape[1] != self.y_dim:
            raise ValueError("y_obs has %d entries, y_dim is %d" % (self.y_obs.shape[1], self.y_dim))
        self.epsilon = epsilon
        self._programs = {}
        self._checked = set()
        self._failed = {}                                 # (algorithm, batch size) -> message of the failed self-check
        self._predictive_rows = 1                         # rows per item the predictive program was compiled with
        self._uncompiled = {}                             # the predictive program's key -> message of the compile that failed
        self.user_prior, self.user_discrepancy, self.user_kernel = (self._announces(m) for m in
                                                                    ("GLABC_USER_PRIOR", "GLABC_USER_DISCREPANCY", "GLABC_USER_KERNEL"))

    def _announces(self, macro):
        import re
        return re.search(r"define[ \t]+%s(?![A-Za-z0-9_])" % macro, self.simulator_source) is not None

    # ---- run-time compiled programs: one per (algorithm, batch size) up to 16, one wide program for GLMCMC above ---------
    WIDE = "wide"

    GAMMA = "gamma"

    MIXTURE = "mixture"

    def program(self, algo, batch_size=1, gamma=False, proposal=None, mixture=False):
        """gamma: the program with the Gamma kernels (GLABC_RTC_GAMMA) -- what a sampler asks for when the prior or its importance /
        global proposal (`proposal`: the object, for the self-check) is a Gamma.  A Model whose prior is a Gamma has no other.
        mixture: the program of the kernels' GaussianMixture variant (glabc_rtc_compile_mix / glabc_rtc_compile_wide_mix), launched by
        glabc_rtc_mix_steps -- what a sampler asks for when its importance / global proposal is a GaussianMixture.  Programs of their
        own in the cache, the wide one compiled once per Model; a Gamma prior has none (ValueError)."""
        if mixture:
            return self._mixture_program(int(algo), batch_size, proposal)
        algo = int(algo)
        n = 1 if algo == _capi.ALGO_GLOBALMCMC else int(batch_size)
        wide = algo == _capi.ALGO_GLMCMC and n > _capi.MAX_BATCH
        if wide and n > _capi.MAX_BATCH_WIDE:
            raise ValueError("batch_size %d: the fused kernels take 1..%d" % (n, _capi.MAX_BATCH_WIDE))
        gamma = bool(gamma) or self._gamma_prior()
        key = (algo, self.WIDE) if wide else (algo, n)   # the program
        check = (algo, n)                                # its self-check: once per batch size (the wide one serves many)
        if gamma:
            key, check = key + (self.GAMMA,), check + (self.GAMMA,)
        flags = _capi.RTC_GAMMA if gamma else 0
        if wide:
            compile_call = ("glabc_rtc_compile_wide_ex", lambda src: (src, self.theta_dim, self.y_dim, self.noise_dim, flags))
        else:
            compile_call = ("glabc_rtc_compile_ex", lambda src: (src, algo, self.theta_dim, self.y_dim, self.noise_dim, n, flags))
        # the wide program is one code object for all batch sizes above 16: the checks it passed at other batch sizes go with it
        siblings = (lambda k: k[0] == algo and k[1] > _capi.MAX_BATCH and len(k) == len(check)) if wide else None
        run_check = (lambda handle: self.self_check(algo, n, gamma=True, proposal=proposal)) if gamma else (lambda handle: self.self_check(algo, n))
        return self._cached_program(key, compile_call, run_check, check_key=check, check_reenters=True, siblings=siblings)

    def _cached_program(self, key, compile_call, check, check_key=None, check_reenters=False, remember_uncompiled=False, siblings=None):
        """The cache protocol of every program kind -> the handle under `key`, compiled once and self-checked before it is handed out.
        compile_call: (entry point, source -> its arguments before `out, log, log_size`), looked at only when there is something to
        compile; a status other than OK raises SimulatorCompileError with the compiler's log.  check(handle): the self-check, once per `check_key` (default: the key; the wide programs serve many batch
        sizes and are checked once for each), skipped under GLABC_RTC_SELF_CHECK=0.  A program that failed (or did not finish) its
        check must never be handed out: it is released, and a SimulatorSelfCheckError is remembered, so that every later call raises
        again instead of running a miscompiled kernel.
        check_reenters: the check comes back into program() for this very key (through the samplers), so the check key is marked
        before it runs and taken back if it fails; otherwise it is marked once the check has passed.
        remember_uncompiled: an ERR_ARG compile -- the source's own defect -- is remembered too, and the source not handed to hiprtc
        again (no device, GLABC_ERR_NO_DEVICE, may be there next time).
        siblings: of a failing wide program, which other passed checks go with it (a predicate on check keys)."""
        check_key = key if check_key is None else check_key
        if key in self._failed:
            raise SimulatorSelfCheckError(self._failed[key])
        if key in self._uncompiled:
            raise SimulatorCompileError(self._uncompiled[key])
        if key not in self._programs:
            name, arguments = compile_call
            handle = C.c_void_p()
            log = C.create_string_buffer(1 << 16)
            rc = getattr(_capi.lib(), name)(*arguments(self.simulator_source.encode()), C.byref(handle), log, len(log))
            if rc != _capi.OK:
                message = "%s failed (status %d):\n%s" % (name, rc, log.value.decode(errors="replace"))
                if remember_uncompiled and rc == _capi.ERR_ARG:
                    self._uncompiled[key] = message
                raise SimulatorCompileError(message)
            self._programs[key] = handle
        if check_key not in self._checked and os.environ.get("GLABC_RTC_SELF_CHECK", "1") != "0":
            if check_reenters:
                self._checked.add(check_key)
            try:
                check(self._programs[key])
                self._checked.add(check_key)
            except BaseException as exc:
                self._checked.discard(check_key)
                if siblings is not None:
                    self._checked -= {k for k in self._checked if siblings(k)}
                handle = self._programs.pop(key, None)
                if handle is not None:
                    _capi.lib().glabc_rtc_release(handle)
                if isinstance(exc, SimulatorSelfCheckError):
                    self._failed[key] = str(exc)
                raise
        return self._programs[key]

    def _source_and_dimensions(self, src):
        """the arguments of the compile entry points that take no more than these"""
        return src, self.theta_dim, self.y_dim, self.noise_dim

    def _mixture_program(self, algo, batch_size, proposal=None):
        n = 1 if algo == _capi.ALGO_GLOBALMCMC else int(batch_size)
        wide = algo == _capi.ALGO_GLMCMC and n > _capi.MAX_BATCH
        if wide and n > _capi.MAX_BATCH_WIDE:
            raise ValueError("batch_size %d: the fused kernels take 1..%d" % (n, _capi.MAX_BATCH_WIDE))
        if self._gamma_prior():
            raise ValueError("the mixture variant knows no Gamma prior")
        key = (algo, self.WIDE if wide else n, self.MIXTURE)
        check = (algo, n, self.MIXTURE)                  # the self-check: once per batch size, as for the other programs
        if wide:
            compile_call = ("glabc_rtc_compile_wide_mix", self._source_and_dimensions)
        else:
            compile_call = ("glabc_rtc_compile_mix", lambda src: (src, algo, self.theta_dim, self.y_dim, self.noise_dim, n))
        siblings = (lambda k: k[0] == algo and k[-1] == self.MIXTURE and k[1] > _capi.MAX_BATCH) if wide else None
        return self._cached_program(key, compile_call, lambda handle: self.self_check_mixture(algo, n, proposal), check_key=check,
                                    check_reenters=True, siblings=siblings)

    def self_check_mixture(self, algo, batch_size=1, proposal=None, n_chains=512, steps=4, seed=20240229):
        """self_check for a mixture program: glabc_rtc_mix_steps against the split-phase iteration glabc_propose_mix -> this Model's
        compiled row callbacks -> glabc_select on the same Philox streams (path="generic", kernel_stream=True), bit for bit, with the
        caller's mixture (`proposal`), else three modes around the prior's location."""
        from .GlobalMCMC import GlobalMCMC
        from .GLMCMC import GLMCMC
        dev = engine.require_device(None)
        g = torch.Generator().manual_seed(seed)
        d = self.theta_dim
        pd = self.prior.descriptor()
        loc = torch.tensor([pd.p0[j] for j in range(d)], dtype=torch.float64)
        scale = torch.tensor([pd.p2[j] for j in range(d)], dtype=torch.float64)
        if pd.kind == _capi.DIST_UNIFORM:                             # p0 = low, p2 = high - low
            loc, scale = loc + 0.5 * scale, scale / 4.0
        mix = proposal
        if mix is None:
            shift = torch.tensor([-1.0, 0.0, 1.0], dtype=torch.float64).view(3, 1)
            mix = distribution.GaussianMixture(3, d, loc=(loc.view(1, d) + shift * scale.view(1, d)).numpy(),
                                               scale=(0.6 * scale).view(1, d).expand(3, d).numpy(), weights=[1.0, 2.0, 1.0])
        theta0 = (loc + scale * torch.randn(n_chains, d, generator=g, dtype=torch.float64)).to(torch.float32)
        local = distribution.DiagGaussian(d, torch.zeros(d), torch.log(0.3 * scale.to(torch.float32)))
        y0 = self.simulate_from_noise(theta0, torch.randn(n_chains, self.noise_dim, generator=g)).cpu()
        out = []
        for path, kw in (("fused", {}), ("generic", dict(sentinel_redraw=False, graph=False, kernel_stream=True))):
            if algo == _capi.ALGO_GLMCMC:
                r = GLMCMC(self, steps + 1, theta0, y0, local, None, 0.5, mix, batch_size, seed=seed, device=dev, verbose=False,
                           path=path, **kw)
            else:
                r = GlobalMCMC(self, steps + 1, theta0, y0, mix, None, 0.5, local, seed=seed, device=dev, verbose=False, path=path,
                               **kw)
            out.append(r.contiguous().view(torch.int32))
        if not torch.equal(out[0], out[1]):
            bad = int((out[0] != out[1]).any(dim=-1).any(dim=0).sum()) if out[0].dim() == 3 else -1
            raise SimulatorSelfCheckError(
                "the run-time compiled mixture kernel (algorithm %d, batch size %d) disagrees with the split-phase path on %d of %d "
                "chains after %d iterations: refusing to sample with it (use path='generic', and please report the "
                "simulator source)" % (algo, batch_size, bad, n_chains, steps))
        return True

    # ---- the draws program: abc_draws_kernel, smc_draws_kernel and its full-covariance twin around the source (rejection.py, smc.py) --------------------
    DRAWS = "draws"

    def draws_refusal(self):
        """why this Model has no draws program (a sentence), or None"""
        if self.user_prior:
            return "the source announces GLABC_USER_PRIOR: the draw kernels draw theta from a descriptor prior"
        try:
            kind = self.prior.descriptor().kind
        except (AttributeError, NotImplementedError, ValueError):
            return "the prior %r has no descriptor()" % (self.prior,)
        if kind not in (_capi.DIST_DIAG_GAUSS, _capi.DIST_UNIFORM):
            return "the prior is neither DiagGaussian nor Uniform"
        return None

    def draws_program(self):
        """The handle of the draws program (glabc_rtc_compile_draws), compiled once and self-checked (self_check_draws) before it is
        handed out; a failed check raises SimulatorSelfCheckError, releases the program and is remembered."""
        reason = self.draws_refusal()
        if reason is not None:
            raise ValueError("no draws program for this Model: " + reason)
        key = (self.DRAWS,)
        return self._cached_program(key, ("glabc_rtc_compile_draws", self._source_and_dimensions), self.self_check_draws)

    def composed_draws(self, handle, desc, seed, row0, n, population=None, chol=None):
        """Draws row0 .. row0 + n - 1 as include/glabc.h specifies them, from the entry points a draw is composed of: theta from
        glabc_dist_forward of the prior (glabc_kde_sample of `population`; with the packed factor `chol`: glabc_kde_sample_full), eps from glabc_dist_forward of a standard DiagGaussian
        under seed ^ GLABC_ABC_NOISE_KEY, y from glabc_rtc_simulate, the distance from glabc_rtc_model_rows / glabc_model_discrepancy,
        log_prior from glabc_model_prior_log_prob (+inf rule applied) -> {name: device tensor}, theta (n, D) and y (n, YD)"""
        lib, dev = _capi.lib(), engine.require_device(None)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        z = torch.empty(self.theta_dim, n, dtype=torch.float32, device=dev)
        lq = torch.empty(n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            if population is None:
                _capi.check(lib.glabc_dist_forward(C.byref(desc.prior), n, seed, row0, z.data_ptr(), lq.data_ptr(), stream), "glabc_dist_forward")
            elif chol is None:
                _capi.check(lib.glabc_kde_sample(C.byref(population.descriptor()), n, seed, row0, z.data_ptr(), stream), "glabc_kde_sample")
            else:
                _capi.check(lib.glabc_kde_sample_full(C.byref(population.descriptor()), chol, n, seed, row0, z.data_ptr(), stream),
                            "glabc_kde_sample_full")
            theta = z.t().contiguous()
            e = torch.empty(self.noise_dim, n, dtype=torch.float32, device=dev)
            _capi.check(lib.glabc_dist_forward(C.byref(desc.noise), n, seed ^ _capi.ABC_NOISE_KEY, row0, e.data_ptr(), lq.data_ptr(), stream),
                        "glabc_dist_forward")
            eps = e.t().contiguous()
            y = torch.empty(n, self.y_dim, dtype=torch.float32, device=dev)
            _capi.check(lib.glabc_rtc_simulate(handle, theta.data_ptr(), eps.data_ptr(), n, y.data_ptr(), stream), "glabc_rtc_simulate")
            dis = torch.empty(n, dtype=torch.float32, device=dev)
            if self.user_discrepancy:
                _capi.check(lib.glabc_rtc_model_rows(handle, C.byref(desc), _capi.RTC_DISCREPANCY, y.data_ptr(), n, dis.data_ptr(), stream),
                            "glabc_rtc_model_rows")
            else:
                _capi.check(lib.glabc_model_discrepancy(C.byref(desc), y.data_ptr(), n, dis.data_ptr(), stream), "glabc_model_discrepancy")
            out = {"theta": theta, "y": y, "distance": dis}
            if population is not None:
                lp = torch.empty(n, dtype=torch.float32, device=dev)
                _capi.check(lib.glabc_model_prior_log_prob(C.byref(desc), theta.data_ptr(), n, lp.data_ptr(), stream),
                            "glabc_model_prior_log_prob")
                out["log_prior"] = lp
                out["distance"] = torch.where(lp == -float("inf"), torch.full_like(dis, float("inf")), dis)
        return out

    def composed_accept(self, desc, seed, ids, dis):
        """The acceptance of include/glabc.h for the descriptor's kernel, from the library's own numerics on the device
        (glabc_selftest_numerics: Philox, glabc_expf) and IEEE float32 arithmetic in NumPy: u < exp(-(0.5 (e e))), e = (dis - 0) / scale
        -> uint8 host array.  `ids`, `dis`: host arrays."""
        lib, dev = _capi.lib(), engine.require_device(None)
        n = len(ids)
        key = (seed ^ _capi.ABC_ACCEPT_KEY) & 0xFFFFFFFFFFFFFFFF
        ctr = np.zeros((n, 6), np.uint32)
        ids = np.asarray(ids, np.uint64)
        ctr[:, 0], ctr[:, 1] = (ids & np.uint64(0xFFFFFFFF)).astype(np.uint32), (ids >> np.uint64(32)).astype(np.uint32)
        ctr[:, 4], ctr[:, 5] = key & 0xFFFFFFFF, key >> 32
        with np.errstate(all="ignore"):
            e = (np.asarray(dis, np.float32) - np.float32(0.0)) / np.float32(desc.kern_scale)
            arg = -(np.float32(0.5) * (e * e))
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        with torch.cuda.device(dev):
            c = torch.from_numpy(ctr.view(np.int32)).to(dev)
            w = torch.empty(n, 4, dtype=torch.int32, device=dev)
            _capi.check(lib.glabc_selftest_numerics(6, c.data_ptr(), w.data_ptr(), n, stream), "glabc_selftest_numerics")
            a = torch.from_numpy(np.ascontiguousarray(arg, np.float32)).to(dev)
            p = torch.empty(n, dtype=torch.float32, device=dev)
            _capi.check(lib.glabc_selftest_numerics(0, a.data_ptr(), p.data_ptr(), n, stream), "glabc_selftest_numerics")
        w0 = w[:, 0].cpu().numpy().view(np.uint32)
        u = (w0 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        return (u < p.cpu().numpy()).astype(np.uint8)

    def self_check_draws(self, handle, seed=20240229):
        """The three draw kernels of a freshly compiled draws program against the composition that specifies a draw (composed_draws),
        bit for bit: 320 draws in three runs of consecutive ids -- from 0, across 2^32 and above 2^40 --, listed out of order; theta,
        y, distance (and log_prior) together, then each output alone; the SMC kernel from a population of 48 prior draws, and its full-covariance twin from the same
        population with a factor that is not diagonal (composition: glabc_kde_sample_full -> glabc_rtc_simulate -> ...).  The
        acceptance byte is compared with composed_accept where the kernel is the descriptor's; a user kernel (GLABC_USER_KERNEL) has
        no entry point that evaluates it at a given distance, so its byte is only held to what must be: the same alone as with the
        other outputs, and 0 where the distance is NaN or +inf.  Runs once per Model (a few ms); GLABC_RTC_SELF_CHECK=0 skips it."""
        from .kernel_density import KernelDensity
        lib, dev = _capi.lib(), engine.require_device(None)
        desc = self.descriptor()
        runs = [(0, 128), (2 ** 32 - 64, 128), (2 ** 40 + 5, 64)]
        ids = np.concatenate([np.arange(a, a + k, dtype=np.int64) for a, k in runs])
        order = np.random.default_rng(seed).permutation(ids.size)
        ids_dev = torch.from_numpy(ids[order]).to(dev)
        n = ids.size
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        # the population of the SMC kernel: 48 draws of the prior, Silverman's bandwidth
        z = torch.empty(self.theta_dim, 48, dtype=torch.float32, device=dev)
        lq = torch.empty(48, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            _capi.check(lib.glabc_dist_forward(C.byref(desc.prior), 48, seed + 1, 0, z.data_ptr(), lq.data_ptr(), stream), "glabc_dist_forward")
        population = KernelDensity("silverman", device=dev).fit(z.t().contiguous())
        # the factor of the full-covariance kernel: the bandwidths on the diagonal, +-0.3 of them below it
        D = self.theta_dim
        bw = [float(v) for v in population.bandwidth.cpu()]
        chol = (C.c_float * (D * (D + 1) // 2))(*[bw[d] * (1.0 if e == d else 0.3 * (-1.0) ** (d + e)) for d in range(D) for e in range(d + 1)])

        def fused(pop, want, chol=None):
            shapes = {"theta": (self.theta_dim, n), "y": (self.y_dim, n), "distance": (n,), "log_prior": (n,), "accept": (n,)}
            out = {k: torch.empty(shapes[k], dtype=torch.uint8 if k == "accept" else torch.float32, device=dev) for k in want}
            ptr = lambda k: out[k].data_ptr() if k in out else None          # noqa: E731
            with torch.cuda.device(dev):
                if pop is None:
                    _capi.check(lib.glabc_rtc_abc_draws(handle, C.byref(desc), seed, 0, ids_dev.data_ptr(), n, n, ptr("theta"), ptr("y"),
                                                        ptr("distance"), ptr("accept"), stream), "glabc_rtc_abc_draws")
                elif chol is None:
                    _capi.check(lib.glabc_rtc_smc_draws(handle, C.byref(desc), C.byref(pop.descriptor()), seed, 0, ids_dev.data_ptr(), n, n,
                                                        ptr("theta"), ptr("y"), ptr("distance"), ptr("log_prior"), ptr("accept"), stream),
                                "glabc_rtc_smc_draws")
                else:
                    _capi.check(lib.glabc_rtc_smc_draws_full(handle, C.byref(desc), C.byref(pop.descriptor()), chol, seed, 0, ids_dev.data_ptr(),
                                                             n, n, ptr("theta"), ptr("y"), ptr("distance"), ptr("log_prior"), ptr("accept"),
                                                             stream), "glabc_rtc_smc_draws_full")
            return {k: (v.t().contiguous() if k in ("theta", "y") else v).cpu().numpy() for k, v in out.items()}

        def refuse(kernel, name, detail=""):
            raise SimulatorSelfCheckError(
                "the run-time compiled %s disagrees with the composition of entry points that specifies a draw in `%s`%s: refusing to "
                "draw with it (use path='generic', and please report the simulator source)" % (kernel, name, detail))

        for pop, L, kernel in ((None, None, "abc_draws_kernel"), (population, None, "smc_draws_kernel"),
                               (population, chol, "smc_draws_kernel (full covariance)")):
            names = ("theta", "y", "distance") + (("log_prior",) if pop is not None else ())
            parts = [self.composed_draws(handle, desc, seed, a, k, pop, L) for a, k in runs]
            want = {k: torch.cat([p[k] for p in parts]).cpu().numpy()[order] for k in names}
            got = fused(pop, names + ("accept",), L)
            for k in names:
                if not np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)):
                    refuse(kernel, k, " (%d of %d draws)" % (int((got[k].view(np.uint32) != want[k].view(np.uint32)).reshape(n, -1).any(axis=1).sum()), n))
            if self.user_kernel:
                if got["accept"][~np.isfinite(want["distance"])].any() or not np.isin(got["accept"], (0, 1)).all():
                    refuse(kernel, "accept", " (a draw without a finite distance was accepted)")
            elif not np.array_equal(got["accept"], self.composed_accept(desc, seed, ids[order], want["distance"])):
                refuse(kernel, "accept")
            for k in names + ("accept",):                               # each output alone: the scalar branches around the NULL ones
                alone = fused(pop, (k,), L)[k]
                if not np.array_equal(alone.view(np.uint8), got[k].view(np.uint8)):
                    refuse(kernel, k, " asked for alone")
        return True

    # ---- the predictive program: predictive_kernel around the source (predictive.py) -----------------------------------------
    PREDICTIVE = "predictive"

    @staticmethod
    def predictive_rows():
        """rows per item of a predictive program compiled now: csrc/glabc_rtc_tables.h rtc_predictive_rows restated
        (RTC_PRED_ROWS = 1; GLABC_RTC_PRED_ROWS=1..16 in the environment forces another, any other value is ignored)"""
        try:
            rows = int(os.environ.get("GLABC_RTC_PRED_ROWS", "1"))
        except ValueError:
            return 1
        return rows if 1 <= rows <= 16 else 1

    def predictive_program(self):
        """The handle of the predictive program (glabc_rtc_compile_predictive), compiled once and self-checked
        (self_check_predictive) before it is handed out; a failed check raises SimulatorSelfCheckError, releases the program and is
        remembered.  Any prior will do: theta comes from the history."""
        key = (self.PREDICTIVE,)
        if key not in self._programs:
            self._predictive_rows = self.predictive_rows()               # what a compile now takes
        return self._cached_program(key, ("glabc_rtc_compile_predictive", self._source_and_dimensions), lambda handle: self.self_check_predictive(handle, rows=self._predictive_rows),
                                    remember_uncompiled=True)

    def composed_predictive(self, handle, desc, hist, seed, id0, id_step):
        """The predictive draws of the chain-major device history `hist` (T, D, C) as include/glabc.h specifies them, from the entry
        points a draw is composed of: per row t, eps from glabc_dist_forward of a standard DiagGaussian under seed ^
        GLABC_PREDICTIVE_KEY at row0 = id0 + t id_step, y from glabc_rtc_simulate, the distance from glabc_rtc_model_rows /
        glabc_model_discrepancy -> (y (T, YD, C), distance (T, C)) device tensors"""
        from .predictive import PREDICTIVE_KEY
        lib, dev = _capi.lib(), hist.device
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        n_rows, _, n = hist.shape
        key = (seed ^ PREDICTIVE_KEY) & 0xFFFFFFFFFFFFFFFF
        ys, ds = [], []
        with torch.cuda.device(dev):
            for t in range(n_rows):
                theta = hist[t].t().contiguous()
                e = torch.empty(self.noise_dim, n, dtype=torch.float32, device=dev)
                lq = torch.empty(n, dtype=torch.float32, device=dev)
                _capi.check(lib.glabc_dist_forward(C.byref(desc.noise), n, key, id0 + t * id_step, e.data_ptr(), lq.data_ptr(), stream),
                            "glabc_dist_forward")
                eps = e.t().contiguous()
                y = torch.empty(n, self.y_dim, dtype=torch.float32, device=dev)
                _capi.check(lib.glabc_rtc_simulate(handle, theta.data_ptr(), eps.data_ptr(), n, y.data_ptr(), stream), "glabc_rtc_simulate")
                dis = torch.empty(n, dtype=torch.float32, device=dev)
                if self.user_discrepancy:
                    _capi.check(lib.glabc_rtc_model_rows(handle, C.byref(desc), _capi.RTC_DISCREPANCY, y.data_ptr(), n, dis.data_ptr(), stream),
                                "glabc_rtc_model_rows")
                else:
                    _capi.check(lib.glabc_model_discrepancy(C.byref(desc), y.data_ptr(), n, dis.data_ptr(), stream), "glabc_model_discrepancy")
                ys.append(y.t())
                ds.append(dis)
        return torch.stack(ys).contiguous(), torch.stack(ds).contiguous()

    def self_check_predictive(self, handle, seed=20240229, rows=None):
        """predictive_kernel of a freshly compiled predictive program against the composition that specifies a draw
        (composed_predictive), bit for bit (a NaN matching a NaN): 65 chains x 2 R + 1 rows (R the kernel's rows per item: a partial
        segment and a partial item), a stride that is no multiple of 4, ids that cross 2^32 inside the call and a second run past 2^40
        with id_step > n_chains; theta about 1 with a spread of 0.5 in every coordinate, whatever the prior, which is never evaluated;
        y and the distance together, then each alone; counts, tails and extremes -- together, then each table
        alone -- against the same bin arithmetic (predictive._torch_tables, glabc_key_counts' key) on the composed draws, as equal
        integers.  Runs once per Model (a few ms); GLABC_RTC_SELF_CHECK=0 skips it."""
        from . import predictive
        lib, dev = _capi.lib(), engine.require_device(None)
        desc = self.descriptor()
        d, yd, k = self.theta_dim, self.y_dim, self.y_dim + 1
        rows = self.predictive_rows() if rows is None else int(rows)
        n, n_rows, stride = 65, 2 * rows + 1, 65 + 17
        g = torch.Generator().manual_seed(seed)
        theta = (1.0 + 0.5 * torch.randn(n_rows, d, n, generator=g, dtype=torch.float64)).to(torch.float32)
        buf = torch.full((n_rows, d, stride), float("nan"), dtype=torch.float32)
        buf[:, :, :n] = theta
        buf = buf.to(dev)
        hist = buf[:, :, :n]
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def refuse(name, detail=""):
            raise SimulatorSelfCheckError(
                "the run-time compiled predictive_kernel disagrees with the composition of entry points that specifies a predictive draw "
                "in `%s`%s: refusing to check with it (use path='generic', and please report the simulator source)" % (name, detail))

        def same(a, b):
            return bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())

        def draws(id0, id_step, want):
            y = torch.empty(n_rows, yd, n + 3, dtype=torch.float32, device=dev) if "y" in want else None
            dis = torch.empty(n_rows, n + 1, dtype=torch.float32, device=dev) if "distance" in want else None
            with torch.cuda.device(dev):
                _capi.check(lib.glabc_rtc_predictive_draws(handle, C.byref(desc), buf.data_ptr(), n_rows, d, n, stride, seed, id0, id_step,
                                                           None if y is None else y.data_ptr(), n + 3, None if dis is None else dis.data_ptr(),
                                                           n + 1, stream), "glabc_rtc_predictive_draws")
            return (None if y is None else y[:, :, :n]), (None if dis is None else dis[:, :n])

        def tables(id0, id_step, bins, lim, thr, want):
            counts = torch.zeros(k, bins + 3, dtype=torch.int64, device=dev) if "counts" in want else None
            tails = torch.zeros(k, 4, dtype=torch.int64, device=dev) if "tails" in want else None
            extremes = (torch.from_numpy(np.array([predictive.KEY_NONE] * k, np.uint32).view(np.int32)).to(dev)
                        if "extremes" in want else None)
            lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
            ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
            with torch.cuda.device(dev):
                _capi.check(lib.glabc_rtc_predictive_counts(
                    handle, C.byref(desc), buf.data_ptr(), n_rows, d, n, stride, seed, id0, id_step, bins,
                    lo.ctypes.data if counts is not None else None, hi.ctypes.data if counts is not None else None,
                    thr.ctypes.data if tails is not None else None, ptr(counts), ptr(tails), ptr(extremes), stream),
                    "glabc_rtc_predictive_counts")
            out = {}
            if counts is not None:
                out["counts"] = counts.cpu().numpy().view(np.uint64)
            if tails is not None:
                out["tails"] = tails.cpu().numpy().view(np.uint64)
            if extremes is not None:
                out["extremes"] = extremes.cpu().numpy().view(np.uint32)
            return out

        for id0, id_step in ((2 ** 32 - 40, n), (2 ** 40 + 5, n + 7)):
            where = " (id0 %d, id_step %d)" % (id0, id_step)
            want_y, want_dis = self.composed_predictive(handle, desc, hist, seed, id0, id_step)
            y, dis = draws(id0, id_step, ("y", "distance"))
            if not same(y, want_y):
                refuse("y", where)
            if not same(dis, want_dis):
                refuse("distance", where)
            if not same(draws(id0, id_step, ("y",))[0], want_y):
                refuse("y", " asked for alone" + where)
            if not same(draws(id0, id_step, ("distance",))[1], want_dis):
                refuse("distance", " asked for alone" + where)
            # the tables of the composed draws: N x K statistics, the bins over a range with values on both sides, thresholds at a drawn value
            stats = torch.cat([want_y.permute(0, 2, 1).reshape(-1, yd), want_dis.reshape(-1, 1)], dim=1)
            host = stats.cpu().numpy()
            lim, thr = np.empty((k, 2)), np.empty(k, np.float32)
            for j in range(k):
                v = np.sort(host[:, j][np.isfinite(host[:, j])])
                if v.size == 0:
                    lim[j], thr[j] = (0.0, 1.0), 0.0
                else:
                    lim[j], thr[j] = (float(v[v.size // 10]), float(v[9 * v.size // 10])), v[v.size // 2]
                if not lim[j, 0] < lim[j, 1]:
                    lim[j] = lim[j, 0] - 0.5, lim[j, 0] + 0.5
            bins = 7
            ref = dict(zip(("counts", "tails"), predictive._torch_tables(stats, bins, lim, thr)))
            ref["extremes"] = np.array([predictive.KEY_NONE] * k, np.uint32)
            for j in range(k):
                v = host[:, j][~np.isnan(host[:, j])]
                if v.size:                                             # include/glabc.h glabc_key_counts: -0 is +0, order-preserving
                    u = np.where(v == 0, np.float32(0.0), v).astype(np.float32).view(np.uint32)
                    keys = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
                    ref["extremes"][j] = keys.min(), keys.max()
            got = tables(id0, id_step, bins, lim, thr, ("counts", "tails", "extremes"))
            for name in ("counts", "tails", "extremes"):
                if not np.array_equal(got[name], ref[name]):
                    refuse(name, where)
                if not np.array_equal(tables(id0, id_step, bins, lim, thr, (name,))[name], ref[name]):
                    refuse(name, " asked for alone" + where)
        return True

    # ---- the weighted predictive program: weighted_predictive_kernel around the source (predictive.check_weighted) ---------------
    WEIGHTED_PREDICTIVE = "weighted_predictive"

    def weighted_predictive_program(self):
        """The handle of the weighted predictive program (glabc_rtc_compile_weighted_predictive; a program of its own in the cache),
        compiled once and self-checked (self_check_weighted_predictive) before it is handed out; a failed check raises
        SimulatorSelfCheckError, releases the program and is remembered.  Any prior will do: theta comes from the draws."""
        key = (self.WEIGHTED_PREDICTIVE,)
        return self._cached_program(key, ("glabc_rtc_compile_weighted_predictive", self._source_and_dimensions),
                                    self.self_check_weighted_predictive, remember_uncompiled=True)

    def self_check_weighted_predictive(self, handle, seed=20240229):
        """weighted_predictive_kernel of a freshly compiled weighted predictive program against integer sums of the multiplicity m over
        the draws that glabc_rtc_predictive_draws of this Model's predictive program (itself checked against the composition that
        specifies a draw) makes for the same ids: 65 + 64 + 1 draws behind a stride that is no multiple of 4, NaN in the padding and
        behind the last weight; ids that cross 2^32 inside the call and a second run past 2^40; under the scale 0.5, ordinary weights,
        an exact 0 on a draw whose theta is NaN, a tie (w scale = 2.5, counted twice) and two draws of multiplicity 2^31, which the
        second table of every run (one bin over the whole range, every threshold +inf) holds in one bin and one tail, where 32-bit
        counters would wrap.  counts, tails and extremes -- together, then each table alone -- against predictive._torch_tables' bin
        arithmetic with m for 1 (predictive._torch_weighted_tables) and glabc_key_counts' key, as equal integers.  Runs once per Model
        (a few ms); GLABC_RTC_SELF_CHECK=0 skips it."""
        from . import predictive, weighted
        lib, dev = _capi.lib(), engine.require_device(None)
        desc = self.descriptor()
        reference = self.predictive_program()
        d, yd, k = self.theta_dim, self.y_dim, self.y_dim + 1
        n, stride, scale = 65 + 64 + 1, 65 + 64 + 1 + 17, 0.5
        g = torch.Generator().manual_seed(seed)
        theta = (1.0 + 0.5 * torch.randn(d, n, generator=g, dtype=torch.float64)).to(torch.float32)
        w = (1.0 + 15.0 * torch.rand(n, generator=g, dtype=torch.float64)).to(torch.float32)
        w[3], theta[:, 3] = 0.0, float("nan")             # no weight: skipped whatever theta holds
        w[7] = 5.0                                        # w scale = 2.5: a tie, to even
        w[20] = w[101] = 2.0 ** 32                        # m = 2^31 each
        buf = torch.full((d, stride), float("nan"), dtype=torch.float32)
        buf[:, :n] = theta
        buf = buf.to(dev)
        wbuf = torch.full((n + 5,), float("nan"), dtype=torch.float32)
        wbuf[:n] = w
        wbuf = wbuf.to(dev)
        m = weighted._multiplicity(wbuf[:n], scale)
        if [int(m[3]), int(m[7]), int(m[20]), int(m[101])] != [0, 2, 2 ** 31, 2 ** 31]:
            raise SimulatorSelfCheckError("the quantised weights of the self-check are not what include/glabc.h specifies")
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def refuse(name, detail=""):
            raise SimulatorSelfCheckError(
                "the run-time compiled weighted_predictive_kernel disagrees with the weighted sums over the draws of the predictive "
                "program in `%s`%s: refusing to check with it (use path='generic', and please report the simulator source)" % (name, detail))

        def tables(id0, bins, lim, thr, want):
            counts = torch.zeros(k, bins + 3, dtype=torch.int64, device=dev) if "counts" in want else None
            tails = torch.zeros(k, 4, dtype=torch.int64, device=dev) if "tails" in want else None
            extremes = (torch.from_numpy(np.array([predictive.KEY_NONE] * k, np.uint32).view(np.int32)).to(dev)
                        if "extremes" in want else None)
            lo, hi = np.ascontiguousarray(lim[:, 0]), np.ascontiguousarray(lim[:, 1])
            ptr = lambda t: None if t is None else t.data_ptr()          # noqa: E731
            with torch.cuda.device(dev):
                _capi.check(lib.glabc_rtc_weighted_predictive_counts(
                    handle, C.byref(desc), buf.data_ptr(), stride, d, wbuf.data_ptr(), n, scale, seed, id0, bins,
                    lo.ctypes.data if counts is not None else None, hi.ctypes.data if counts is not None else None,
                    thr.ctypes.data if tails is not None else None, ptr(counts), ptr(tails), ptr(extremes), stream),
                    "glabc_rtc_weighted_predictive_counts")
            out = {}
            if counts is not None:
                out["counts"] = counts.cpu().numpy().view(np.uint64)
            if tails is not None:
                out["tails"] = tails.cpu().numpy().view(np.uint64)
            if extremes is not None:
                out["extremes"] = extremes.cpu().numpy().view(np.uint32)
            return out

        for id0 in (2 ** 32 - 40, 2 ** 40 + 5):
            y = torch.empty(1, yd, n, dtype=torch.float32, device=dev)
            dis = torch.empty(1, n, dtype=torch.float32, device=dev)
            with torch.cuda.device(dev):
                _capi.check(lib.glabc_rtc_predictive_draws(reference, C.byref(desc), buf.data_ptr(), 1, d, n, stride, seed, id0, n,
                                                           y.data_ptr(), n, dis.data_ptr(), n, stream), "glabc_rtc_predictive_draws")
            stats = torch.cat([y[0].t(), dis[0].reshape(-1, 1)], dim=1)
            host, mult = stats.cpu().numpy(), m.cpu().numpy()
            lim, thr, whole = np.empty((k, 2)), np.empty(k, np.float32), np.empty((k, 2))
            extremes = np.array([predictive.KEY_NONE] * k, np.uint32)
            for j in range(k):
                counted = host[:, j][mult > 0]
                v = np.sort(counted[np.isfinite(counted)])
                if v.size == 0:
                    lim[j], thr[j], whole[j] = (0.0, 1.0), 0.0, (0.0, 1.0)
                else:
                    lim[j], thr[j] = (float(v[v.size // 10]), float(v[9 * v.size // 10])), v[v.size // 2]
                    whole[j] = float(v[0]), float(v[-1])
                for pair in (lim[j], whole[j]):
                    if not pair[0] < pair[1]:
                        pair[:] = pair[0] - 0.5, pair[0] + 0.5
                v = counted[~np.isnan(counted)]
                if v.size:                                             # include/glabc.h glabc_key_counts: -0 is +0, order-preserving
                    u = np.where(v == 0, np.float32(0.0), v).astype(np.float32).view(np.uint32)
                    keys = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
                    extremes[j] = keys.min(), keys.max()
            for bins, edges, levels in ((7, lim, thr), (1, whole, np.full(k, np.inf, np.float32))):
                where = " (id0 %d, %d bins)" % (id0, bins)
                ref = dict(zip(("counts", "tails"), predictive._torch_weighted_tables(stats, m, bins, edges, levels)))
                ref["extremes"] = extremes
                got = tables(id0, bins, edges, levels, ("counts", "tails", "extremes"))
                for name in ("counts", "tails", "extremes"):
                    if not np.array_equal(got[name], ref[name]):
                        refuse(name, where)
                    if not np.array_equal(tables(id0, bins, edges, levels, (name,))[name], ref[name]):
                        refuse(name, " asked for alone" + where)
        return True

    def _gamma_prior(self):
        try:
            return self.prior.descriptor().kind == _capi.DIST_GAMMA
        except (AttributeError, NotImplementedError, ValueError):
            return False

    def self_check(self, algo, batch_size=1, n_chains=512, steps=4, seed=20240229, gamma=False, proposal=None):
        """The freshly compiled kernel against the split-phase path on the same Philox streams: a few iterations of
        `n_chains` synthetic chains through both (same simulator binary for the rows, library kernels for everything
        else -- the path tests/test_generic_path.py holds to the CPU checker), compared bit for bit.  Runs once per program
        (a few ms; the wide program once per batch size, at the lanes per chain the library launches for it);
        GLABC_RTC_SELF_CHECK=0 skips it.  It exists because the run-time compiler has miscompiled this very
        kernel before: a mismatch raises instead of returning samples from the wrong law.
        gamma: the check of a GLABC_RTC_GAMMA program runs its Gamma kernel -- the importance / global proposal is `proposal` (the
        sampler call's), else the prior when that is a Gamma, else Gamma(shape 4, rate 2) per coordinate; the chains start at
        positive states around a Gamma's mean."""
        from .GlobalMCMC import GlobalMCMC
        from .GLMCMC import GLMCMC
        dev = engine.require_device(None)
        g = torch.Generator().manual_seed(seed)
        d = self.theta_dim
        pd = self.prior.descriptor()
        loc = torch.tensor([pd.p0[j] for j in range(d)])
        scale = torch.tensor([pd.p2[j] for j in range(d)])
        if gamma or pd.kind == _capi.DIST_GAMMA:
            if proposal is not None:
                imp = proposal
            elif pd.kind == _capi.DIST_GAMMA:
                imp = self.prior
            else:
                imp = distribution.Gamma(torch.full((d,), 4.0), torch.full((d,), 2.0))
            gd = pd if pd.kind == _capi.DIST_GAMMA else imp.descriptor()
            if gd.kind != _capi.DIST_GAMMA:
                raise ValueError("a Gamma program is checked with a Gamma prior or proposal")
            shape = torch.tensor([gd.p0[j] for j in range(d)])        # p0 = shape, p2 = 1 / rate
            mean = shape * torch.tensor([gd.p2[j] for j in range(d)])
            theta0 = mean * torch.exp(0.3 * torch.randn(n_chains, d, generator=g))
            spread = mean / torch.sqrt(shape)                         # the Gamma's standard deviation
        elif pd.kind == _capi.DIST_UNIFORM:                           # p0 = low, p2 = high - low
            theta0 = loc + scale * torch.rand(n_chains, d, generator=g)
            imp = distribution.Uniform(d, loc, loc + scale)
            spread = scale / 4.0
        else:
            theta0 = loc + scale * torch.randn(n_chains, d, generator=g)
            imp = distribution.DiagGaussian(d, loc.clone(), torch.log(scale))
            spread = scale
        local = distribution.DiagGaussian(d, torch.zeros(d), torch.log(0.3 * spread))
        y0 = self.simulate_from_noise(theta0, torch.randn(n_chains, self.noise_dim, generator=g)).cpu()
        out = []
        for path, kw in (("fused", {}), ("generic", dict(sentinel_redraw=False, graph=False))):
            if algo == _capi.ALGO_GLMCMC:
                r = GLMCMC(self, steps + 1, theta0, y0, local, None, 0.5, imp, batch_size, seed=seed, device=dev, verbose=False,
                           path=path, **kw)
            else:
                r = GlobalMCMC(self, steps + 1, theta0, y0, imp, None, 0.5, local, seed=seed, device=dev, verbose=False, path=path,
                               **kw)
            out.append(r[1].contiguous().view(torch.int32))
        if not torch.equal(out[0], out[1]):
            bad = int((out[0] != out[1]).any(dim=-1).any(dim=0).sum()) if out[0].dim() == 3 else -1
            raise SimulatorSelfCheckError(
                "the run-time compiled kernel (algorithm %d, batch size %d) disagrees with the split-phase path on %d of %d "
                "chains after %d iterations: refusing to sample with it (use path='generic', and please report the "
                "simulator source)" % (algo, batch_size, bad, n_chains, steps))
        return True

    def __del__(self):
        try:
            for h in self._programs.values():
                _capi.lib().glabc_rtc_release(h)
        except Exception:                       # interpreter shutdown
            pass

    # ---- the duck-typed Model protocol (examples/Mixture.py:5-53) ----------------------------------------------------
    def simulate_from_noise(self, theta, eps):
        """generate_samples(theta, 1) with the simulator's standard normals supplied (rows on the device)"""
        dev = engine.require_device(theta.device if theta.is_cuda else None)
        th = theta.detach().to(device=dev, dtype=torch.float32).reshape(-1, self.theta_dim).contiguous()
        ee = eps.detach().to(device=dev, dtype=torch.float32).reshape(th.shape[0], self.noise_dim).contiguous()
        y = torch.empty(th.shape[0], self.y_dim, dtype=torch.float32, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _capi.check(_capi.lib().glabc_rtc_simulate(self.program(_capi.ALGO_GLOBALMCMC), th.data_ptr(), ee.data_ptr(),
                                                       th.shape[0], y.data_ptr(), C.c_void_p(stream)), "glabc_rtc_simulate")
        return y if theta.is_cuda else y.cpu()

    def generate_samples(self, theta, num_samples=1):
        theta = theta.reshape(-1, self.theta_dim)
        if num_samples != 1:
            theta = theta.repeat_interleave(num_samples, dim=0) if theta.shape[0] > 1 else theta.expand(num_samples, -1)
        eps = torch.randn(theta.shape[0], self.noise_dim, device=theta.device)
        return self.simulate_from_noise(theta, eps)

    def _dev(self, t):
        return t if t.is_cuda else t.to(engine.require_device(None))

    def _rows(self, what, rows, epsilon=None):
        """glabc_rtc_model_rows: a callback the source replaces, on rows, through the functions the fused kernel calls"""
        x = self._dev(rows).detach().to(torch.float32).contiguous()
        out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
        m = self.descriptor(epsilon)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        with torch.cuda.device(x.device):
            _capi.check(_capi.lib().glabc_rtc_model_rows(self.program(_capi.ALGO_GLOBALMCMC), C.byref(m), what, x.data_ptr(),
                                                         x.shape[0], out.data_ptr(), C.c_void_p(stream)), "glabc_rtc_model_rows")
        return out

    def prior_log_prob(self, samples):
        s = samples.reshape(-1, self.theta_dim)
        if self.user_prior:
            out = self._rows(_capi.RTC_PRIOR_LOG_PROB, s)
        else:
            out = _launch_rowwise("glabc_model_prior_log_prob", self.descriptor(), self._dev(s), "prior_log_prob")
        return out if samples.is_cuda else out.cpu()

    def discrepancy(self, y):
        yy = y.reshape(-1, self.y_dim)
        if self.user_discrepancy:
            out = self._rows(_capi.RTC_DISCREPANCY, yy)
        else:
            out = _launch_rowwise("glabc_model_discrepancy", self.descriptor(), self._dev(yy), "discrepancy")
        return out if y.is_cuda else out.cpu()

    def calculate_log_kernel(self, y, epsilon=None):
        yy = y.reshape(-1, self.y_dim)
        if self.user_discrepancy or self.user_kernel:
            out = self._rows(_capi.RTC_LOG_KERNEL, yy, epsilon)
        else:
            out = _launch_rowwise("glabc_model_log_kernel", self.descriptor(epsilon), self._dev(yy), "calculate_log_kernel")
        return out if y.is_cuda else out.cpu()

    def descriptor(self, epsilon=None):
        if epsilon is None:
            epsilon = self.epsilon
        m = _capi.Model()
        m.sim_kind = _capi.SIM_USER
        m.theta_dim, m.y_dim = self.theta_dim, self.y_dim
        m.prior = self.prior.descriptor()
        m.noise = distribution.DiagGaussian(self.noise_dim, torch.zeros(self.noise_dim), torch.zeros(self.noise_dim)).descriptor()
        _fill(m.y_obs, self.y_obs.reshape(-1))
        kern = distribution.DiagGaussian(1, loc=torch.tensor([0.0]), log_scale=torch.log(torch.tensor([epsilon]))).descriptor()
        m.kern_log_scale, m.kern_scale, m.kern_c0 = kern.p1[0], kern.p2[0], kern.c0
        m.epsilon = float(np.float32(epsilon))
        return m
