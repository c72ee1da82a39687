"""glabc_rtc_abc_draws / glabc_rtc_smc_draws (csrc/glabc_rtc.hip: the draw kernels of csrc/glabc_abc.h / glabc_smc.h compiled around a user's
simulator) on the GPU, bit for bit.

(a) The restated Mixture source equals the built-in glabc_abc_draws / glabc_smc_draws on the equivalent GLABC_SIM_ABS_GAUSS Model in
    every output, with a DiagGaussian and with a Uniform prior.
(b) NONLINEAR (3, 2, 4), a source with its own discrepancy and kernel (2, 3, 3), and the edge pair theta 1 / noise 1 and theta 8, y 8,
    noise 5 (noise dimensions 4 and 5 straddle a Philox block; theta_dim 8 is where model_after_search matters) equal the composed entry
    points of include/glabc.h in theta, y, distance and log-prior, and a host restatement in every output, the acceptance included:
    tests/rejection_ref.py / smc_ref.py for theta and the noise, the same source through gcc (test_rtc.host_simulator) for the simulator,
    the discrepancy and the kernel, the checker's glabc_expf and uniform.
Shapes: n = 1, 255, 256, 257 and 1000 (one draw per lane, workgroups of 256), stride > n between canaries, row0 = 2^32 - 3 (crosses the
counter's low word), listed ids out of order with repeats and values >= 2^32, every output alone; populations of 1, 2 and 4097 centres;
the +inf rule under a Uniform prior with a bandwidth that puts proposals on both sides of the support; every refusal in its order and
the refusals between the three kinds of program.  Five draws programs are compiled, once each, and a sampler and a mixture program
for the cross-refusals.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle_lib
import rejection_ref as R
import smc_ref as S
from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import distribution
from glabcmcmc_amd.compiled import CompiledModel
from helpers import bits, dev, host
from test_rejection_shapes import ERR_ARG, ERR_DIM, ERR_KIND, ERR_NULL, SEED, Guarded
from test_rtc import NONLINEAR, host_hooks, host_simulator, mixture_source, user_model_desc
from test_rtc_draws_host import DIS_AND_KERNEL
from test_smc_shapes import DevicePopulation

pytestmark = pytest.mark.gpu

N_REF = 1000
ROW0 = 2 ** 32 - 3
SIZES = (1, 255, 256, 257, 1000)
NAMES = ("theta", "y", "distance", "log_prior", "accept")

EDGE1 = """
GLABC_SIMULATOR void glabc_user_simulate(const float* theta, const float* eps, float* y)
{
    y[0] = theta[0] * theta[0] + 0.5f * eps[0];
}
"""
EDGE8 = """
/* theta[8], eps[5] -> y[8]: five normals, the fifth from the second Philox block */
GLABC_SIMULATOR void glabc_user_simulate(const float* theta, const float* eps, float* y)
{
    for (int j = 0; j < 8; ++j) y[j] = fmaf(0.25f + 0.05f * (float)j, eps[j % 5], fabsf(theta[j])) + 0.125f * eps[4];
}
"""
# name -> (source, (theta_dim, y_dim, noise_dim)); the Mixture source's noise scale is the built-in Model's own float32
SOURCES = {"nonlinear": (NONLINEAR, (3, 2, 4)), "dis_and_kernel": (DIS_AND_KERNEL, (2, 3, 3)), "edge1": (EDGE1, (1, 1, 1)),
           "edge8": (EDGE8, (8, 8, 5))}
CASES = [(name, prior) for name in SOURCES for prior in ("gauss", "uniform")]


def prior_of(kind, d):
    if kind == "gauss":
        return distribution.DiagGaussian(d, torch.tensor([0.1 * j for j in range(d)]), torch.log(torch.tensor([1.0 + 0.25 * j for j in range(d)])))
    return distribution.Uniform(d, torch.tensor([-2.0 - 0.5 * j for j in range(d)]), torch.tensor([2.5 + 0.25 * j for j in range(d)]))


@functools.lru_cache(maxsize=None)
def builtin_mixture(kind):
    return R.abs_gauss_model(2, prior_of(kind, 2), epsilon=1.0).descriptor()


@functools.lru_cache(maxsize=None)
def source_of(name):
    if name == "mixture":
        m = builtin_mixture("gauss")
        return mixture_source([m.noise.p2[0], m.noise.p2[1]]), (2, 2, 2)
    return SOURCES[name]


@functools.lru_cache(maxsize=None)
def model_of(case):
    """the glabc_model (GLABC_SIM_USER) of a case; epsilon wide enough for both acceptance outcomes to occur"""
    name, kind = case
    if name == "mixture":
        return user_model_desc(builtin_mixture(kind), 2)
    source, (d, yd, nd) = source_of(name)
    return CompiledModel(theta_dim=d, y_dim=yd, simulator_source=source, prior=prior_of(kind, d), y_obs=[1.0 - 0.1 * j for j in range(yd)],
                         epsilon=0.6 + 0.5 * yd, noise_dim=nd).descriptor()


@functools.lru_cache(maxsize=None)
def program_of(name):
    """the draws program of a source: compiled once per module, never released before the interpreter ends"""
    source, (d, yd, nd) = source_of(name)
    handle, log = C.c_void_p(), C.create_string_buffer(1 << 14)
    rc = A.lib().glabc_rtc_compile_draws(source.encode(), d, yd, nd, C.byref(handle), log, len(log))
    assert rc == 0, log.value.decode()
    assert b"spills" not in log.value, log.value.decode()
    return handle


@functools.lru_cache(maxsize=None)
def host_source(name):
    source, dims = source_of(name)
    return host_simulator(source, *dims)


@functools.lru_cache(maxsize=None)
def population_of(case):
    """1000 centres with random weights holding exact zeros; Uniform priors: centres inside the support and a bandwidth of 1.5, so
    that proposals fall on both sides of its edge"""
    d = model_of(case).theta_dim
    rng = np.random.default_rng(200 + d)
    w = rng.random(1000).astype(np.float32)
    w[rng.random(1000) < 0.1] = 0.0
    X = rng.uniform(-1.5, 1.5, (1000, d)).astype(np.float32)
    if case[1] == "uniform":
        return DevicePopulation(S.HostPopulation(X, w, bw=[1.5] * d))
    return DevicePopulation(S.HostPopulation(X, w, h=0.7))


# ---------------------------------------------------------------------------------- the host restatement
def restate(case, ids, hostpop=None, seed=SEED):
    """-> {name: array} of the draws `ids` from the checker's functions and the source through gcc (module docstring)"""
    L = oracle_lib.load()
    model = model_of(case)
    lib, fn = host_source(case[0])
    L.oracle_set_user_simulator(fn)
    L.oracle_set_user_model(*host_hooks(lib))
    ids = np.asarray(ids, np.int64)
    n, d, yd, nd = ids.size, model.theta_dim, model.y_dim, model.noise.dim
    theta = np.ascontiguousarray(R.prior_draws(model.prior, seed, ids) if hostpop is None else S.kde_rows(hostpop, seed, ids))
    eps = R.noise_normals(seed, ids, nd)
    y, dis = np.empty((n, yd), np.float32), np.empty(n, np.float32)
    for i in range(n):                                                     # row by row: the checker strides eps by y_dim
        assert L.oracle_model_simulate(C.byref(model), theta[i].ctypes.data, eps[i].ctypes.data, 1, y[i].ctypes.data) == 0
    assert L.oracle_model_discrepancy(C.byref(model), y.ctypes.data, n, dis.ctypes.data) == 0
    out = {"theta": theta, "y": y}
    if hostpop is not None:
        lp = np.empty(n, np.float32)
        assert L.oracle_model_prior_log_prob(C.byref(model), theta.ctypes.data, n, lp.ctypes.data) == 0
        out["log_prior"] = lp
        dis = np.where(lp == -np.inf, np.float32(np.inf), dis).astype(np.float32)
    out["distance"] = dis
    w = R.philox_blocks((seed ^ R.ACCEPT_KEY) & R.M64, ids, 0)
    w0, w1 = np.ascontiguousarray(w[:, 0]), np.ascontiguousarray(w[:, 1])
    u, upos, u64 = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.float64)
    L.oracle_uniforms_v(w0.ctypes.data, w1.ctypes.data, n, u.ctypes.data, upos.ctypes.data, u64.ctypes.data)
    with np.errstate(all="ignore"):
        if hasattr(lib, "glabc_user_kern_host"):                           # K(dis) / K(0) from the user's two logarithms
            scale = C.c_float(model.kern_scale)
            lk0 = np.float32(lib.glabc_user_kern_host(C.c_float(0.0), scale))
            arg = np.array([np.float32(lib.glabc_user_kern_host(C.c_float(float(v)), scale)) for v in dis], np.float32) - lk0
        else:
            e = (dis - np.float32(0.0)) / np.float32(model.kern_scale)
            arg = -(np.float32(0.5) * (e * e))
    arg = np.ascontiguousarray(arg, np.float32)
    p = np.empty(n, np.float32)
    L.oracle_expf_v(arg.ctypes.data, n, p.ctypes.data)
    out["accept"] = (u < p).astype(np.uint8)
    L.oracle_set_user_model(None, None, None)
    return out


@functools.lru_cache(maxsize=None)
def reference(case, smc, row0):
    """the restated draws row0 .. row0 + N_REF - 1: computed once, never modified"""
    out = restate(case, np.arange(N_REF, dtype=np.int64) + row0, population_of(case).host if smc else None)
    for a in out.values():
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------- the calls
def call(hip, case, pop, row0, ids, n, stride, want=None, seed=SEED, expect=0, program=None, model=None, builtin=False):
    """one call into guarded buffers -> {name: host array}, theta / y as [n][dim].  pop None: glabc_rtc_abc_draws, else
    glabc_rtc_smc_draws; builtin: glabc_abc_draws / glabc_smc_draws on `model`"""
    model = model_of(case) if model is None else model
    program = program_of(case[0]) if program is None and not builtin else program
    names = tuple(k for k in NAMES if pop is not None or k != "log_prior")
    want = names if want is None else want
    buf = {k: Guarded(model.theta_dim if k == "theta" else model.y_dim if k == "y" else 1, stride, u8=k == "accept") for k in names}
    idt = None if ids is None else dev(np.asarray(ids, np.int64))
    p = lambda k: buf[k].ptr if k in want else None          # noqa: E731
    head = () if builtin else (program,)
    idp = None if idt is None else idt.data_ptr()
    if pop is None:
        fn = hip.glabc_abc_draws if builtin else hip.glabc_rtc_abc_draws
        rc = fn(*head, C.byref(model), seed, row0, idp, n, stride, p("theta"), p("y"), p("distance"), p("accept"), None)
    else:
        fn = hip.glabc_smc_draws if builtin else hip.glabc_rtc_smc_draws
        popd = None if pop == "null" else C.byref(pop if isinstance(pop, A.Kde) else pop.struct)
        rc = fn(*head, C.byref(model), popd, seed, row0, idp, n, stride, p("theta"), p("y"), p("distance"), p("log_prior"), p("accept"), None)
    torch.cuda.synchronize()
    assert rc == expect, rc
    out = {}
    for k, b in buf.items():
        if k in want and rc == 0 and n > 0:
            a = b.read(n)
            out[k] = np.ascontiguousarray(a.T) if k in ("theta", "y") else a[0].copy()
        else:
            b.untouched()
    if "accept" in out:
        assert np.isin(out["accept"], (0, 1)).all()
    return out


def same(a, b):
    return np.array_equal(a, b) if a.dtype == np.uint8 else np.array_equal(bits(a), bits(b))


def assert_equals(got, ref, rows, what):
    for k in got:
        assert same(got[k], ref[k][rows]), "%s: %s differs" % (what, k)


def composed(hip, case, pop, row0, n):
    """the entry points a draw is composed of (include/glabc.h), theta, eps and y through device memory"""
    model, prog = model_of(case), program_of(case[0])
    d, yd, nd = model.theta_dim, model.y_dim, model.noise.dim
    z, lq = torch.empty(d, n, device="cuda"), torch.empty(n, device="cuda")
    if pop is None:
        assert hip.glabc_dist_forward(C.byref(model.prior), n, SEED, row0, z.data_ptr(), lq.data_ptr(), None) == 0
    else:
        assert hip.glabc_kde_sample(C.byref(pop.struct), n, SEED, row0, z.data_ptr(), None) == 0
    theta = z.t().contiguous()
    e = torch.empty(nd, n, device="cuda")
    assert hip.glabc_dist_forward(C.byref(model.noise), n, SEED ^ R.NOISE_KEY, row0, e.data_ptr(), lq.data_ptr(), None) == 0
    eps = e.t().contiguous()
    y, dis = torch.empty(n, yd, device="cuda"), torch.empty(n, device="cuda")
    assert hip.glabc_rtc_simulate(prog, theta.data_ptr(), eps.data_ptr(), n, y.data_ptr(), None) == 0
    if "GLABC_USER_DISCREPANCY" in source_of(case[0])[0]:
        assert hip.glabc_rtc_model_rows(prog, C.byref(model), A.RTC_DISCREPANCY, y.data_ptr(), n, dis.data_ptr(), None) == 0
    else:
        assert hip.glabc_model_discrepancy(C.byref(model), y.data_ptr(), n, dis.data_ptr(), None) == 0
    out = {"theta": host(theta), "y": host(y)}
    if pop is not None:
        lp = torch.empty(n, device="cuda")
        assert hip.glabc_model_prior_log_prob(C.byref(model), theta.data_ptr(), n, lp.data_ptr(), None) == 0
        out["log_prior"] = host(lp)
        dis = torch.where(lp == -np.inf, torch.full_like(dis, np.inf), dis)
    out["distance"] = host(dis)
    return out


# ---------------------------------------------------------------------------------- (a) the Mixture source against the built-in kernels
@pytest.mark.parametrize("kind", ["gauss", "uniform"])
def test_mixture_source_equals_the_builtin_kernels(hip, kind):
    case, pop = ("mixture", kind), population_of(("mixture", kind))
    for row0 in (0, ROW0):
        for p in (None, pop):
            got = call(hip, case, p, row0, None, N_REF, N_REF + 5)
            want = call(hip, case, p, row0, None, N_REF, N_REF + 5, model=builtin_mixture(kind), builtin=True)
            assert set(got) == set(want) and len(got) == (4 if p is None else 5)
            assert_equals(got, want, slice(None), "mixture %s row0 %d" % (kind, row0))
            assert 0 < got["accept"].sum() < N_REF
    ids = np.array([ROW0 + 700, 5, ROW0 + 2, 5, 2 ** 40 + 999, 0], np.int64)
    for p in (None, pop):
        assert_equals(call(hip, case, p, 0, ids, ids.size, ids.size + 3),
                      call(hip, case, p, 0, ids, ids.size, ids.size + 3, model=builtin_mixture(kind), builtin=True), slice(None), "ids")


# ---------------------------------------------------------------------------------- (b) composition and restatement
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s" % c)
def test_fused_equals_composition_and_restatement(hip, case):
    pop = population_of(case)
    for p in (None, pop):
        for row0 in (0, ROW0):
            ref = reference(case, p is not None, row0)
            got = call(hip, case, p, row0, None, N_REF, N_REF + 5)
            assert_equals(got, ref, slice(None), "%r row0 %d against the restatement" % (case, row0))
            twin = composed(hip, case, p, row0, N_REF)
            for k, want in twin.items():
                assert same(got[k], want), "%r row0 %d: %s differs from the composed entry points" % (case, row0, k)
            assert 0 < got["accept"].sum() < N_REF                          # both outcomes occur


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_the_workgroup(hip, n):
    for case in (("nonlinear", "gauss"), ("dis_and_kernel", "uniform"), ("edge8", "uniform"), ("edge1", "gauss")):
        for p in (None, population_of(case)):
            for row0, stride in ((0, n + 5), (ROW0, n)):
                got = call(hip, case, p, row0, None, n, stride)
                assert_equals(got, reference(case, p is not None, row0), slice(0, n), "%r n %d row0 %d" % (case, n, row0))


@pytest.mark.parametrize("case", [("nonlinear", "uniform"), ("dis_and_kernel", "gauss"), ("edge1", "uniform"), ("edge8", "gauss")],
                         ids=lambda c: "%s-%s" % c)
def test_listed_ids_and_each_output_alone(hip, case):
    pop = population_of(case)
    rng = np.random.default_rng(3)
    ids = np.concatenate([[ROW0 + 700, 5, ROW0 + 2, 5, 2 ** 40 + 999, 0, ROW0 + 3, 999, ROW0 + 2], rng.permutation(300) + ROW0 - 100]).astype(np.int64)
    rng.shuffle(ids)
    for p in (None, pop):
        ref = restate(case, ids, None if p is None else p.host)
        got = call(hip, case, p, 0, ids, ids.size, ids.size + 5)
        assert_equals(got, ref, slice(None), "%r listed ids" % (case,))
        for k in got:                                                       # each output alone, the others NULL
            alone = call(hip, case, p, 0, ids, ids.size, ids.size + 5, want=(k,))
            assert set(alone) == {k} and same(alone[k], ref[k]), "%r: %s alone" % (case, k)
        assert call(hip, case, p, 0, ids, 0, 0) == {}                       # n = 0: OK, nothing written


@pytest.mark.parametrize("n_centres", [1, 2, 4097])
def test_populations_of_one_two_and_4097_centres(hip, n_centres):
    for case in (("nonlinear", "gauss"), ("edge8", "uniform")):
        d = model_of(case).theta_dim
        rng = np.random.default_rng(n_centres)
        X = rng.uniform(-1.0, 1.0, (n_centres, d)).astype(np.float32)
        w = None if n_centres == 1 else rng.random(n_centres).astype(np.float32)
        pop = DevicePopulation(S.HostPopulation(X, w, bw=[0.4] * d))
        ids = np.arange(300, dtype=np.int64) + ROW0 - 150
        got = call(hip, case, pop, ROW0 - 150, None, 300, 300)
        assert_equals(got, restate(case, ids, pop.host), slice(None), "%r %d centres" % (case, n_centres))


@pytest.mark.parametrize("name", list(SOURCES))
def test_support_rule_under_a_uniform_prior(hip, name):
    case = (name, "uniform")
    ref = reference(case, True, 0)                                          # theta from glabc_kde_sample's restatement, not the code under test
    outside = np.isinf(ref["log_prior"])
    assert 20 < outside.sum() < N_REF - 20                                   # both classes occur
    got = call(hip, case, population_of(case), 0, None, N_REF, N_REF)
    assert same(got["log_prior"], ref["log_prior"])
    assert np.isposinf(got["distance"][outside]).all() and not got["accept"][outside].any()
    assert np.isfinite(got["distance"][~outside]).all() and got["accept"][~outside].any()
    assert np.isfinite(got["y"]).all() and same(got["y"], ref["y"])          # y is still the simulated row
    only = call(hip, case, population_of(case), 0, None, N_REF, N_REF, want=("distance",))
    assert np.isposinf(only["distance"][outside]).all()


# ---------------------------------------------------------------------------------- refusals
def other_programs(hip):
    """a sampler program and a mixture program of NONLINEAR's shape"""
    out = []
    for fn in (hip.glabc_rtc_compile, hip.glabc_rtc_compile_mix):
        handle, log = C.c_void_p(), C.create_string_buffer(1 << 14)
        assert fn(NONLINEAR.encode(), A.ALGO_GLMCMC, 3, 2, 4, 5, C.byref(handle), log, len(log)) == 0, log.value.decode()
        out.append(handle)
    return out


def test_refusals_in_their_order(hip):
    case = ("nonlinear", "gauss")
    m, pop = model_of(case), population_of(case)

    def changed(**fields):
        c = A.Model()
        C.memmove(C.byref(c), C.byref(m), C.sizeof(A.Model))
        for k, v in fields.items():
            obj, name = (c.prior, k[6:]) if k.startswith("prior_") else (c.noise, k[6:]) if k.startswith("noise_") else (c, k)
            setattr(obj, name, v)
        return c

    def popc(**fields):
        k = A.Kde()
        C.memmove(C.byref(k), C.byref(pop.struct), C.sizeof(A.Kde))
        for name, v in fields.items():
            if name == "bandwidth0":
                k.bandwidth[0] = v
            else:
                setattr(k, name, v)
        return k

    sampler, mix = other_programs(hip)
    try:
        for p in (None, pop):
            every = dict(case=case, pop=p, row0=0, ids=None, n=4, stride=4)
            # NULL outputs; NULL program and model (each ahead of everything else)
            call(hip, want=(), expect=ERR_NULL, **every)
            call(hip, want=(), expect=ERR_NULL, **dict(every, model=changed(sim_kind=A.SIM_ABS_GAUSS)))
            hipf = hip.glabc_rtc_abc_draws if p is None else hip.glabc_rtc_smc_draws
            tail = (SEED, 0, None, 4, 4, None, None, None, None) + (() if p is None else (None,)) + (None,)
            popa = () if p is None else (C.byref(pop.struct),)
            assert hipf(None, C.byref(m), *popa, *tail) == ERR_NULL and hipf(program_of("nonlinear"), None, *popa, *tail) == ERR_NULL
            # the simulator's kind, ahead of the program's kind, ahead of the dimensions
            call(hip, expect=ERR_KIND, **dict(every, model=changed(sim_kind=A.SIM_ABS_GAUSS), program=sampler))
            call(hip, expect=ERR_KIND, **dict(every, model=changed(sim_kind=A.SIM_GK, theta_dim=4)))
            for other in (sampler, mix):
                call(hip, expect=ERR_KIND, **dict(every, program=other))
                call(hip, expect=ERR_KIND, **dict(every, program=other, model=changed(theta_dim=2)))
            # the dimensions, ahead of the prior
            for f in (dict(theta_dim=2), dict(y_dim=3), dict(noise_dim=3)):
                call(hip, expect=ERR_DIM, **dict(every, model=changed(prior_kind=A.DIST_GAMMA, **f)))
            call(hip, expect=ERR_DIM, **dict(every, program=program_of("edge1")))
            # the prior, ahead of the population and the range
            call(hip, expect=ERR_KIND, **dict(every, model=changed(prior_kind=A.DIST_GAMMA), n=-1))
            call(hip, expect=ERR_KIND, **dict(every, model=changed(prior_dim=2), n=-1))
            if p is not None:
                call(hip, expect=ERR_KIND, **dict(every, model=changed(prior_dim=2), pop=popc(n_samples=0)))
                # the population, in check_smc_draws' order, ahead of the range
                call(hip, expect=ERR_NULL, **dict(every, pop="null", n=-1))
                call(hip, expect=ERR_DIM, **dict(every, pop=popc(dim=9, n_samples=0), n=-1))
                call(hip, expect=ERR_ARG, **dict(every, pop=popc(n_samples=0, x=None), n=-1))
                call(hip, expect=ERR_NULL, **dict(every, pop=popc(x=None, bandwidth0=0.0), n=-1))
                call(hip, expect=ERR_NULL, **dict(every, pop=popc(log_w=None), n=-1))
                call(hip, expect=ERR_ARG, **dict(every, pop=popc(bandwidth0=0.0, cum_q=None), n=-1))
                call(hip, expect=ERR_ARG, **dict(every, pop=popc(bandwidth0=float("inf")), n=-1))
                call(hip, expect=ERR_NULL, **dict(every, pop=popc(cum_q=None, dim=2), n=-1))
                call(hip, expect=ERR_DIM, **dict(every, pop=popc(dim=2), n=-1))
            # the range of draws
            call(hip, expect=ERR_ARG, **dict(every, n=-1))
            call(hip, expect=ERR_ARG, **dict(every, stride=3))
            call(hip, expect=ERR_ARG, **dict(every, row0=-1))
            call(hip, expect=ERR_ARG, **dict(every, row0=1, ids=[0, 1, 2, 3]))
        # the built-in entry points keep refusing a user simulator
        call(hip, case, None, 0, None, 4, 4, expect=ERR_KIND, builtin=True)
        call(hip, case, pop, 0, None, 4, 4, expect=ERR_KIND, builtin=True)
    finally:
        hip.glabc_rtc_release(sampler)
        hip.glabc_rtc_release(mix)


def test_sampler_entry_points_refuse_a_draws_program_and_the_row_kernels_take_it(hip):
    case = ("nonlinear", "gauss")
    m, prog = model_of(case), program_of("nonlinear")
    d = 3
    local = distribution.DiagGaussian(d, torch.zeros(d), torch.zeros(d)).descriptor()
    th, y = torch.zeros(d, 64, device="cuda"), torch.zeros(2, 64, device="cuda")
    lw, flags = torch.zeros(64, device="cuda"), torch.zeros(64, dtype=torch.int32, device="cuda")
    c = A.Chains()
    c.theta, c.y, c.log_w, c.flags = th.data_ptr(), y.data_ptr(), lw.data_ptr(), flags.data_ptr()
    c.n_chains, c.stride = 64, 64
    r = A.Run()
    r.n_steps, r.batch_size, r.global_frequency = 1, 5, 0.5
    assert hip.glabc_rtc_steps(prog, C.byref(m), C.byref(local), C.byref(local), C.byref(c), C.byref(r), None) == ERR_KIND
    mix = distribution.GaussianMixture(2, d, loc=np.zeros((2, d)), scale=np.ones((2, d)), weights=[1.0, 1.0]).descriptor()
    assert hip.glabc_rtc_mix_steps(prog, C.byref(m), C.byref(local), C.byref(mix), C.byref(c), C.byref(r), None) == ERR_KIND
    torch.cuda.synchronize()
    assert not th.any() and not y.any()
    up, ud, uk = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    assert hip.glabc_rtc_hooks(program_of("dis_and_kernel"), C.byref(up), C.byref(ud), C.byref(uk)) == 0
    assert (up.value, ud.value, uk.value) == (0, 1, 1)
