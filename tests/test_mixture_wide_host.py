"""GaussianMixture importance proposals at batch sizes 17..4096 on the host: the argument check of glabc_glmcmc_mix_wide_steps
(csrc/glabc_check.h on the CPU, the way tests/test_mixture_host.py drives check_mix_run) and the dispatch's answer.

check_mix_wide_run is check_mix_run with the lane-group kernel's batch sizes and lanes per chain: every row of the support
matrix is asked of both with the same spoiled arguments and has to return the same status, and rows that hold two defects with
different statuses pin the order of the checks.
"""
import ctypes as C

import numpy as np

from helpers import AbsGaussModel, make_dist
from test_arg_checks import ARG, DIM, KIND, NULL, OK, check_table
from test_mixture_host import MIX_PRELUDE, make_mixture
from test_stream_independence import abs_gauss_model
from glabcmcmc_amd import _capi as A
from glabcmcmc_amd import generic

WIDE = "check_mix_wide_run(&b.m, &b.g, &x, &b.c, &b.r)"
NARROW = "check_mix_run(&b.m, &b.g, &x, &b.c, &b.r, true)"
DIM5 = ("b.m.theta_dim = b.m.y_dim = 5; b.m.prior.dim = b.m.noise.dim = b.g.dim = 5; b.m.prior.p1[3] = b.m.prior.p1[4] = 3.0f; "
        "b.g.p2[3] = b.g.p2[4] = 0.5f; b.m.noise.p2[3] = b.m.noise.p2[4] = 0.5f;")
GK = "make_gk(b); b.g.dim = 4; b.g.p2[3] = 0.5f;"


def wide_rows():
    rows = []

    def row(spoil, want, dim=3, both=False, batch=17):
        """both: the same spoiled arguments, at a batch size of its own, give check_mix_run the same status"""
        pre = "glabc_mixture x = mix3(%d); glabc_tape tp; std::memset(&tp, 0, sizeof tp); (void)tp; " % dim
        rows.append((pre + "b.r.batch_size = %d; " % batch + spoil, WIDE, want))
        if both:
            rows.append((pre + "b.r.batch_size = 5; " + spoil, NARROW, want))

    # batch sizes and lanes per chain
    for n in (17, 18, 64, 4095, 4096):
        row("", OK, batch=n)
    for n in (16, 1, 5, 0, -1, 4097, 1 << 20):
        row("", ARG, batch=n)
    for lanes in (0, 8, 16, 32, 64):
        row("b.r.lanes_per_chain = %d;" % lanes, OK)
        row("b.r.lanes_per_chain = %d;" % lanes, OK, batch=4096)
    for lanes in (1, 2, 4, 7, -8, 12, 128):
        row("b.r.lanes_per_chain = %d;" % lanes, ARG)
    row("b.r.debug_flags = GLABC_DEBUG_EXACT_INDEX; b.r.history = b.f; b.r.hist_stride = 65; b.r.moments = &b.mo; "
        "b.r.global_frequency_per_chain = b.f;", OK, both=True)
    row("b.m.prior = dist3(GLABC_DIST_DIAG_GAUSS); b.g = dist3(GLABC_DIST_UNIFORM);", OK, both=True)
    row(GK, OK, dim=4, both=True)
    # the support matrix
    row(DIM5, KIND, dim=5, both=True)
    row("b.m.prior = dist3(GLABC_DIST_GAMMA);", KIND, both=True)
    row(GK + " b.m.prior = dist3(GLABC_DIST_GAMMA); b.m.prior.dim = 4; b.m.prior.p0[3] = 2.0f; b.m.prior.p1[3] = 0.5f; "
        "b.m.prior.p2[3] = 2.0f;", KIND, dim=4, both=True)
    row("b.g = dist3(GLABC_DIST_GAMMA);", KIND, both=True)                  # the local increment is never a Gamma
    row("b.r.tape = &tp;", ARG, both=True)
    row("b.r.math_mode = GLABC_MATH_FAST;", ARG, both=True)
    row("b.r.step0_device = b.u;", ARG, both=True)
    # a defective mixture
    row("x.n_modes = 0;", ARG, both=True)
    row("x.n_modes = 9;", ARG, both=True)
    row("", DIM, dim=2, both=True)
    row("x.inv_scale[2][1] = Inf;", ARG, both=True)
    row("x.scale[1][0] = 0.0;", ARG, both=True)
    row("x.cum_weight[1] = 0.2;", ARG, both=True)
    row("x.cum_weight[0] = 0.0; x.log_weight[0] = -Inf;", OK, both=True)    # a mode of weight zero
    row("x.c0 = NaN;", ARG, both=True)
    # what every stepping entry point asks
    row("b.r.n_steps = -1;", ARG, both=True)
    row("b.r.n_steps = 0;", OK, both=True)
    row("b.r.global_frequency = NaN;", ARG, both=True)
    row("b.r.history = b.f; b.r.hist_stride = 64;", ARG, both=True)
    row("b.r.step0 = 0xFFFFFFFFu; b.r.n_steps = 1;", ARG, both=True)
    row("b.c.theta = nullptr;", NULL, both=True)
    row("b.c.log_w = nullptr;", NULL, both=True)
    row("b.c.flags = nullptr;", NULL, both=True)
    row("b.c.chain0 = -1;", ARG, both=True)
    row("b.mo.sum_jump = nullptr; b.r.moments = &b.mo;", NULL, both=True)
    # the order of the checks: model, mixture, local increment, pointers, tape, chains, ..., batch size, lanes, history, moments
    row(DIM5, KIND, dim=5, batch=16)
    row("b.m.prior = dist3(GLABC_DIST_GAMMA); x.n_modes = 9;", KIND)
    row("x.n_modes = 9; b.g = dist3(GLABC_DIST_GAMMA);", ARG)
    row("b.g = dist3(GLABC_DIST_GAMMA);", KIND, batch=16)
    row("b.g = dist3(GLABC_DIST_GAMMA); b.r.tape = &tp;", KIND)
    row("b.c.theta = nullptr;", NULL, batch=16)
    row("b.c.theta = nullptr; b.r.tape = &tp;", ARG)
    row("b.c.flags = nullptr; b.r.lanes_per_chain = 4;", NULL)
    row("b.mo.sum_jump = nullptr; b.r.moments = &b.mo;", ARG, batch=16)
    row("b.mo.sum_jump = nullptr; b.r.moments = &b.mo;", ARG, batch=4097)
    row("b.mo.sum_jump = nullptr; b.r.moments = &b.mo; b.r.lanes_per_chain = 4;", ARG)
    row("b.mo.sum_jump = nullptr; b.r.moments = &b.mo; b.r.step0_device = b.u;", NULL)
    rows.append(("b.r.batch_size = 17;", "check_mix_wide_run(&b.m, &b.g, nullptr, &b.c, &b.r)", NULL))
    rows.append(("glabc_mixture x = mix3(3); b.r.batch_size = 17;", "check_mix_wide_run(&b.m, &b.g, &x, &b.c, nullptr)", NULL))
    rows.append(("glabc_mixture x = mix3(3); b.r.batch_size = 17;", "check_mix_wide_run(&b.m, &b.g, &x, nullptr, &b.r)", NULL))
    rows.append(("glabc_mixture x = mix3(3); b.r.batch_size = 17;", "check_mix_wide_run(&b.m, nullptr, &x, &b.c, &b.r)", NULL))
    rows.append(("glabc_mixture x = mix3(3); b.r.batch_size = 17;", "check_mix_wide_run(nullptr, &b.g, &x, &b.c, &b.r)", NULL))
    return rows


def test_mixture_wide_argument_checks(tmp_path_factory, monkeypatch):
    import test_arg_checks
    monkeypatch.setattr(test_arg_checks, "PRELUDE", test_arg_checks.PRELUDE.replace("struct Base {", MIX_PRELUDE + "struct Base {"))
    check_table(tmp_path_factory, "mixture_wide", wide_rows())


def test_dispatch_takes_a_mixture_up_to_the_lane_group_batch_sizes():
    from glabcmcmc_amd.examples.GK import GK_set

    def ok(model, d, N, K=3, mix=None, **kw):
        local = make_dist(("gauss", [0.0] * d, [0.3] * d))
        return generic.fused_supported(model, (local, mix or make_mixture(K, d)), N, A.MAX_BATCH_WIDE, gamma_ok=True, mixture_ok=True, **kw)

    wide = dict(mixture_max_batch=A.MAX_BATCH_WIDE)
    for N in (1, 16, 17, 64, 4096):
        for d in (1, 2, 3, 4):
            assert ok(AbsGaussModel(0.3, [1.5] * d), d, N, **wide), (d, N)
        assert ok(GK_set(1.0), 4, N, **wide), N
    assert ok(AbsGaussModel(0.3, [1.5] * 2), 2, 4096, K=8, **wide) and ok(AbsGaussModel(0.3, [1.5] * 2), 2, None, **wide)
    assert not ok(AbsGaussModel(0.3, [1.5] * 2), 2, 4097, **wide) and not ok(AbsGaussModel(0.3, [1.5] * 2), 2, 0, **wide)
    assert not ok(GK_set(1.0), 4, 4097, **wide)
    assert not ok(AbsGaussModel(0.3, [1.5] * 5), 5, 64, **wide) and not ok(AbsGaussModel(0.3, [1.5] * 5), 5, 5, **wide)     # theta_dim 5..8
    gamma = make_dist(("gamma", [3.0, 2.0, 2.0, 1.5], [1.0, 2.0, 1.0, 3.0]))
    assert not ok(GK_set(1.0, prior=gamma), 4, 64, **wide)                                                                  # a Gamma prior
    assert not ok(AbsGaussModel(0.3, [1.5] * 2), 2, 64, mix=make_mixture(3, 3), **wide)                                     # dimension mismatch
    model, local, mix = AbsGaussModel(0.3, [1.5] * 2), make_dist(("gauss", [0.0] * 2, [0.3] * 2)), make_mixture(3, 2)
    assert not generic.fused_supported(model, (mix, mix), 64, A.MAX_BATCH_WIDE, gamma_ok=True, mixture_ok=True, **wide)     # a mixture as the local increment
    assert not generic.fused_supported(model, (local, mix), 64, A.MAX_BATCH_WIDE, gamma_ok=True, **wide)                    # an entry point without the variant
    # without the keyword (and with None) the answers of before: the register kernels' batch sizes only
    assert ok(model, 2, 16) and not ok(model, 2, 17) and not ok(model, 2, 64)
    assert not ok(model, 2, 17, mixture_max_batch=None) and ok(model, 2, 16, mixture_max_batch=None)
    # the other proposals' answers do not depend on it
    gauss = make_dist(("gauss", [0.0] * 2, [1.0] * 2))
    for N in (16, 17, 4096, 4097):
        assert generic.fused_supported(model, (local, gauss), N, A.MAX_BATCH_WIDE) == generic.fused_supported(model, (local, gauss), N, A.MAX_BATCH_WIDE, **wide)


def test_wide_entry_point_refuses_before_touching_a_device():
    """the library itself (it loads without a GPU): a refused call returns its status with no device present"""
    lib = A.bind(A.LIB_PATH)
    model = abs_gauss_model(3, 0.3)
    local = make_dist(("gauss", [0.0] * 3, [0.3] * 3)).descriptor()
    mix = make_mixture(3, 3).descriptor()
    buf = np.zeros(256, np.float64)
    chains = A.Chains(65, 0, 65, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None, None, None, None, None)

    def call(entry="glabc_glmcmc_mix_wide_steps", mod=model, loc=local, x=mix, ch=chains, **fields):
        run = A.Run()
        run.step0, run.n_steps, run.global_frequency, run.batch_size = 1, 3, 0.5, 17
        for k, v in fields.items():
            setattr(run, k, v)
        return getattr(lib, entry)(C.byref(mod), C.byref(loc), C.byref(x), C.byref(ch), C.byref(run), None)

    for n in (16, 5, 0, 4097):
        assert call(batch_size=n) == ARG, n
    assert call("glabc_glmcmc_mix_steps", batch_size=17) == ARG              # the register kernels' entry point, as before
    for lanes in (1, 2, 4, 7):
        assert call(lanes_per_chain=lanes) == ARG, lanes
    assert call(math_mode=A.MATH_FAST) == ARG
    tape = A.Tape(buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, 17, 0)
    assert call(tape=C.pointer(tape)) == ARG
    gamma_model = abs_gauss_model(3, 0.3)
    gamma_model.prior = make_dist(("gamma", [2.0] * 3, [1.0] * 3)).descriptor()
    assert call(mod=gamma_model) == KIND
    assert call(loc=make_dist(("gamma", [2.0] * 3, [1.0] * 3)).descriptor()) == KIND
    m5, l5, x5 = abs_gauss_model(5, 0.3), make_dist(("gauss", [0.0] * 5, [0.3] * 5)).descriptor(), make_mixture(3, 5).descriptor()
    assert call(mod=m5, loc=l5, x=x5) == KIND
    assert call(x=make_mixture(3, 2).descriptor()) == DIM
    bad = make_mixture(3, 3).descriptor()
    bad.n_modes = 9
    assert call(x=bad) == ARG
    empty = A.Chains(0, 0, 0, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data, None, None, None, None, None)
    assert call(ch=empty) == OK and call(n_steps=0) == OK                    # nothing to do
    assert call(ch=empty, batch_size=16) == ARG                              # ... but checked all the same
