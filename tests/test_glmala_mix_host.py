"""glabc_glmala_mix_steps without a GPU.

(a) The yardstick's yardstick: the numpy restatement of GLMALA's iSIR move (tests/mala_mix_ref.py) with a DiagGaussian and a Uniform
    candidate provider, assembled iteration by iteration around the checker's MALA move, equals an uninterrupted oracle_glmala_steps
    run bit for bit on every owned array.  This passes without the feature, by design.
(b) The conditions the GPU parity cases of tests/test_glmala_mix_shapes.py must meet, asserted on the reference alone.
(d) check_mala_mix_run (csrc/glabc_check.h) as a table through the stand-alone g++ driver of tests/test_arg_checks.py under the address
    and undefined-behaviour sanitizers; the dispatch decision GLMALA.py makes; the binding's argument types against the header.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import glmala_mix_cases as cases
import mala_mix_ref as ref
from glabcmcmc_amd import _capi as A
from helpers import AbsGaussModel, make_dist
from test_arg_checks import ARG, DIM, KIND, NULL, OK, check_table
from test_glmala_shapes import assert_equal_runs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ (a) the restatement against the checker
@pytest.mark.parametrize("kind", ("gauss", "uniform"))
@pytest.mark.parametrize("d,N", [(1, 1), (1, 16), (2, 5), (2, 3), (3, 4), (3, 9), (4, 5), (4, 16)])
def test_restatement_with_a_dist_provider_equals_the_uninterrupted_checker(oracle, d, N, kind):
    """130 chains x 60 iterations, gf 0.5: the chain assembled from the checker's MALA move and the restated iSIR move, the
    proposal a glabc_dist through oracle_dist_forward / oracle_dist_log_prob (float64 state: a numpy log-prob), against one
    oracle_glmala_steps call with the same glabc_dist.  The filler of step 2 is ANOTHER DiagGaussian, so nothing of the global
    branch can come from it."""
    c = cases.make_case(d, N, K=3, n=130, T=60, gf=0.5, num=(3, 7, 12)[N % 3], y_kind=("away", "zero")[N % 2], seed=900 + 17 * d + N)
    model, mix, mala, filler = cases.descriptors(c)
    imp = make_dist(("uniform", [-3.0] * d, [3.5] * d) if kind == "uniform"
                    else ("gauss", [0.2 - 0.1 * j for j in range(d)], [1.3 + 0.1 * j for j in range(d)])).descriptor()
    theta0, y0 = cases.inputs(c)
    kw = dict(seed=c["seed"], chain0=c["chain0"], T=c["T"], N=N, gf=c["gf"])
    stats = ref.new_stats()
    got = ref.assemble(oracle, model, mala, ref.DistProvider(oracle, imp), filler, theta0, y0, stats=stats, **kw)
    want = ref.uninterrupted(oracle, model, mala, imp, theta0, y0, **kw)
    assert_equal_runs(got, want, "d%d N%d %s" % (d, N, kind))
    # ... and the comparison saw the restated code: every precision combination of the state slot, moves and stays
    for k in ref.COMBOS:
        assert stats[k] >= 3 and stats[k + "_moved"] >= 1, (k, stats)
    assert stats["stay"] >= 3 and stats["both_branches_in_a_wavefront"] >= 3
    assert (want["flags"] & A.FLAG_LW64).any() and want["n_moves"].sum() > 0


# ------------------------------------------------------------------------------------------ (b) conditions on the GPU cases' inputs
@pytest.mark.parametrize("c", cases.DEEP, ids=cases.case_id)
def test_deep_cases_reach_every_branch_of_the_move(oracle, c):
    """Every deep case reaches, in at least 3 chain-iterations each: the state slot as float32 state + float32 weights, TH64 +
    float32 weights, TH64 + LW64 -- each taken with ind > 0 at least once --, every mode of the mixture, and ind = -1 / stay; both
    branches meet in one wavefront in one iteration.  The Uniform-prior case has a mode outside the prior's support: candidates of
    weight 0, and an iteration of some chain with ALL N candidates outside."""
    r, stats, modes = cases.reference(oracle, c)
    for k in ref.COMBOS:
        assert stats[k] >= 3 and stats[k + "_moved"] >= 1, (k, stats)
    assert (modes >= 3).all(), modes
    assert stats["stay"] >= 3 and stats["both_branches_in_a_wavefront"] >= 3
    assert r["n_moves"].sum() > 0 and (r["flags"] & A.FLAG_TH64).any() and (r["flags"] & A.FLAG_LW64).any()
    if c["prior"] == "uniform":
        assert stats["zero_weight"] >= 3 and stats["all_zero_weight"] >= 1, stats
    else:
        assert stats["zero_weight"] == 0                               # a DiagGaussian prior has no candidate of weight 0


def test_sweep_walks_every_instantiation():
    """theta_dim 1..4 x batch size 1..16 x the lean / general square root; mode counts 1, 3, 4, 5, 8 (the branches of the logsumexp
    sum order) and gf 0.3 / 0.5 / 0.8 / 1.0 at every theta_dim; launches that do not divide T; chain0 above 2^32; theta_dim 2 at
    both launch geometries."""
    for d in (1, 2, 3, 4):
        cs = [c for c in cases.SWEEP if c["d"] == d]
        assert {(c["N"], c["y_kind"]) for c in cs} == {(N, y) for N in range(1, 17) for y in ("away", "zero")}
        assert {c["K"] for c in cs} == {1, 3, 4, 5, 8} and {c["gf"] for c in cs} == {0.3, 0.5, 0.8, 1.0}
        assert {c["lanes"] for c in cs} == ({1, 2} if d == 2 else {0})
    for c in cases.SWEEP:
        assert c["n"] == 65 and 8 <= c["T"] <= 12 and 2 <= c["num"] <= 9 and c["T"] % c["spl"] != 0 and c["chain0"] > 2 ** 32
        assert cases.lean(c) == (c["y_kind"] == "away")


@pytest.mark.parametrize("d", (1, 2, 3, 4))
def test_sweep_cases_are_not_idle(oracle, d):
    """per theta_dim, over the sweep: global moves taken and refused, and the float64 state slot where gf < 1"""
    tot = ref.new_stats()
    for c in cases.SWEEP:
        if c["d"] == d and c["lanes"] in (0, 1):
            r, stats, modes = cases.reference(oracle, c)
            assert stats["global_steps"] > 0 and modes.sum() == stats["global_steps"] * c["N"]
            for k in tot:
                tot[k] += stats[k]
    assert tot["f32_moved"] > 0 and tot["stay"] > 0 and tot["th64_lw64"] > 0 and tot["th64_w32"] > 0 and tot["local_steps"] > 0


# ------------------------------------------------------------------------------------------ (d) check_mala_mix_run
MIX = ("glabc_mixture g; std::memset(&g, 0, sizeof g); g.n_modes = 3; g.dim = 3; g.c0 = -2.7568155; "
       "for (int k = 0; k < 3; ++k) { g.log_weight[k] = -1.0986123; g.cum_weight[k] = (k + 1) / 3.0; g.sum_log_scale[k] = -2.0794415; "
       "for (int q = 0; q < 3; ++q) { g.loc[k][q] = k - 1.0; g.scale[k][q] = 0.5; g.inv_scale[k][q] = 2.0; } } ")
BASE = (MIX + "glabc_mala p = {0.25, 0.0625, 0.09, 10, 0}; glabc_tape tp; std::memset(&tp, 0, sizeof tp); (void)tp; ")
CALL = "check_mala_mix_run(&b.m, &g, &p, &b.c, &b.r)"


def mala_mix_rows():
    out = []

    def row(spoil, want, call=CALL):
        out.append((BASE + spoil, call, want))

    row("", OK)
    row("b.m.prior = dist3(GLABC_DIST_DIAG_GAUSS);", OK)
    for d in (1, 2, 4):
        row("b.m.theta_dim = b.m.y_dim = b.m.prior.dim = b.m.noise.dim = g.dim = %d; b.m.prior.p1[3] = 3.0f; b.m.prior.p2[3] = 4.0f; "
            "b.m.noise.p2[3] = 0.5f; for (int k = 0; k < 3; ++k) { g.scale[k][3] = 0.5; g.inv_scale[k][3] = 2.0; }" % d, OK)
    # 1. the model: null, then check_model's own order; a Gamma prior is GLABC_ERR_KIND, whatever else is wrong
    row("", NULL, "check_mala_mix_run(nullptr, &g, &p, &b.c, &b.r)")
    row("", NULL, "check_mala_mix_run(nullptr, nullptr, nullptr, nullptr, nullptr)")
    row("b.m.sim_kind = GLABC_SIM_USER;", KIND)
    row("b.m.theta_dim = 9;", DIM)
    row("b.m.prior = dist3(GLABC_DIST_GAMMA);", KIND)
    row("b.m.prior = dist3(GLABC_DIST_GAMMA); b.m.prior.p0[0] = -1.0f; g.n_modes = 0;", KIND)
    row("b.m.prior.p0[1] = NaN;", ARG)
    row("b.m.kern_scale = 0.0f; g.dim = 2;", ARG)
    row("b.m.y_obs[2] = Inf;", ARG)
    # 2. the simulator kind: GLMALA is the |theta| + noise Model's, ahead of the mixture
    row("make_gk(b);", KIND)
    row("make_gk(b); g.n_modes = 0;", KIND)
    row("make_gk(b);", KIND, "check_mala_mix_run(&b.m, nullptr, &p, &b.c, &b.r)")
    # 3. theta_dim 5..8: no kernel, GLABC_ERR_DIM ahead of the mixture and everything after it
    for d in (5, 8):
        big = ("b.m.theta_dim = b.m.y_dim = b.m.prior.dim = b.m.noise.dim = %d; for (int j = 3; j < 8; ++j) { b.m.prior.p1[j] = 3.0f; "
               "b.m.prior.p2[j] = 4.0f; b.m.noise.p2[j] = 0.5f; } " % d)
        row(big, DIM)
        row(big + "g.n_modes = 0; b.r.batch_size = 17;", DIM)
        row(big, DIM, "check_mala_mix_run(&b.m, nullptr, &p, &b.c, &b.r)")
    # 4. the mixture's own checks where glabc_glmala_steps checks its glabc_dist: ahead of null mala / run and of the chains
    row("", NULL, "check_mala_mix_run(&b.m, nullptr, &p, &b.c, &b.r)")
    row("g.n_modes = 0;", ARG)
    row("g.n_modes = 9;", ARG)
    row("g.dim = 2;", DIM)
    row("g.n_modes = 0; g.dim = 2;", ARG)                                        # n_modes before dim, as check_mixture has them
    row("g.dim = 2;", DIM, "check_mala_mix_run(&b.m, &g, nullptr, &b.c, &b.r)")
    row("g.dim = 2; b.c.theta64 = nullptr;", DIM)
    row("g.scale[1][2] = 0.0;", ARG)
    row("g.inv_scale[0][0] = Inf;", ARG)
    row("g.loc[2][1] = NaN;", ARG)
    row("g.log_weight[0] = -Inf;", OK)                                           # a mode of weight 0
    row("g.log_weight[0] = NaN;", ARG)
    row("g.cum_weight[1] = 0.1;", ARG)
    row("g.cum_weight[2] = 1.5;", ARG)
    row("g.c0 = NaN;", ARG)
    row("g.n_modes = 8; for (int k = 3; k < 8; ++k) { g.log_weight[k] = -1.0; g.cum_weight[k] = 1.0; for (int q = 0; q < 3; ++q) "
        "{ g.scale[k][q] = 0.5; g.inv_scale[k][q] = 2.0; } }", OK)
    # 5. null mala / run, ahead of the chains
    row("", NULL, "check_mala_mix_run(&b.m, &g, nullptr, &b.c, &b.r)")
    row("", NULL, "check_mala_mix_run(&b.m, &g, &p, &b.c, nullptr)")
    row("b.c.stride = 64;", NULL, "check_mala_mix_run(&b.m, &g, nullptr, &b.c, &b.r)")
    # 6. the chains: GLMALA's arrays (log_w and n_moves are optional), then the range
    row("", NULL, "check_mala_mix_run(&b.m, &g, &p, nullptr, &b.r)")
    for field in ("theta", "y", "flags", "theta64", "y64", "log_w64", "grad"):
        row("b.c.%s = nullptr;" % field, NULL)
    row("b.c.log_w = nullptr;", OK)
    row("b.c.n_moves = nullptr;", OK)
    row("b.c.stride = 64;", ARG)
    row("b.c.n_chains = -1;", ARG)
    row("b.c.chain0 = -1;", ARG)
    row("b.c.grad = nullptr; b.c.stride = 64; b.r.n_steps = -1;", NULL)
    row("b.c.n_chains = 0;", OK)
    # 7. n_steps and the batch size, ahead of the frequency
    row("b.r.n_steps = -1;", ARG)
    row("b.r.n_steps = 0;", OK)
    for n, want in ((0, ARG), (1, OK), (16, OK), (17, ARG), (-3, ARG)):
        row("b.r.batch_size = %d;" % n, want)
    # 8. global_frequency, a per-chain array
    row("b.r.global_frequency = NaN;", ARG)
    row("b.r.global_frequency = 1.5f;", OK)
    row("b.r.global_frequency_per_chain = b.f;", ARG)
    # 9. the MALA parameters, ahead of history and moments
    for spoil, want in (("p.num_grad = 1;", ARG), ("p.num_grad = 2;", OK), ("p.num_grad = 65536;", OK), ("p.num_grad = 65537;", ARG),
                        ("p.tau = 0.0;", ARG), ("p.tau = -1.0;", ARG), ("p.tau = NaN;", ARG), ("p.tau = Inf;", ARG), ("p.tau_sq = NaN;", ARG),
                        ("p.eps_sq = -1e-9;", ARG), ("p.eps_sq = 0.0;", OK), ("p.eps_sq = Inf;", ARG)):
        row(spoil, want)
    row("p.num_grad = 1; b.r.moments = &b.mo; b.mo.sum_jump = nullptr;", ARG)     # the MALA parameters before the moments
    row("b.r.batch_size = 17; b.r.moments = &b.mo; b.mo.sum_jump = nullptr;", ARG)
    # 10. history, moments, tape / math mode / dump_draws, lanes_per_chain, the step counter: in this order
    row("b.r.history = b.f; b.r.hist_stride = 64;", ARG)
    row("b.r.history = b.f; b.r.hist_stride = 65;", OK)
    row("b.r.moments = &b.mo; b.mo.sum_jump = nullptr;", NULL)
    row("b.r.moments = &b.mo;", OK)
    row("b.r.history = b.f; b.r.hist_stride = 64; b.r.moments = &b.mo; b.mo.sum_theta = nullptr;", ARG)      # history before moments
    row("b.r.moments = &b.mo; b.mo.sum_theta = nullptr; b.r.tape = &tp;", NULL)                              # moments before the tape
    row("b.r.tape = &tp;", ARG)
    row("b.r.math_mode = GLABC_MATH_FAST;", ARG)
    row("glabc_draws_out dd; std::memset(&dd, 0, sizeof dd); b.r.dump_draws = &dd;", ARG)
    for lanes, want in ((0, OK), (1, OK), (2, OK), (3, ARG), (4, ARG), (-1, ARG)):
        row("b.r.lanes_per_chain = %d;" % lanes, want)
    row("b.r.step0 = 0xFFFFFFFEu;", ARG)
    row("b.r.step0 = 0xFFFFFFFCu;", OK)
    row("b.r.step0_device = b.u;", OK)                                           # not read, as glabc_glmala_steps does not
    return out


def test_check_mala_mix_run(tmp_path_factory):
    check_table(tmp_path_factory, "mala_mix", mala_mix_rows(), flags=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


# ------------------------------------------------------------------------------------------ (d) the dispatch decision
def _mixture(K, d):
    from glabcmcmc_amd import distribution
    rng = np.random.default_rng(K + d)
    return distribution.GaussianMixture(K, d, loc=rng.standard_normal((K, d)), scale=0.5 + rng.random((K, d)))


def test_glmala_dispatch_takes_a_mixture_where_the_kernels_do():
    """GLMALA.py's path="auto" decision (GLMALA.fused_dispatch): fused for a GaussianMixture of the Model's dimension on the |theta| +
    noise Model at theta_dim 1..4 and batch size 1..16; the callback path at theta_dim 5, batch size 17, with a Gamma prior, on g-and-k,
    on a CompiledModel and with a mixture of the wrong dimension.  What it answered for a glabc_dist proposal is unchanged."""
    import importlib
    from glabcmcmc_amd import compiled, generic
    from glabcmcmc_amd.examples.GK import GK_set
    GLMALA = importlib.import_module("glabcmcmc_amd.GLMALA")
    y_obs = [1.5, 0.8, 1.0, 0.5, 1.2]
    for d in (1, 2, 3, 4):
        m = AbsGaussModel(0.3, y_obs[:d])
        for N in range(1, 17):
            assert GLMALA.fused_dispatch(m, _mixture(3, d), N) is True, (d, N)
        assert GLMALA.fused_dispatch(m, _mixture(8, d), 5) is True
        assert GLMALA.fused_dispatch(m, _mixture(3, d), 17) is False
        assert GLMALA.fused_dispatch(m, _mixture(3, d), 0) is False
        assert GLMALA.fused_dispatch(m, _mixture(3, d % 4 + 1), 5) is False             # a mixture of another dimension
        assert GLMALA.fused_dispatch(m, make_dist(("gauss", [0.0] * d, [1.0] * d)), 5) is True
        assert GLMALA.fused_dispatch(m, make_dist(("uniform", [-3.0] * d, [3.0] * d)), 16) is True
        assert GLMALA.fused_dispatch(m, make_dist(("gauss", [0.0] * d, [1.0] * d)), 17) is False
    m5 = AbsGaussModel(0.3, y_obs)
    assert GLMALA.fused_dispatch(m5, _mixture(3, 5), 5) is False
    assert GLMALA.fused_dispatch(m5, make_dist(("gauss", [0.0] * 5, [1.0] * 5)), 5) is False
    mg = AbsGaussModel(0.3, y_obs[:2])
    mg._prior = lambda: make_dist(("gamma", [2.0, 2.0], [1.0, 1.0]))
    assert mg.descriptor().prior.kind == A.DIST_GAMMA
    assert GLMALA.fused_dispatch(mg, _mixture(3, 2), 5) is False
    assert GLMALA.fused_dispatch(GK_set(1.0), _mixture(3, 4), 5) is False
    assert GLMALA.fused_dispatch(GK_set(1.0), make_dist(("gauss", [0.0] * 4, [1.0] * 4)), 5) is False
    cm = compiled.CompiledModel.__new__(compiled.CompiledModel)                            # a descriptor is all the decision reads
    desc = AbsGaussModel(0.3, y_obs[:2]).descriptor()
    desc.sim_kind = A.SIM_USER
    cm.descriptor = lambda: desc
    cm.user_prior = False
    assert hasattr(cm, "program")
    assert GLMALA.fused_dispatch(cm, _mixture(3, 2), 5) is False
    assert GLMALA.fused_dispatch(cm, make_dist(("gauss", [0.0] * 2, [1.0] * 2)), 5) is False
    # fused_supported's answers to its existing callers: a sample
    m2, lp, dg = AbsGaussModel(0.3, y_obs[:2]), make_dist(("gauss", [0.0] * 2, [0.3] * 2)), make_dist(("gauss", [0.0] * 2, [1.0] * 2))
    mix2 = _mixture(3, 2)
    assert generic.fused_supported(m2, (mix2,), 5, max_dim=4) is False                   # GLMALA's call before this entry point
    assert generic.fused_supported(m2, (mix2,), 5, max_dim=4, mixture_ok=True) is False  # a single proposal without mixture_single
    assert generic.fused_supported(m2, (lp, mix2), 5, mixture_ok=True) is True
    assert generic.fused_supported(m2, (lp, mix2), 5) is False
    assert generic.fused_supported(m2, (lp, mix2), 17, mixture_ok=True) is False
    assert generic.fused_supported(m2, (lp, mix2), 17, A.MAX_BATCH_WIDE, mixture_ok=True, mixture_max_batch=A.MAX_BATCH_WIDE) is True
    assert generic.fused_supported(m2, (mix2, lp), 5, mixture_ok=True) is False          # a mixture as the local increment
    assert generic.fused_supported(mg, (lp, mix2), 5, mixture_ok=True, gamma_ok=True) is False
    assert generic.fused_supported(GK_set(1.0), (make_dist(("gauss", [0.0] * 4, [0.1] * 4)), _mixture(3, 4)), 5, mixture_ok=True) is True
    assert generic.fused_supported(m2, (lp, dg), 5) is True and generic.fused_supported(m2, (lp, dg), 17) is False
    assert generic.fused_supported(m5, (dg,), 5, max_dim=4) is False
    assert generic.fused_supported(m2, (dg,), 16, max_dim=4) is True


# ------------------------------------------------------------------------------------------ (d) the binding against the header
def test_binding_of_glabc_glmala_mix_steps_matches_the_header():
    header = open(os.path.join(ROOT, "include", "glabc.h")).read()
    m = re.search(r"^int\s+glabc_glmala_mix_steps\s*\(([^;]*)\)\s*;", header, flags=re.M)
    assert m, "include/glabc.h does not declare glabc_glmala_mix_steps"
    params = [re.sub(r"\s+", " ", p).strip() for p in m.group(1).split(",")]
    types = [re.sub(r"\s*\w+$", "", p) for p in params]                     # drop the parameter's name
    by_type = {"const glabc_model*": A.Model, "const glabc_mixture*": A.Mixture, "const glabc_mala*": A.Mala,
               "const glabc_chains*": A.Chains, "const glabc_run*": A.Run}
    assert types == ["const glabc_model*", "const glabc_mixture*", "const glabc_mala*", "const glabc_chains*", "const glabc_run*", "void*"]
    res, args = A.ENTRY_POINTS["glabc_glmala_mix_steps"]
    assert res is C.c_int and len(args) == len(types)
    for t, a in zip(types[:-1], args[:-1]):
        assert a is C.POINTER(by_type[t]), (t, a)
    assert args[-1] is C.c_void_p
    # ... and it is glabc_glmala_steps' with the mixture where that takes a glabc_dist
    _, base = A.ENTRY_POINTS["glabc_glmala_steps"]
    assert [a for i, a in enumerate(args) if i != 1] == [a for i, a in enumerate(base) if i != 1]
    assert base[1] is C.POINTER(A.Dist) and args[1] is C.POINTER(A.Mixture)
