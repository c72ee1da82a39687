"""check_rtc_mix_run (csrc/glabc_check.h): what glabc_rtc_mix_steps refuses, in the order include/glabc.h documents -- a null pointer, a
Model that is not the caller's simulator, the program's dimensions, a program built from the other kernel table, a Gamma prior, an invalid
descriptor, a tape / GLABC_MATH_FAST, the mixture's own checks as glabc_glmcmc_mix_steps makes them, the chains, the launch's batch size and
lanes, and the four checks of every stepping entry point.  A g++ driver (tests/test_arg_checks.py) under the address and
undefined-behaviour sanitizers, a stand-alone program; every row spoils a fresh valid baseline, and rows with two defects say which wins."""
from test_arg_checks import ARG, DIM, KIND, NULL, OK, check_table

GAUSS = "GLABC_DIST_DIAG_GAUSS"
# three modes in three dimensions, every field valid
MIX = ("glabc_mixture g; std::memset(&g, 0, sizeof g); g.n_modes = 3; g.dim = 3; g.c0 = -2.7568155; "
       "for (int k = 0; k < 3; ++k) { g.log_weight[k] = -1.0986123; g.cum_weight[k] = (k + 1) / 3.0; g.sum_log_scale[k] = -2.0794415; "
       "for (int q = 0; q < 3; ++q) { g.loc[k][q] = k - 1.0; g.scale[k][q] = 0.5; g.inv_scale[k][q] = 2.0; } } ")
BASE = ("b.m.sim_kind = GLABC_SIM_USER; glabc_dist lo = dist3(%s); " % GAUSS + MIX +
        "RtcShape p = {GLABC_ALGO_GLMCMC, 3, 3, 3, 5, 1, 0, 0, 0}; bool mixp = true; glabc_tape tp; std::memset(&tp, 0, sizeof tp); (void)tp; ")
CALL = "check_rtc_mix_run(p, mixp, &b.m, &lo, &g, &b.c, &b.r)"
GLOBAL = "p.algo = GLABC_ALGO_GLOBALMCMC; p.batch_size = 1; "
WIDE = "p.batch_size = 0; p.lanes = 0; p.wide = 1; b.r.batch_size = 17; "


def rows():
    out = []

    def row(spoil, want, call=CALL):
        out.append((BASE + spoil, call, want))

    def every_program(spoil, want):
        for program in ("", GLOBAL, WIDE):
            row(program + spoil, want)

    every_program("", OK)
    every_program("p.hooks = 1; p.lanes = 4;", OK)                               # neither is a matter of the launch
    # 1. null pointers, whatever else is wrong
    for call in ("check_rtc_mix_run(p, mixp, nullptr, &lo, &g, &b.c, &b.r)", "check_rtc_mix_run(p, mixp, &b.m, nullptr, &g, &b.c, &b.r)",
                 "check_rtc_mix_run(p, mixp, &b.m, &lo, nullptr, &b.c, &b.r)", "check_rtc_mix_run(p, mixp, &b.m, &lo, &g, nullptr, &b.r)",
                 "check_rtc_mix_run(p, mixp, &b.m, &lo, &g, &b.c, nullptr)"):
        row("", NULL, call)
        row("b.m.sim_kind = GLABC_SIM_GK; b.m.theta_dim = 2; mixp = false;", NULL, call)
    # 2. the caller's simulator, ahead of the dimensions
    every_program("b.m.sim_kind = GLABC_SIM_ABS_GAUSS;", KIND)
    row("b.m.sim_kind = GLABC_SIM_GK;", KIND)
    row("b.m.sim_kind = GLABC_SIM_ABS_GAUSS; b.m.theta_dim = 2;", KIND)
    # 3. the program's dimensions, ahead of the program's kind
    every_program("b.m.theta_dim = 2;", DIM)
    row("b.m.y_dim = 2;", DIM)
    row("b.m.noise.dim = 2;", DIM)
    row("b.m.noise.dim = 2; mixp = false;", DIM)
    # 4. a program built from the other table, ahead of everything the launch says
    every_program("mixp = false;", KIND)
    row("mixp = false; b.r.tape = &tp;", KIND)
    row("mixp = false; g.n_modes = 0;", KIND)
    # 5. a Gamma prior, ahead of its own validity and of the run
    every_program("b.m.prior = dist3(GLABC_DIST_GAMMA);", KIND)
    row("b.m.prior = dist3(GLABC_DIST_GAMMA); b.m.prior.p0[0] = -1.0f; b.r.tape = &tp;", KIND)
    # ... an invalid prior / local increment / kernel scale: GLABC_ERR_ARG whatever the defect
    row("b.m.prior.p2[1] = NaN;", ARG)
    row("b.m.prior.dim = 2;", ARG)
    row("lo = dist3(GLABC_DIST_GAMMA);", ARG)
    row("lo.dim = 2;", ARG)
    row("b.m.kern_scale = 0.0f;", ARG)
    row("b.m.kern_c0 = Inf;", ARG)
    # 6. a tape, GLABC_MATH_FAST, dump_draws: ahead of the mixture's dimension
    every_program("b.r.tape = &tp;", ARG)
    every_program("b.r.math_mode = GLABC_MATH_FAST;", ARG)
    row("glabc_draws_out dd; std::memset(&dd, 0, sizeof dd); b.r.dump_draws = &dd;", ARG)
    row("b.r.tape = &tp; g.dim = 2;", ARG)
    # 7. the mixture's own checks (check_mixture with the Model's theta_dim), ahead of the chains
    every_program("g.n_modes = 0;", ARG)
    row("g.n_modes = 9;", ARG)
    every_program("g.dim = 2;", DIM)
    row("g.dim = 2; b.c.theta = nullptr;", DIM)
    row("g.n_modes = 0; g.dim = 2;", ARG)                                        # n_modes before dim, as check_mixture has them
    row("g.scale[1][2] = 0.0;", ARG)
    row("g.inv_scale[0][0] = Inf;", ARG)
    row("g.loc[2][1] = NaN;", ARG)
    row("g.log_weight[0] = -Inf;", OK)                                           # a mode of weight 0
    row("g.log_weight[0] = NaN;", ARG)
    row("g.cum_weight[1] = 0.1;", ARG)                                           # not monotone
    row("g.cum_weight[2] = 1.5;", ARG)
    row("g.c0 = NaN;", ARG)
    # ... the chains: iSIR arrays for GLMCMC only
    row("b.c.theta = nullptr;", NULL)
    row("b.c.log_w = nullptr;", NULL)
    row(GLOBAL + "b.c.log_w = nullptr; b.c.flags = nullptr;", OK)
    row(WIDE + "b.c.flags = nullptr;", NULL)
    row("b.c.stride = 64;", ARG)
    row("b.c.chain0 = -1;", ARG)
    row("b.c.theta = nullptr; b.r.n_steps = -1;", NULL)
    # ... the launch: a register program takes its own batch size at one lane per chain, a wide one 17..4096 in lane groups
    every_program("b.r.n_steps = -1;", ARG)
    every_program("b.r.step0_device = b.u;", ARG)
    row("b.r.batch_size = 6;", ARG)
    row("b.r.batch_size = 17;", ARG)
    row(GLOBAL + "b.r.batch_size = 6;", OK)                                      # GlobalMCMC does not read it
    row("b.r.lanes_per_chain = 1;", OK)
    row("b.r.lanes_per_chain = 2;", ARG)
    row("b.r.lanes_per_chain = 8;", ARG)
    for n, want in ((16, ARG), (17, OK), (4096, OK), (4097, ARG)):
        row(WIDE + "b.r.batch_size = %d;" % n, want)
    for lanes, want in ((0, OK), (1, ARG), (4, ARG), (8, OK), (16, OK), (32, OK), (64, OK), (128, ARG)):
        row(WIDE + "b.r.lanes_per_chain = %d;" % lanes, want)
    row("b.r.batch_size = 6; b.r.global_frequency = NaN;", ARG)
    # 8. the four checks of every stepping entry point, in their order
    every_program("b.r.global_frequency = NaN;", ARG)
    every_program("b.r.history = b.f; b.r.hist_stride = 64;", ARG)
    row("b.r.history = b.f; b.r.hist_stride = 65;", OK)
    every_program("b.r.moments = &b.mo; b.mo.sum_jump = nullptr;", NULL)
    row("b.r.moments = &b.mo;", OK)
    every_program("b.r.step0 = 0xFFFFFFFEu;", ARG)
    row("b.r.step0 = 0xFFFFFFFCu;", OK)
    row("b.r.history = b.f; b.r.hist_stride = 64; b.r.moments = &b.mo; b.mo.sum_theta = nullptr;", ARG)      # history before moments
    row("b.r.moments = &b.mo; b.mo.sum_theta = nullptr; b.r.step0 = 0xFFFFFFFEu;", NULL)                     # moments before the counter
    return out


def test_check_rtc_mix_run(tmp_path_factory):
    check_table(tmp_path_factory, "rtc_mix", rows(), flags=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
