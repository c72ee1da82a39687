// glabc_rtc_tables.h -- the kernel tables of the run-time compiled programs that are no sampler programs: mixture
// (glabc_rtc_compile_mix / _wide_mix), draws (glabc_rtc_compile_draws), predictive (glabc_rtc_compile_predictive) and weighted
// predictive (glabc_rtc_compile_weighted_predictive).  Each kind is a slot enumeration and one function from an RtcShape to an
// RtcKernels (glabc_rtc_kernels.h, which has the types, the shared pieces and the sampler programs); its entry points name the
// kernel to launch, no launch plan maps to these slots.  Host only, no HIP, never handed to hiprtc; tests/test_rtc_mix_kernels.py and
// tests/test_rtc_tables.py hold the tables to hand-written ones.
#pragma once

#include <cstdlib>
#include <string>

#include "glabc_rtc_kernels.h"

namespace glabc {

// Each enumeration in the order the name expressions are handed to hiprtc
// a mixture program (glabc_rtc_compile_mix / _wide_mix)
enum RtcMixSlot {
    RTC_MIX_ENTRY,                                         // sampler_kernel<.., 1, VAR_MIX, 0>
    RTC_MIX_WIDE,                                          // wide_kernel<.., WIDE_LANES[k], false, true> at RTC_MIX_WIDE + k
    RTC_MIX_SIMULATE_ROWS = RTC_MIX_WIDE + 4, RTC_MIX_MODEL_ROWS,
    RTC_MIX_SLOTS
};

// a draws program (glabc_rtc_compile_draws)
enum RtcDrawsSlot {
    RTC_DRAWS_ABC,                                         // abc_draws_kernel<D, YD>
    RTC_DRAWS_SMC,                                         // smc_draws_kernel<D, YD>
    RTC_DRAWS_SIMULATE_ROWS, RTC_DRAWS_MODEL_ROWS,
    RTC_DRAWS_SMC_FULL,                                    // smc_draws_kernel<D, YD, true> (glabc_rtc_smc_draws_full)
    RTC_DRAWS_SLOTS
};

// a predictive program (glabc_rtc_compile_predictive)
enum RtcPredictiveSlot {
    RTC_PRED_KERNEL,                                       // predictive_kernel<D, YD, rows>
    RTC_PRED_SIMULATE_ROWS, RTC_PRED_MODEL_ROWS,
    RTC_PRED_SLOTS
};

// a weighted predictive program (glabc_rtc_compile_weighted_predictive)
enum RtcWeightedPredictiveSlot {
    RTC_WPRED_KERNEL,                                      // weighted_predictive_kernel<D, YD, RTC_WEIGHTED_PRED_SEGMENTS>
    RTC_WPRED_SIMULATE_ROWS, RTC_WPRED_MODEL_ROWS,
    RTC_WPRED_SLOTS
};

static_assert((int)RTC_MIX_SLOTS <= (int)RTC_SLOTS && (int)RTC_DRAWS_SLOTS <= (int)RTC_SLOTS && (int)RTC_PRED_SLOTS <= (int)RTC_SLOTS &&
                  (int)RTC_WPRED_SLOTS <= (int)RTC_SLOTS,
              "RtcKernels::k, sized for a sampler program, holds any kind's slots");

// The GaussianMixture variant of the sampler (VAR_MIX) or of the lane-group kernel (MX) at every lane count.  shape.lanes, .gamma
// and .hooks are not read: a mixture program runs one lane per chain (chain_step asserts it for VAR_MIX), knows no Gamma, and takes
// the user's hooks as the generic kernels do.  Its block: that of a one-lane sampler program of the same shape, and the line that
// makes glabc_rtc_kernel.h instantiate the mixture kernels instead of the generic ones
inline RtcKernels rtc_mix_kernels(const RtcShape& s)
{
    RtcKernels t = rtc_new_table(RTC_MIX_SLOTS, RTC_MIX_SIMULATE_ROWS, RTC_MIX_MODEL_ROWS, RTC_MIX_WIDE, 4);
    auto add = [&t](int slot, const char* format, auto... values) {
        t.k[slot] = RtcKernel{true, true, true, "GLABC_RTC_WITH_MIX", rtc_text(format, values...)};
    };
    const int A = s.algo == GLABC_ALGO_GLMCMC ? 0 : 1, D = s.theta_dim, YD = s.y_dim;
    if (s.wide)
        for (int k = 0; k < 4; ++k) add(RTC_MIX_WIDE + k, "glabc::wide_kernel<%d, %d, %d, false, true>", D, YD, WIDE_LANES[k]);
    else
        add(RTC_MIX_ENTRY, "glabc::sampler_kernel<%d, %d, %d, %d, 1, glabc::VAR_MIX, 0>", A, D, YD, s.batch_size);
    RtcShape plain = s;
    plain.lanes = s.wide ? 0 : 1;
    plain.gamma = 0;
    t.defines = rtc_defines(plain, RtcKernels()) + "#define GLABC_RTC_WITH_MIX 1\n";
    return t;
}

// abc_draws_kernel (glabc_abc.h), smc_draws_kernel and its FULL twin (glabc_smc.h); no sampler kernel.  Of the shape, theta_dim,
// y_dim and noise_dim are read: a draws program has no algorithm, batch size or lane count, knows no Gamma, and takes the user's
// discrepancy and kernel as the generic kernels do (a user prior is refused before anything is built)
inline RtcKernels rtc_draws_kernels(const RtcShape& s)
{
    RtcKernels t = rtc_new_table(RTC_DRAWS_SLOTS, RTC_DRAWS_SIMULATE_ROWS, RTC_DRAWS_MODEL_ROWS);
    auto add = [&t](int slot, const char* format, auto... values) {
        t.k[slot] = RtcKernel{true, true, true, "GLABC_RTC_DRAWS", rtc_text(format, values...)};
    };
    add(RTC_DRAWS_ABC, "glabc::abc_draws_kernel<%d, %d>", s.theta_dim, s.y_dim);
    add(RTC_DRAWS_SMC, "glabc::smc_draws_kernel<%d, %d>", s.theta_dim, s.y_dim);
    add(RTC_DRAWS_SMC_FULL, "glabc::smc_draws_kernel<%d, %d, true>", s.theta_dim, s.y_dim);
    t.defines = "#define GLABC_RTC_DRAWS 1\n" + rtc_dimension_defines(s) + rtc_simulator_defines(s);
    return t;
}

// Rows per item of predictive_kernel in a run-time compiled program: one, whatever the source.  Every row of an item is a copy of the
// force-inlined simulator, and a user's simulator is of any size (the Lotka-Volterra example integrates 3000 RK4 steps): at the built-in
// kernels' 16 / D rows its code would stand up to 16 times in the kernel, against a 64 KB instruction cache, for the sake of loads in
// flight that a simulator of that length does not wait for, and the per-row arrays of so many live draws are no longer all kept
// in registers (the Lotka-Volterra kernel gets a private segment at R = 8 with no register spilled).  profiles/rtc_predictive_kernel_resources.txt has the compiler's figures
// at R = 1 and at 16 / D for a cheap and for an expensive source.  A draw's bits do not depend on the number.  GLABC_RTC_PRED_ROWS=1..16
// in the environment of glabc_rtc_compile_predictive forces another (a debugging knob as GLABC_RTC_LANES: what the figures were
// taken with); any other value is ignored.  The program remembers its number for the grid rule.
constexpr int RTC_PRED_ROWS = 1;

// the rows per item a compile takes: `asked` is the environment's GLABC_RTC_PRED_ROWS or null (compiled.py restates this for its self-check)
inline int rtc_predictive_rows(const char* asked)
{
    const int rows = asked ? std::atoi(asked) : RTC_PRED_ROWS;
    return rows >= 1 && rows <= 16 ? rows : RTC_PRED_ROWS;
}

// predictive_kernel (glabc_predictive.h) at `rows` rows per item; no sampler and no draw kernel, one kernel for
// glabc_rtc_predictive_draws and glabc_rtc_predictive_counts.  Of the shape, theta_dim, y_dim and noise_dim are read: a predictive
// program has no algorithm, batch size or lane count, never evaluates a prior (theta comes from the history) and takes the user's
// discrepancy as the draw kernels do
inline RtcKernels rtc_predictive_kernels(const RtcShape& s, int rows = RTC_PRED_ROWS)
{
    RtcKernels t = rtc_new_table(RTC_PRED_SLOTS, RTC_PRED_SIMULATE_ROWS, RTC_PRED_MODEL_ROWS);
    t.k[RTC_PRED_KERNEL] = RtcKernel{true, true, true, "GLABC_RTC_PREDICTIVE",
                                     rtc_text("glabc::predictive_kernel<%d, %d, %d>", s.theta_dim, s.y_dim, rows)};
    t.defines = rtc_text("#define GLABC_RTC_PREDICTIVE 1\n#define GLABC_RTC_PRED_ROWS %d\n", rows) + rtc_dimension_defines(s) +
                rtc_simulator_defines(s);
    return t;
}

// Segments per item of weighted_predictive_kernel in a run-time compiled program: one, whatever the source, for the reason given
// above for one row per item -- every segment of an item is a copy of the force-inlined simulator, and a user's simulator is of any
// size.  A draw's bits do not depend on the number.
constexpr int RTC_WEIGHTED_PRED_SEGMENTS = 1;

// weighted_predictive_kernel (glabc_weighted_predictive.h): a program kind of its own -- the predictive program, its slots, its
// compile time and its log are untouched by it.  Of the shape, theta_dim, y_dim and noise_dim are read, as for a predictive program
inline RtcKernels rtc_weighted_predictive_kernels(const RtcShape& s)
{
    RtcKernels t = rtc_new_table(RTC_WPRED_SLOTS, RTC_WPRED_SIMULATE_ROWS, RTC_WPRED_MODEL_ROWS);
    t.k[RTC_WPRED_KERNEL] = RtcKernel{true, true, true, "GLABC_RTC_WEIGHTED_PREDICTIVE",
                                      rtc_text("glabc::weighted_predictive_kernel<%d, %d, %d>", s.theta_dim, s.y_dim, RTC_WEIGHTED_PRED_SEGMENTS)};
    t.defines = rtc_text("#define GLABC_RTC_WEIGHTED_PREDICTIVE 1\n#define GLABC_RTC_WPRED_SEGMENTS %d\n", RTC_WEIGHTED_PRED_SEGMENTS) +
                rtc_dimension_defines(s) + rtc_simulator_defines(s);
    return t;
}

}  // namespace glabc
