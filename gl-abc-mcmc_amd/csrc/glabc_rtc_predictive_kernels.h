// glabc_rtc_predictive_kernels.h -- which kernels a run-time compiled PREDICTIVE program (glabc_rtc_compile_predictive, glabc_rtc.hip)
// holds, as a pure function of its shape: predictive_kernel (glabc_predictive.h) around the user's source, and the two row kernels every
// program holds.  No sampler and no draw kernel.  The pair of glabc_rtc_draws_kernels.h for these programs: rtc_predictive_kernels says
// for every slot whether the shape has it, whether its absence is an error, its name expression and its #define;
// rtc_predictive_defines writes the translation unit's #define block.  The entry point names the kernel (glabc_rtc_predictive_draws /
// glabc_rtc_predictive_counts, one kernel for both): no launch plan maps to these slots.  Host only, no HIP, never handed to hiprtc.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <string>

#include "glabc_rtc_kernels.h"

namespace glabc {

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

// In the order the name expressions are handed to hiprtc
enum RtcPredictiveSlot {
    RTC_PRED_KERNEL,                                       // predictive_kernel<D, YD, RTC_PRED_ROWS>
    RTC_PRED_SIMULATE_ROWS, RTC_PRED_MODEL_ROWS,           // the extern "C" row kernels
    RTC_PRED_SLOTS
};

struct RtcPredictiveKernels {
    RtcKernel k[RTC_PRED_SLOTS];
};

// Of the shape, theta_dim, y_dim and noise_dim are read: a predictive program has no algorithm, batch size or lane count, never
// evaluates a prior (theta comes from the history) and takes the user's discrepancy as the draw kernels do
inline RtcPredictiveKernels rtc_predictive_kernels(const RtcShape& s, int rows = RTC_PRED_ROWS)
{
    RtcPredictiveKernels t;
    char name[160];
    std::snprintf(name, sizeof name, "glabc::predictive_kernel<%d, %d, %d>", s.theta_dim, s.y_dim, rows);
    t.k[RTC_PRED_KERNEL] = RtcKernel{true, true, true, "GLABC_RTC_PREDICTIVE", name};
    t.k[RTC_PRED_SIMULATE_ROWS] = RtcKernel{true, true, false, nullptr, "glabc_rtc_simulate_rows"};
    t.k[RTC_PRED_MODEL_ROWS] = RtcKernel{true, true, false, nullptr, "glabc_rtc_model_rows_kernel"};
    return t;
}

// The configuration's #define block of the translation unit: the dimensions and the simulator's macros as every program has them,
// and the lines that make glabc_rtc_kernel.h instantiate the predictive kernel, at `rows` rows per item, instead of a sampler
inline std::string rtc_predictive_defines(const RtcShape& s, const RtcPredictiveKernels&, int rows = RTC_PRED_ROWS)
{
    char text[640];
    std::snprintf(text, sizeof text, "#define GLABC_RTC_PREDICTIVE 1\n#define GLABC_RTC_PRED_ROWS %d\n#define GLABC_RTC_D %d\n"
                  "#define GLABC_RTC_YD %d\n#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM %d\n#define GLABC_THETA_DIM %d\n"
                  "#define GLABC_Y_DIM %d\n#define GLABC_NOISE_DIM %d\n#define GLABC_SIMULATOR static __device__ __forceinline__\n",
                  rows, s.theta_dim, s.y_dim, s.noise_dim, s.theta_dim, s.y_dim, s.noise_dim);
    return text;
}

}  // namespace glabc
