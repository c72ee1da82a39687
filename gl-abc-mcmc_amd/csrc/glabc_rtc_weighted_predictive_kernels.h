// glabc_rtc_weighted_predictive_kernels.h -- which kernels a run-time compiled WEIGHTED PREDICTIVE program
// (glabc_rtc_compile_weighted_predictive, glabc_rtc.hip) holds, as a pure function of its shape: weighted_predictive_kernel
// (glabc_weighted_predictive.h) around the user's source, and the two row kernels every program holds.  A program kind of its own:
// the predictive program (glabc_rtc_predictive_kernels.h), its slots, its compile time and its log are untouched by it.  The pair of
// glabc_rtc_predictive_kernels.h for these programs; the entry point names the kernel (glabc_rtc_weighted_predictive_counts): no launch
// plan maps to these slots.  Host only, no HIP, never handed to hiprtc.
#pragma once

#include <cstdio>
#include <string>

#include "glabc_rtc_kernels.h"

namespace glabc {

// Segments per item of weighted_predictive_kernel in a run-time compiled program: one, whatever the source, for the reason
// glabc_rtc_predictive_kernels.h gives for one row per item -- every segment of an item is a copy of the force-inlined simulator, and
// a user's simulator is of any size.  A draw's bits do not depend on the number.
constexpr int RTC_WEIGHTED_PRED_SEGMENTS = 1;

// In the order the name expressions are handed to hiprtc
enum RtcWeightedPredictiveSlot {
    RTC_WPRED_KERNEL,                                      // weighted_predictive_kernel<D, YD, RTC_WEIGHTED_PRED_SEGMENTS>
    RTC_WPRED_SIMULATE_ROWS, RTC_WPRED_MODEL_ROWS,         // the extern "C" row kernels
    RTC_WPRED_SLOTS
};

struct RtcWeightedPredictiveKernels {
    RtcKernel k[RTC_WPRED_SLOTS];
};

// Of the shape, theta_dim, y_dim and noise_dim are read, as for a predictive program
inline RtcWeightedPredictiveKernels rtc_weighted_predictive_kernels(const RtcShape& s)
{
    RtcWeightedPredictiveKernels t;
    char name[160];
    std::snprintf(name, sizeof name, "glabc::weighted_predictive_kernel<%d, %d, %d>", s.theta_dim, s.y_dim, RTC_WEIGHTED_PRED_SEGMENTS);
    t.k[RTC_WPRED_KERNEL] = RtcKernel{true, true, true, "GLABC_RTC_WEIGHTED_PREDICTIVE", name};
    t.k[RTC_WPRED_SIMULATE_ROWS] = RtcKernel{true, true, false, nullptr, "glabc_rtc_simulate_rows"};
    t.k[RTC_WPRED_MODEL_ROWS] = RtcKernel{true, true, false, nullptr, "glabc_rtc_model_rows_kernel"};
    return t;
}

// The configuration's #define block of the translation unit: the dimensions and the simulator's macros as every program has them,
// and the lines that make glabc_rtc_kernel.h instantiate the weighted predictive kernel instead of a sampler
inline std::string rtc_weighted_predictive_defines(const RtcShape& s, const RtcWeightedPredictiveKernels&)
{
    char text[640];
    std::snprintf(text, sizeof text, "#define GLABC_RTC_WEIGHTED_PREDICTIVE 1\n#define GLABC_RTC_WPRED_SEGMENTS %d\n#define GLABC_RTC_D %d\n"
                  "#define GLABC_RTC_YD %d\n#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM %d\n#define GLABC_THETA_DIM %d\n"
                  "#define GLABC_Y_DIM %d\n#define GLABC_NOISE_DIM %d\n#define GLABC_SIMULATOR static __device__ __forceinline__\n",
                  RTC_WEIGHTED_PRED_SEGMENTS, s.theta_dim, s.y_dim, s.noise_dim, s.theta_dim, s.y_dim, s.noise_dim);
    return text;
}

}  // namespace glabc
