// glabc_rtc_draws_kernels.h -- which kernels a run-time compiled DRAWS program (glabc_rtc_compile_draws, glabc_rtc.hip) holds, as a
// pure function of its shape: abc_draws_kernel (glabc_abc.h), smc_draws_kernel and its FULL twin (glabc_smc.h) around the
// user's source, and the two row kernels every program holds.  No sampler kernel.  The pair of glabc_rtc_kernels.h / glabc_rtc_mix_kernels.h for these programs:
// rtc_draws_kernels says for every slot whether the shape has it, whether its absence is an error, its name expression and its
// #define; rtc_draws_defines writes the translation unit's #define block.  The entry point names the kernel (glabc_rtc_abc_draws /
// glabc_rtc_smc_draws / glabc_rtc_smc_draws_full): no launch plan maps to these slots.  Host only, no HIP, never handed to hiprtc.
#pragma once

#include <cstdio>
#include <string>

#include "glabc_rtc_kernels.h"

namespace glabc {

// In the order the name expressions are handed to hiprtc
enum RtcDrawsSlot {
    RTC_DRAWS_ABC,                                         // abc_draws_kernel<D, YD>
    RTC_DRAWS_SMC,                                         // smc_draws_kernel<D, YD>
    RTC_DRAWS_SIMULATE_ROWS, RTC_DRAWS_MODEL_ROWS,         // the extern "C" row kernels
    RTC_DRAWS_SMC_FULL,                                    // smc_draws_kernel<D, YD, true> (glabc_rtc_smc_draws_full)
    RTC_DRAWS_SLOTS
};

struct RtcDrawsKernels {
    RtcKernel k[RTC_DRAWS_SLOTS];
};

// Of the shape, theta_dim, y_dim and noise_dim are read: a draws program has no algorithm, batch size or lane count, knows no Gamma,
// and takes the user's discrepancy and kernel as the generic kernels do (a user prior is refused before anything is built)
inline RtcDrawsKernels rtc_draws_kernels(const RtcShape& s)
{
    RtcDrawsKernels t;
    auto add = [&t](int slot, const char* format, auto... values) {
        char name[160];
        std::snprintf(name, sizeof name, format, values...);
        t.k[slot] = RtcKernel{true, true, true, "GLABC_RTC_DRAWS", name};
    };
    t.k[RTC_DRAWS_SIMULATE_ROWS] = RtcKernel{true, true, false, nullptr, "glabc_rtc_simulate_rows"};
    t.k[RTC_DRAWS_MODEL_ROWS] = RtcKernel{true, true, false, nullptr, "glabc_rtc_model_rows_kernel"};
    add(RTC_DRAWS_ABC, "glabc::abc_draws_kernel<%d, %d>", s.theta_dim, s.y_dim);
    add(RTC_DRAWS_SMC, "glabc::smc_draws_kernel<%d, %d>", s.theta_dim, s.y_dim);
    add(RTC_DRAWS_SMC_FULL, "glabc::smc_draws_kernel<%d, %d, true>", s.theta_dim, s.y_dim);
    return t;
}

// The configuration's #define block of the translation unit: the dimensions and the simulator's macros as every program has them,
// and the line that makes glabc_rtc_kernel.h instantiate the draw kernels instead of a sampler
inline std::string rtc_draws_defines(const RtcShape& s, const RtcDrawsKernels&)
{
    char text[600];
    std::snprintf(text, sizeof text, "#define GLABC_RTC_DRAWS 1\n#define GLABC_RTC_D %d\n#define GLABC_RTC_YD %d\n"
                  "#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM %d\n#define GLABC_THETA_DIM %d\n#define GLABC_Y_DIM %d\n"
                  "#define GLABC_NOISE_DIM %d\n#define GLABC_SIMULATOR static __device__ __forceinline__\n", s.theta_dim, s.y_dim, s.noise_dim,
                  s.theta_dim, s.y_dim, s.noise_dim);
    return text;
}

}  // namespace glabc
