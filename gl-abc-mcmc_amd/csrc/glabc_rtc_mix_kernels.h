// glabc_rtc_mix_kernels.h -- which kernels a run-time compiled MIXTURE program (glabc_rtc_compile_mix / _wide_mix, glabc_rtc.hip)
// holds, as a pure function of its shape: the GaussianMixture variant of the sampler (VAR_MIX, one lane per chain) or of the
// lane-group kernel (MX) at every lane count, and the two row kernels every program holds.  The pair of glabc_rtc_kernels.h for
// these programs: rtc_mix_kernels says for every slot whether the shape has it, whether its absence is an error, its name
// expression and its #define; rtc_mix_defines writes the translation unit's #define block.  The entry point names the kernel
// (glabc_rtc_mix_steps): no launch plan maps to these slots.  Host only, no HIP, never handed to hiprtc;
// tests/test_rtc_mix_kernels.py holds it to a hand-written table.
#pragma once

#include <cstdio>
#include <string>

#include "glabc_rtc_kernels.h"

namespace glabc {

// In the order the name expressions are handed to hiprtc
enum RtcMixSlot {
    RTC_MIX_ENTRY,                                         // sampler_kernel<.., 1, VAR_MIX, 0>
    RTC_MIX_WIDE,                                          // wide_kernel<.., WIDE_LANES[k], false, true> at RTC_MIX_WIDE + k
    RTC_MIX_SIMULATE_ROWS = RTC_MIX_WIDE + 4, RTC_MIX_MODEL_ROWS,       // the extern "C" row kernels
    RTC_MIX_SLOTS
};

struct RtcMixKernels {
    RtcKernel k[RTC_MIX_SLOTS];
};

// shape.lanes, .gamma and .hooks are not read: a mixture program runs one lane per chain (chain_step asserts it for VAR_MIX), knows
// no Gamma, and takes the user's hooks as the generic kernels do
inline RtcMixKernels rtc_mix_kernels(const RtcShape& s)
{
    RtcMixKernels t;
    auto add = [&t](int slot, const char* format, auto... values) {
        char name[160];
        std::snprintf(name, sizeof name, format, values...);
        t.k[slot] = RtcKernel{true, true, true, "GLABC_RTC_WITH_MIX", name};
    };
    t.k[RTC_MIX_SIMULATE_ROWS] = RtcKernel{true, true, false, nullptr, "glabc_rtc_simulate_rows"};
    t.k[RTC_MIX_MODEL_ROWS] = RtcKernel{true, true, false, nullptr, "glabc_rtc_model_rows_kernel"};
    const int A = s.algo == GLABC_ALGO_GLMCMC ? 0 : 1, D = s.theta_dim, YD = s.y_dim;
    if (s.wide)
        for (int k = 0; k < 4; ++k) add(RTC_MIX_WIDE + k, "glabc::wide_kernel<%d, %d, %d, false, true>", D, YD, WIDE_LANES[k]);
    else
        add(RTC_MIX_ENTRY, "glabc::sampler_kernel<%d, %d, %d, %d, 1, glabc::VAR_MIX, 0>", A, D, YD, s.batch_size);
    return t;
}

// The configuration's #define block of the translation unit: the block of a one-lane program of the same shape (rtc_defines), and
// the line that makes glabc_rtc_kernel.h instantiate the mixture kernels instead of the generic ones
inline std::string rtc_mix_defines(const RtcShape& s, const RtcMixKernels&)
{
    RtcShape plain = s;
    plain.lanes = s.wide ? 0 : 1;
    plain.gamma = 0;
    return rtc_defines(plain, RtcKernels()) + "#define GLABC_RTC_WITH_MIX 1\n";
}

}  // namespace glabc
