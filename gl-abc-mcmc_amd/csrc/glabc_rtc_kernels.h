// glabc_rtc_kernels.h -- which kernels a run-time compiled program (glabc_rtc.hip) holds, as a pure function of its shape.  A kind of
// program has one function from an RtcShape to an RtcKernels: for every slot whether the shape has it, whether its absence after the
// compile is an error, the name expression hiprtc is asked for and the #define that makes glabc_rtc_kernel.h instantiate it; which
// two slots hold the row kernels every program has; where the lane-group kernels stand; and the translation unit's #define block.
// Here: the types, the pieces every kind shares, and the sampler programs (rtc_kernels, rtc_defines; rtc_slot_for maps a launch plan
// to the slot to launch).  glabc_rtc_tables.h beside it holds the mixture, draws, predictive and weighted predictive kinds.  Host
// only, no HIP, never handed to hiprtc; tests/test_rtc_kernels.py holds it to a hand-written table, DESIGN.md 4.1g has the rules.
#pragma once

#include <cstdio>
#include <string>

#include "glabc_geometry.h"
#include "glabc_plan.h"

namespace glabc {

struct RtcShape {
    int algo, theta_dim, y_dim, noise_dim;
    int batch_size;                // GLMCMC register programs: the compiled batch size; GlobalMCMC: 1; wide programs: 0 (any of 17..4096)
    int lanes;                     // lanes per chain of the generic and unit entries (1 / 2 / 4); wide programs: 0
    int wide;                      // glabc_rtc_compile_wide: wide_kernel at every lane count instead of the register kernels
    int gamma;                     // GLABC_RTC_GAMMA: the VAR_GAMMA kernels next to the generic ones
    int hooks;                     // the source announces GLABC_USER_PRIOR, _DISCREPANCY or _KERNEL
};

// The slots of a sampler program (glabc_rtc_compile[_wide][_ex]), in the order the name expressions are handed to hiprtc.  No kind
// has more: RTC_SLOTS sizes every table
enum RtcSlot {
    RTC_ENTRY, RTC_ENTRY_UNIT, RTC_ENTRY_GAMMA,            // sampler_kernel: `lanes` lanes per chain; the Gamma entry always one
    RTC_TEAM2_GAMMA, RTC_TEAM3_GAMMA,                      // team_sampler_kernel (GLMCMC), 2 / 3 wavefronts per 64 chains
    RTC_TEAM2, RTC_TEAM2_UNIT, RTC_TEAM3, RTC_TEAM3_UNIT,
    RTC_GTEAM, RTC_GTEAM_UNIT,                             // global_team_kernel (GlobalMCMC)
    RTC_WIDE,                                              // wide_kernel<.., WIDE_LANES[k], false> at RTC_WIDE + k
    RTC_WIDE_GAMMA = RTC_WIDE + 4,                         // wide_kernel<.., WIDE_LANES[k], true> at RTC_WIDE_GAMMA + k
    RTC_SIMULATE_ROWS = RTC_WIDE_GAMMA + 4, RTC_MODEL_ROWS,       // the extern "C" row kernels
    RTC_SLOTS
};

struct RtcKernel {
    bool present = false;          // this shape has it
    bool fatal = false;            // no lowered name / module function: the compile fails; otherwise the slot stays empty
    bool lowered = false;          // `name` is a name expression (a template instantiation), not the symbol itself
    const char* define = nullptr;  // what makes glabc_rtc_kernel.h instantiate it; the unit variants follow the header's own #if
    std::string name;
};

// All a build needs of a program, by value
struct RtcKernels {
    RtcKernel k[RTC_SLOTS];        // by the kind's slot enumeration; k[n_slots..] stay absent
    int n_slots = 0;
    int wide0 = 0, n_wide = 0;     // the lane-group kernels: k[wide0 .. wide0 + n_wide)
    int simulate_rows = 0, model_rows = 0;       // the slots of the two extern "C" row kernels
    std::string defines;           // the configuration's #define block of the translation unit (glabc_rtc_kernel.h lists what it reads)
};

template <class... Values>
inline std::string rtc_text(const char* format, Values... values)
{
    char text[320];
    std::snprintf(text, sizeof text, format, values...);
    return text;
}

// an empty table of a kind's geometry, with the row kernels every program holds
inline RtcKernels rtc_new_table(int n_slots, int simulate_rows, int model_rows, int wide0 = 0, int n_wide = 0)
{
    RtcKernels t;
    t.n_slots = n_slots, t.wide0 = wide0, t.n_wide = n_wide, t.simulate_rows = simulate_rows, t.model_rows = model_rows;
    t.k[simulate_rows] = RtcKernel{true, true, false, nullptr, "glabc_rtc_simulate_rows"};
    t.k[model_rows] = RtcKernel{true, true, false, nullptr, "glabc_rtc_model_rows_kernel"};
    return t;
}

// the #define lines every kind shares: the dimensions the kernel header instantiates at ...
inline std::string rtc_dimension_defines(const RtcShape& s)
{
    return rtc_text("#define GLABC_RTC_D %d\n#define GLABC_RTC_YD %d\n", s.theta_dim, s.y_dim);
}

// ... and what the user's source and the device headers read
inline std::string rtc_simulator_defines(const RtcShape& s)
{
    return rtc_text("#define GLABC_USER_SIM 1\n#define GLABC_USER_NOISE_DIM %d\n#define GLABC_THETA_DIM %d\n#define GLABC_Y_DIM %d\n"
                    "#define GLABC_NOISE_DIM %d\n#define GLABC_SIMULATOR static __device__ __forceinline__\n", s.noise_dim, s.theta_dim, s.y_dim,
                    s.noise_dim);
}

// The #define block of a sampler program from its shape and slots; with no slot present, the block of a sampler translation unit
// that the mixture programs extend
inline std::string rtc_defines(const RtcShape& s, const RtcKernels& t)
{
    std::string defs = s.wide ? "#define GLABC_RTC_WIDE 1\n#define GLABC_RTC_ALGO 0\n" + rtc_dimension_defines(s)
                              : rtc_text("#define GLABC_RTC_L %d\n#define GLABC_RTC_ALGO %d\n", s.lanes, s.algo == GLABC_ALGO_GLMCMC ? 0 : 1) +
                                    rtc_dimension_defines(s) + rtc_text("#define GLABC_RTC_N %d\n", s.batch_size);
    defs += rtc_simulator_defines(s);
    // one line per slot that has a #define of its own (the four Gamma lane groups share the first's)
    for (int slot : {RTC_TEAM3, RTC_TEAM2, RTC_GTEAM, RTC_ENTRY_GAMMA, RTC_WIDE_GAMMA, RTC_TEAM3_GAMMA, RTC_TEAM2_GAMMA})
        if (t.k[slot].present) defs += std::string("#define ") + t.k[slot].define + " 1\n";
    return defs;
}

inline RtcKernels rtc_kernels(const RtcShape& s)
{
    RtcKernels t = rtc_new_table(RTC_SLOTS, RTC_SIMULATE_ROWS, RTC_MODEL_ROWS, RTC_WIDE, 8);
    auto add = [&t](int slot, bool fatal, const char* define, const char* format, auto... values) {
        t.k[slot] = RtcKernel{true, fatal, true, define, rtc_text(format, values...)};
    };
    const int A = s.algo == GLABC_ALGO_GLMCMC ? 0 : 1, D = s.theta_dim, YD = s.y_dim, N = s.batch_size;
    if (s.wide) {
        for (int k = 0; k < 4; ++k) {
            add(RTC_WIDE + k, true, nullptr, "glabc::wide_kernel<%d, %d, %d, false>", D, YD, WIDE_LANES[k]);
            if (s.gamma) add(RTC_WIDE_GAMMA + k, true, "GLABC_RTC_WITH_GAMMA", "glabc::wide_kernel<%d, %d, %d, true>", D, YD, WIDE_LANES[k]);
        }
    } else {
        // the unit-Gaussian variant assumes the descriptor's prior and kernel; a Gamma program does without it
        const bool unit = D == YD && !s.hooks && !s.gamma;
        add(RTC_ENTRY, true, nullptr, "glabc::sampler_kernel<%d, %d, %d, %d, %d, glabc::VAR_GENERIC, 0>", A, D, YD, N, s.lanes);
        if (unit) add(RTC_ENTRY_UNIT, false, nullptr, "glabc::sampler_kernel<%d, %d, %d, %d, %d, glabc::VAR_GAUSS_UNIT, 0>", A, D, YD, N, s.lanes);
        // the Gamma kernels run one lane per chain whatever `lanes` the generic entry gets: their teams do not depend on it either
        if (s.gamma) add(RTC_ENTRY_GAMMA, true, "GLABC_RTC_WITH_GAMMA", "glabc::sampler_kernel<%d, %d, %d, %d, 1, glabc::VAR_GAMMA, 0>", A, D, YD, N);
        // team geometry (glabc_team.h): GLMCMC, one lane per chain, where the helpers' candidates fit a workgroup's LDS budget
        for (int nw = 2; nw <= 3; ++nw) {
            if (s.algo != GLABC_ALGO_GLMCMC || !team_config_ok(D, YD, N, nw)) continue;
            const char* team = "glabc::team_sampler_kernel<%d, %d, %d, glabc::%s, %d, false>";
            if (s.gamma) add(nw == 2 ? RTC_TEAM2_GAMMA : RTC_TEAM3_GAMMA, false, nw == 2 ? "GLABC_RTC_GAMMA_TEAM2" : "GLABC_RTC_GAMMA_TEAM3", team, D, YD, N, "VAR_GAMMA", nw);
            if (s.lanes != 1) continue;
            add(nw == 2 ? RTC_TEAM2 : RTC_TEAM3, false, nw == 2 ? "GLABC_RTC_TEAM2" : "GLABC_RTC_TEAM3", team, D, YD, N, "VAR_GENERIC", nw);
            if (unit) add(nw == 2 ? RTC_TEAM2_UNIT : RTC_TEAM3_UNIT, false, nullptr, team, D, YD, N, "VAR_GAUSS_UNIT", nw);
        }
        // held by a Gamma program too, never launched for a Gamma run (rtc_slot_for)
        if (s.algo == GLABC_ALGO_GLOBALMCMC && s.lanes == 1 && global_team_lds_bytes(D, s.noise_dim) <= 48 * 1024) {
            add(RTC_GTEAM, false, "GLABC_RTC_GTEAM", "glabc::global_team_kernel<%d, %d, glabc::VAR_GENERIC, 2>", D, YD);
            if (unit) add(RTC_GTEAM_UNIT, false, nullptr, "glabc::global_team_kernel<%d, %d, glabc::VAR_GAUSS_UNIT, 2>", D, YD);
        }
    }
    t.defines = rtc_defines(s, t);
    return t;
}

// The slot a plan launches in a sampler program, or -1 where there is none.  held[slot]: converts to true where the program holds
// the slot.  A unit launch (glabc_pack.h gauss_unit_config) whose unit slot is empty runs the generic kernel; a Gamma launch never
// takes a unit slot, and has no GlobalMCMC team.
template <class Held>
inline int rtc_slot_for(const LaunchPlan& plan, bool gamma, bool unit, const Held* held)
{
    int generic = -1, unit_slot = -1, gamma_slot = -1;
    switch (plan.kind) {
    case PLAN_LANES: generic = RTC_ENTRY, unit_slot = RTC_ENTRY_UNIT, gamma_slot = RTC_ENTRY_GAMMA; break;
    case PLAN_TEAM:
        if (plan.waves == 2) generic = RTC_TEAM2, unit_slot = RTC_TEAM2_UNIT, gamma_slot = RTC_TEAM2_GAMMA;
        if (plan.waves == 3) generic = RTC_TEAM3, unit_slot = RTC_TEAM3_UNIT, gamma_slot = RTC_TEAM3_GAMMA;
        break;
    case PLAN_GLOBAL_TEAM: generic = RTC_GTEAM, unit_slot = RTC_GTEAM_UNIT; break;
    case PLAN_WIDE:
        for (int k = 0; k < 4; ++k)
            if (WIDE_LANES[k] == plan.lanes) generic = RTC_WIDE + k, gamma_slot = RTC_WIDE_GAMMA + k;
        break;
    default: break;
    }
    if (gamma) return gamma_slot;
    return (unit && unit_slot >= 0 && held[unit_slot]) ? unit_slot : generic;
}

}  // namespace glabc
