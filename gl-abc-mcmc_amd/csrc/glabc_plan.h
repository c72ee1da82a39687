// glabc_plan.h -- which kernel a glabc_glmcmc_steps / glabc_globalmcmc_steps / glabc_rtc_steps call launches, decided in one
// pure function of plain integers (no HIP, no environment, no pointers): plan_launch.  run_sampler (glabc_hip.hip) and
// glabc_rtc_steps (glabc_rtc.hip) fill a PlanIn from their checked arguments and launch what the plan names; DESIGN.md 4.0 has
// the rules as a table, tests/test_launch_plan.py holds this function to it.  Geometry only: results never depend on the plan.
#pragma once

#include "../../include/glabc.h"
#include "glabc_geometry.h"

namespace glabc {

enum PlanKind {
    PLAN_REFUSED = 0,              // no kernel for this configuration: return LaunchPlan::status
    PLAN_LANES,                    // sampler_kernel, `lanes` lanes per chain
    PLAN_TEAM,                     // team_sampler_kernel, `waves` wavefronts per 64 chains
    PLAN_GLOBAL_TEAM,              // global_team_kernel, `waves` wavefronts per 64 chains
    PLAN_WIDE                      // wide_kernel, a group of `lanes` lanes per chain
};

struct LaunchPlan {
    int kind;                      // PlanKind
    int status;                    // PLAN_REFUSED: the GLABC_ERR_* to return, else GLABC_OK
    int waves;                     // team kinds: wavefronts per 64 chains
    int lanes;                     // PLAN_LANES: 1 / 2 / 4;  PLAN_WIDE: 8 / 16 / 32 / 64
    int ilp;                       // PLAN_LANES: the max-ilp objects (1) or the default schedule (0)
    int prio;                      // team kinds: s_setprio level of the main wavefront
};

// A tuning override from the environment (execution strategy only).  Set and unset are distinct: GLABC_TEAM_WAVES=0 clamps to 2.
struct PlanKnob {
    int set, value;
};

struct PlanIn {
    int algo;                      // GLABC_ALGO_GLMCMC / GLABC_ALGO_GLOBALMCMC
    int theta_dim, y_dim;
    int gk;                        // the g-and-k simulator (theta_dim 4, y_dim 8)
    int gamma;                     // a Gamma prior / importance proposal
    int fast;                      // GLABC_MATH_FAST
    int tape;                      // replayed random numbers
    int debug_flags, lanes_per_chain, batch_size;      // of glabc_run, checked by the caller
    int64_t n_chains;
    PlanKnob team_waves, team_prio;                     // GLABC_TEAM_WAVES, GLABC_TEAM_PRIO
    // a run-time compiled program (glabc_rtc.hip): which of its kernels exist, and the lanes per chain its entry was compiled for
    int rtc, rtc_team2, rtc_team3, rtc_gteam, rtc_lanes;
};

constexpr LaunchPlan plan_of(int kind, int waves, int lanes, int ilp, int prio) { return LaunchPlan{kind, GLABC_OK, waves, lanes, ilp, prio}; }
constexpr LaunchPlan plan_refused(int status) { return LaunchPlan{PLAN_REFUSED, status, 0, 0, 0, 0}; }

constexpr LaunchPlan plan_launch(const PlanIn& in)
{
    const bool glmcmc = in.algo == GLABC_ALGO_GLMCMC;
    const bool low = in.gk || (in.theta_dim >= 1 && in.theta_dim <= 4);      // where team, wide and max-ilp instantiations exist
    const int N = in.batch_size;
    if (!in.rtc && !in.gk && (in.theta_dim < 1 || in.theta_dim > GLABC_MAX_DIM)) return plan_refused(GLABC_ERR_DIM);

    // Lane groups: every batch size the register kernels do not hold
    if (glmcmc && N > GLABC_MAX_BATCH) {
        if (!in.rtc && !low) return plan_refused(GLABC_ERR_DIM);
        return plan_of(PLAN_WIDE, 0, in.lanes_per_chain ? in.lanes_per_chain : wide_default_lanes(N), 0, 0);
    }

    // Teams serve the launches that would otherwise leave the SIMDs with at most two wavefronts of sampler_kernel each -- 16 384
    // to 131 072 chains -- when the caller leaves the geometry to the library.  GLABC_DEBUG_TEAM opens that window for any
    // launch, GLABC_DEBUG_NO_TEAM closes it and wins; GLABC_MATH_FAST exists as team kernels only and ignores all three.
    const bool window = in.lanes_per_chain == 0 && in.n_chains >= 64 * 256 && in.n_chains <= 2 * 1024 * 64;
    const bool team_wanted = in.fast || (!(in.debug_flags & GLABC_DEBUG_NO_TEAM) && ((in.debug_flags & GLABC_DEBUG_TEAM) || window));
    // wavefronts per 64 chains: enough for about three wavefronts per SIMD (1024 SIMDs)
    const int by_size = (in.n_chains + 63) / 64 <= 1024 ? 3 : 2;

    if (in.rtc) {                  // a program holds the kernels it was compiled with: GLABC_TEAM_WAVES / _PRIO do not reach it
        if (glmcmc && team_wanted) {
            const bool have[4] = {false, false, in.rtc_team2 != 0, in.rtc_team3 != 0};
            const int nw = have[by_size] ? by_size : have[2] ? 2 : have[3] ? 3 : 0;
            if (nw) return plan_of(PLAN_TEAM, nw, 0, 0, 1);
        }
        if (!glmcmc && team_wanted && in.rtc_gteam) return plan_of(PLAN_GLOBAL_TEAM, 2, 0, 0, 1);
        return plan_of(PLAN_LANES, 0, in.rtc_lanes, 0, 0);
    }

    const int waves_knob = in.team_waves.value < 2 ? 2 : in.team_waves.value > 4 ? 4 : in.team_waves.value;
    if (glmcmc && team_wanted && !in.tape) {
        // the main wavefront carries the serial part of an iteration: s_setprio 1
        const int prio = !in.team_prio.set ? 1 : in.team_prio.value < 0 ? 0 : in.team_prio.value > 3 ? 3 : in.team_prio.value;
        // the wanted size, or fewer wavefronts when the batch is too small to split that far or the helpers' candidates
        // exceed the LDS budget; the Gamma and the fast variants are instantiated for two and three wavefronts
        for (int nw = in.team_waves.set ? waves_knob : by_size; low && nw >= 2; --nw)
            if (team_config_ok(in.theta_dim, in.y_dim, N, nw) && (nw <= 3 || !(in.gamma || in.fast))) return plan_of(PLAN_TEAM, nw, 0, 0, prio);
        if (in.fast) return plan_refused(GLABC_ERR_ARG);            // no team kernel, and nothing else computes in fast arithmetic
    }
    // GlobalMCMC: two wavefronts (three -- the helper's work split once more -- measured slower: 1.22 against 1.17 ms)
    if (!glmcmc && team_wanted && !in.tape && !in.gamma && low)
        return plan_of(PLAN_GLOBAL_TEAM, in.team_waves.set && in.team_waves.value >= 3 ? 3 : 2, 0, 0, 1);

    // sampler_kernel.  theta_dim 5..8: a lane keeps (2 theta_dim + 4) registers per candidate, so the candidates are dealt to
    // 2 / 4 lanes as soon as there are that many (the arrays would leave the registers otherwise)
    const int picked = (glmcmc && !in.tape && !in.gamma) ? pick_lanes(in.lanes_per_chain, N, in.n_chains) : 1;
    const int lanes = low ? picked : (!glmcmc || in.tape) ? 1 : in.lanes_per_chain ? picked : (N >= 3 ? 4 : N);
    // Two builds of the same kernels: up to two waves per SIMD (131 072 lanes on this part) a launch is latency-bound and runs
    // the max-ilp schedule (217 VGPRs, 6 % faster at 65 536 chains); larger launches need the occupancy of the default schedule
    // (126 VGPRs).  The tape and Gamma variants, lane groups, g-and-k and theta_dim 5..8 exist in the default objects only.
    const bool ilp = lanes == 1 && low && !in.gk && !in.tape && !in.gamma && in.n_chains <= 2 * 1024 * 64 &&
                     !(in.debug_flags & GLABC_DEBUG_DEFAULT_SCHEDULE);
    return plan_of(PLAN_LANES, 0, lanes, ilp ? 1 : 0, 0);
}

}  // namespace glabc
