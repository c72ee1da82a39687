// glabc_smc.h -- smc_draws_kernel<D, YD>: the kernel of the ABC-SMC proposals, as glabc_smc.hip instantiates it for the built-in
// simulators (glabc_smc_draws) and as hiprtc instantiates it around a user's simulator (glabc_rtc_compile_draws, glabc_rtc_kernel.h).
// include/glabc.h holds the specification of a draw.  No host includes: the header is handed to hiprtc as text.
// smc_draws_kernel<D, YD, true> is the same text under a full-covariance perturbation kernel (glabc_smc_draws_full): theta through
// kde_draw_row<D, true>, the Cholesky factor behind the block (SmcFullArgs) and read after the ancestor search
// (profiles/smc_full_kernel_resources.txt).  The diagonal instantiations compile to the instructions they had before the flag.
//
// smc_draws_kernel<D, YD> is abc_draws_kernel (glabc_abc.h) with theta from a fitted population instead of the prior, the prior's
// log-density as a fifth output and the distance +inf where that is -inf; the rest is glabc_draw.h's, which both call.  One lane owns
// one draw and keeps it in registers from the ancestor to the distance: theta through kde_draw_row (glabc_kde_draw.h, what
// glabc_kde_sample's kernel draws with), the prior's log-density through dist_log_prob, y through model_simulate and the distance
// through model_discrepancy_rows of glabc_device.h -- the functions the row-wise entry points inline, which is what makes the bits
// agree with their composition.  A proposal of prior density 0 gets the distance +inf by a select, so neither acceptance rule keeps
// it and a distance-only sweep still writes 4 bytes per draw.
// What is read from memory: the id (when the caller lists ids), log2(S) + 1 words of cum_q in the ancestor search and the D
// coordinates of the ancestor.  The search is in global memory: cum_q is 8 S bytes and every lane reads it, so it sits in L2.
// Which outputs are wanted is wave-uniform (a NULL pointer in the argument block): what only a NULL output needs is skipped on a
// scalar branch.  Every index is 64 bits wide.  The by-value argument arrays are indexed by unrolled loop counters only
// (profiles/smc_kernel_resources.txt).  Geometry: workgroups of 256 lanes, one draw per lane.
#pragma once

#include "glabc_device.h"
#include "glabc_draw.h"
#include "glabc_kde_draw.h"

namespace glabc {

template <int D, int YD>
struct SmcArgs {
    StepArgs<D, YD> s;            // the Model as the samplers' kernels see it: prior, simulator, y_obs, kern_scale
    const float* x;               // the population: centres [D][S], inclusive integer prefix sums of the weights, bandwidth
    const int64_t* cum_q;
    int64_t S;
    float bw[D];
    DrawArgs d;                   // theta's key is the proposal's: the seed
    float* log_prior;
};

// The argument of smc_draws_kernel<D, YD, true> (glabc_smc_draws_full): the same fields under the same names -- `bw` is not read --
// and the lower Cholesky factor of the perturbation's covariance behind them, packed row-major (glabc_kde_draw.h)
template <int D, int YD>
struct SmcFullArgs {
    StepArgs<D, YD> s;
    const float* x;
    const int64_t* cum_q;
    int64_t S;
    float bw[D];
    DrawArgs d;
    float* log_prior;
    float chol[D * (D + 1) / 2];
};

template <int D, int YD, bool FULL>
struct SmcKernelArgs { using type = SmcArgs<D, YD>; };
template <int D, int YD>
struct SmcKernelArgs<D, YD, true> { using type = SmcFullArgs<D, YD>; };

// The Model block of the kernel's argument, read where it is used.  The compiler loads a by-value argument in the entry block and sinks
// the loads no further than the head of the ancestor search's loop: at D = 7 and 8 the prior, the noise and y_obs then live in scalar
// registers across the loop, past the 102 a wavefront has (8 spilled, seven wavefronts per SIMD).  Behind a pointer the compiler
// cannot see through, the loads are emitted after the loop.  `s` is the first member of the only argument: offset 0 of the segment
template <int D, int YD, class Args>
GLABC_DEV const StepArgs<D, YD>& model_after_search(const Args& a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(__builtin_offsetof(Args, s) == 0, "the Model block leads the argument");
    auto p = __builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return *(const StepArgs<D, YD>*)p;
#else
    return a.s;
#endif
}

// L in the same way: up to 36 more scalars at D = 8, which must not live across the search either.  kde_draw_row asks for it after
// its loop
template <int D, int YD>
struct CholAfterSearch {
    const SmcFullArgs<D, YD>& a;
    __device__ __forceinline__ const float* operator()() const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        auto p = __builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(p));
        return ((const SmcFullArgs<D, YD>*)p)->chol;
#else
        return a.chol;
#endif
    }
};

// FULL: glabc_smc_draws_full, the full-covariance perturbation of include/glabc.h; one text for both
template <int D, int YD, bool FULL = false>
__global__ void __launch_bounds__(DRAW_BLOCK) smc_draws_kernel(const typename SmcKernelArgs<D, YD, FULL>::type a)
{
    const int64_t r = draw_row(a.d);
    if (r >= a.d.n) return;
    const uint64_t id = draw_id(a.d, r);

    // theta: row id of glabc_kde_sample(population), through the function its kernel draws with (glabc_kde_draw.h)
    float theta[D], y[YD];
    if constexpr (FULL) kde_draw_row<D, true>(a.x, a.cum_q, a.S, a.bw, id, a.d.theta_lo, a.d.theta_hi, theta, CholAfterSearch<D, YD>{a});
    else kde_draw_row<D>(a.x, a.cum_q, a.S, a.bw, id, a.d.theta_lo, a.d.theta_hi, theta);
    draw_store<D>(a.d.theta, a.d, r, theta);
    if (!a.d.y && !a.d.dis && !a.log_prior && !a.d.accept) return;
    const StepArgs<D, YD>& m = model_after_search<D, YD>(a);

    // the prior's log-density: glabc_model_prior_log_prob; the distance and the acceptance need to know where it is -inf
    float lp = 0.0f;
    if (a.d.dis || a.log_prior || a.d.accept) {
        lp = dist_log_prob<D>(m.prior, theta);
        if (a.log_prior) a.log_prior[r] = lp;
    }
    if (!a.d.y && !a.d.dis && !a.d.accept) return;

    draw_simulate<D, YD>(m, a.d, r, id, theta, y);
    if (!a.d.dis && !a.d.accept) return;

    // outside the prior's support the distance is +inf: a select, so y above is still the simulated row
    const float d0 = model_discrepancy_rows<YD>(y, m.y_obs);
    draw_finish<D, YD>(m, a.d, r, id, lp == -__builtin_inff() ? __builtin_inff() : d0);
}

}  // namespace glabc
