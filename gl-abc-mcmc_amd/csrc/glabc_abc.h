// glabc_abc.h -- abc_draws_kernel<D, YD>: the kernel of plain rejection ABC, as glabc_abc.hip instantiates it for the built-in
// simulators (glabc_abc_draws) and as hiprtc instantiates it around a user's simulator (glabc_rtc_compile_draws, glabc_rtc_kernel.h).
// include/glabc.h holds the specification of a draw; glabc_draw.h holds what this kernel shares with smc_draws_kernel and
// predictive_kernel (the id, the noise, the stores, the acceptance).  No host includes: the header is handed to hiprtc as text.
//
// One lane owns one draw and keeps it in registers from the prior draw to the distance: theta through
// dist_forward_variates (glabc_forward.h, what glabc_dist_forward's kernel draws with), y through model_simulate and the distance
// through model_discrepancy_rows of glabc_device.h -- the very functions the samplers and the row-wise entry points inline, which is
// what makes the bits agree with their composition -- and the acceptance through glabc_expf.  Nothing is read from memory but the id
// (when the caller lists ids); a distance-only call writes 4 bytes per draw.
// Which outputs are wanted is wave-uniform (a NULL pointer in the argument block): what only a NULL output needs is skipped on a
// scalar branch -- the simulation when only theta is asked for, the acceptance's Philox block and exponential when accept is NULL.
// Every index is 64 bits wide.  The by-value argument arrays are indexed by unrolled loop counters only, so the block stays in
// scalar registers and the kernels have no private segment (profiles/rejection_kernel_resources.txt).
// Geometry: workgroups of 256 lanes, one draw per lane.  A draw is 200 to 900 vector instructions and no load, so there is no latency
// for a second draw per lane to hide; at 16 to 50 vector registers every SIMD holds its full complement of wavefronts anyway.
#pragma once

#include "glabc_device.h"
#include "glabc_draw.h"
#include "glabc_forward.h"

namespace glabc {

template <int D, int YD>
struct AbcArgs {
    StepArgs<D, YD> s;            // the Model as the samplers' kernels see it: prior, simulator, y_obs, kern_scale
    DrawArgs d;                   // theta's key is the prior's: the seed
};

template <int D, int YD>
__global__ void __launch_bounds__(DRAW_BLOCK) abc_draws_kernel(const AbcArgs<D, YD> a)
{
    const int64_t r = draw_row(a.d);
    if (r >= a.d.n) return;
    const uint64_t id = draw_id(a.d, r);

    // theta: row id of glabc_dist_forward(prior), through the function its kernel draws with (glabc_forward.h)
    float e[4 * ((D + 3) / 4)], theta[D];
    dist_forward_variates<D>(a.s.prior, id, a.d.theta_lo, a.d.theta_hi, e);
#pragma unroll
    for (int j = 0; j < D; ++j) theta[j] = a.s.prior.p0[j] + a.s.prior.p2[j] * e[j];       // distribution.py:170 / :77
    draw_store<D>(a.d.theta, a.d, r, theta);
    if (!a.d.y && !a.d.dis && !a.d.accept) return;

    // the shared tail (glabc_draw.h): y under the noise key, the distance, the acceptance
    float y[YD];
    draw_simulate<D, YD>(a.s, a.d, r, id, theta, y);
    if (!a.d.dis && !a.d.accept) return;

    const float dis = model_discrepancy_rows<YD>(y, a.s.y_obs);
    draw_finish<D, YD>(a.s, a.d, r, id, dis);
}

}  // namespace glabc
