// glabc_abc.h -- abc_draws_kernel<D, YD>: the kernel of plain rejection ABC, as glabc_abc.hip instantiates it for the built-in
// simulators (glabc_abc_draws) and as hiprtc instantiates it around a user's simulator (glabc_rtc_compile_draws, glabc_rtc_kernel.h).
// include/glabc.h holds the specification of a draw.  No host includes: the header is handed to hiprtc as text.
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
#include "glabc_forward.h"

namespace glabc {

constexpr int ABC_BLOCK = 256;
constexpr int64_t ABC_MAX_LAUNCH = (int64_t)1 << 30;          // draws per launch: the grid stays far inside 32 bits

template <int D, int YD>
struct AbcArgs {
    StepArgs<D, YD> s;            // the Model as the samplers' kernels see it: prior, simulator, y_obs, kern_scale
    const int64_t* ids;           // NULL: draw r has id row0 + r
    int64_t row0, first, n, stride;                             // this launch covers draws first .. n - 1
    uint32_t prior_lo, prior_hi, noise_lo, noise_hi, accept_lo, accept_hi;      // the three Philox keys
    float* theta;
    float* y;
    float* dis;
    uint8_t* accept;
};

// The Model's own kernel relative to its mode, K(dis) / K(0): calculate_log_kernel_dis, Mixture.py:38-45.  A user's kernel
// (GLABC_USER_KERNEL, run-time compiled builds) has no closed form to cancel: the ratio is formed from its two logarithms, as the
// generic paths of rejection.py and smc.py form it
template <int D, int YD>
GLABC_DEV float draw_accept_probability(const StepArgs<D, YD>& m, float dis)
{
#ifdef GLABC_USER_KERNEL
    return glabc_expf(model_log_kernel_of(dis, m.kern_scale, m.kern_log_scale, m.kern_c0) -
                      model_log_kernel_of(0.0f, m.kern_scale, m.kern_log_scale, m.kern_c0));
#else
    const float q = (dis - 0.0f) / m.kern_scale;
    return glabc_expf(-(0.5f * (q * q)));
#endif
}

template <int D, int YD>
__global__ void __launch_bounds__(ABC_BLOCK) abc_draws_kernel(const AbcArgs<D, YD> a)
{
    const int64_t r = a.first + (int64_t)blockIdx.x * ABC_BLOCK + threadIdx.x;
    if (r >= a.n) return;
    const uint64_t id = (uint64_t)(a.ids ? a.ids[r] : a.row0 + r);
    const uint32_t id_lo = (uint32_t)id, id_hi = (uint32_t)(id >> 32);

    // theta: row id of glabc_dist_forward(prior), through the function its kernel draws with (glabc_forward.h)
    float e[4 * ((D + 3) / 4)], theta[D];
    dist_forward_variates<D>(a.s.prior, id, a.prior_lo, a.prior_hi, e);
#pragma unroll
    for (int j = 0; j < D; ++j) theta[j] = a.s.prior.p0[j] + a.s.prior.p2[j] * e[j];       // distribution.py:170 / :77
    if (a.theta) {
#pragma unroll
        for (int j = 0; j < D; ++j) a.theta[(int64_t)j * a.stride + r] = theta[j];
    }
    if (!a.y && !a.dis && !a.accept) return;

    // y: glabc_model_simulate(eps = NULL) under the noise key -- normal j is word pair (2j, 2j + 1) of the blocks (id, 0, b); a user's
    // simulator (run-time compiled builds) declares how many it reads, the built-in ones read y_dim
    constexpr int ND = NoiseDim<YD>::value, NYB = (ND + 3) / 4;
    float nrm[4 * NYB], eps[ND], y[YD];
#pragma unroll
    for (int b = 0; b < NYB; ++b) {
        const glabc_u32x4 w = glabc_philox4x32_10(id_lo, id_hi, 0u, (uint32_t)b, a.noise_lo, a.noise_hi);
        glabc_normal_pair(w.v[0], w.v[1], &nrm[4 * b], &nrm[4 * b + 1]);
        glabc_normal_pair(w.v[2], w.v[3], &nrm[4 * b + 2], &nrm[4 * b + 3]);
    }
#pragma unroll
    for (int j = 0; j < ND; ++j) eps[j] = nrm[j];
    model_simulate<D, YD>(a.s, theta, eps, y);
    if (a.y) {
#pragma unroll
        for (int j = 0; j < YD; ++j) a.y[(int64_t)j * a.stride + r] = y[j];
    }
    if (!a.dis && !a.accept) return;

    const float dis = model_discrepancy_rows<YD>(y, a.s.y_obs);
    if (a.dis) a.dis[r] = dis;
    if (!a.accept) return;

    const glabc_u32x4 w = glabc_philox4x32_10(id_lo, id_hi, 0u, 0u, a.accept_lo, a.accept_hi);
    const float u = glabc_uniform_f32(w.v[0]);
    const float p = draw_accept_probability<D, YD>(a.s, dis);
    a.accept[r] = u < p ? (uint8_t)1 : (uint8_t)0;              // a NaN distance: p is NaN, the comparison false
}

}  // namespace glabc
