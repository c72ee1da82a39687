// glabc_abc.hip -- plain rejection ABC: glabc_abc_draws of include/glabc.h, which holds the specification of a draw.
//
// abc_draws_kernel<D, YD>.  One lane owns one draw and keeps it in registers from the prior draw to the distance: theta through
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
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "glabc_check.h"
#include "glabc_device.h"
#include "glabc_dispatch.h"
#include "glabc_forward.h"
#include "glabc_launch.h"
#include "glabc_pack.h"

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

    // y: glabc_model_simulate(eps = NULL) under the noise key -- normal j is word pair (2j, 2j + 1) of the blocks (id, 0, b)
    constexpr int NYB = (YD + 3) / 4;
    float nrm[4 * NYB], eps[YD], y[YD];
#pragma unroll
    for (int b = 0; b < NYB; ++b) {
        const glabc_u32x4 w = glabc_philox4x32_10(id_lo, id_hi, 0u, (uint32_t)b, a.noise_lo, a.noise_hi);
        glabc_normal_pair(w.v[0], w.v[1], &nrm[4 * b], &nrm[4 * b + 1]);
        glabc_normal_pair(w.v[2], w.v[3], &nrm[4 * b + 2], &nrm[4 * b + 3]);
    }
#pragma unroll
    for (int j = 0; j < YD; ++j) eps[j] = nrm[j];
    model_simulate<D, YD>(a.s, theta, eps, y);
    if (a.y) {
#pragma unroll
        for (int j = 0; j < YD; ++j) a.y[(int64_t)j * a.stride + r] = y[j];
    }
    if (!a.dis && !a.accept) return;

    const float dis = model_discrepancy_rows<YD>(y, a.s.y_obs);
    if (a.dis) a.dis[r] = dis;
    if (!a.accept) return;

    // the Model's own kernel relative to its mode, K(dis) / K(0): calculate_log_kernel_dis, Mixture.py:38-45
    const glabc_u32x4 w = glabc_philox4x32_10(id_lo, id_hi, 0u, 0u, a.accept_lo, a.accept_hi);
    const float u = glabc_uniform_f32(w.v[0]);
    const float q = (dis - 0.0f) / a.s.kern_scale;
    const float p = glabc_expf(-(0.5f * (q * q)));
    a.accept[r] = u < p ? (uint8_t)1 : (uint8_t)0;              // a NaN distance: p is NaN, the comparison false
}

template <int D, int YD>
inline int launch_abc(const glabc_model* m, uint64_t seed, int64_t row0, const int64_t* ids, int64_t n, int64_t stride, float* theta,
                      float* y, float* dis, uint8_t* accept, hipStream_t s)
{
    glabc_chains none;
    std::memset(&none, 0, sizeof none);
    AbcArgs<D, YD> a;
    std::memset(&a, 0, sizeof a);
    a.s = pack_args_rinv<D, YD>(m, nullptr, &m->prior, &none, nullptr, 0.0f);
    a.ids = ids;
    a.row0 = row0, a.n = n, a.stride = stride;
    const uint64_t kn = seed ^ GLABC_ABC_NOISE_KEY, ka = seed ^ GLABC_ABC_ACCEPT_KEY;
    a.prior_lo = (uint32_t)seed, a.prior_hi = (uint32_t)(seed >> 32);
    a.noise_lo = (uint32_t)kn, a.noise_hi = (uint32_t)(kn >> 32);
    a.accept_lo = (uint32_t)ka, a.accept_hi = (uint32_t)(ka >> 32);
    a.theta = theta, a.y = y, a.dis = dis, a.accept = accept;
    for (a.first = 0; a.first < n; a.first += ABC_MAX_LAUNCH) {
        const int64_t part = n - a.first < ABC_MAX_LAUNCH ? n - a.first : ABC_MAX_LAUNCH;
        hipLaunchKernelGGL((abc_draws_kernel<D, YD>), dim3(grid_for(part, ABC_BLOCK)), dim3(ABC_BLOCK), 0, s, a);
        if (int e = launch_status()) return e;
    }
    return GLABC_OK;
}

}  // namespace glabc

using namespace glabc;

extern "C" {

__attribute__((visibility("default"))) int glabc_abc_draws(const glabc_model* model, uint64_t seed, int64_t row0, const int64_t* ids,
                                                           int64_t n, int64_t stride, float* theta_out, float* y_out, float* dis_out,
                                                           uint8_t* accept_out, void* stream)
{
    if (int e = check_abc_draws(model, row0, ids, n, stride, theta_out, y_out, dis_out, accept_out)) return e;
    if (n == 0) return GLABC_OK;
    hipStream_t s = (hipStream_t)stream;
    if (model->sim_kind == GLABC_SIM_GK)
        return launch_abc<4, 8>(model, seed, row0, ids, n, stride, theta_out, y_out, dis_out, accept_out, s);
    return dispatch_range<1, 8>(model->theta_dim, GLABC_ERR_DIM, [&](auto d) {
        constexpr int D = decltype(d)::value;
        return launch_abc<D, D>(model, seed, row0, ids, n, stride, theta_out, y_out, dis_out, accept_out, s);
    });
}

}  // extern "C"
