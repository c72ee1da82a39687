// glabc_draw.h -- what the kernels that make a draw share: abc_draws_kernel (glabc_abc.h), smc_draws_kernel (glabc_smc.h) and, for
// the noise, predictive_kernel (glabc_predictive.hip).  One text for the launch geometry, the id of a draw, its noise, the
// dimension-major stores, the acceptance and the argument fields the two draw kernels have in common, so that a draw is the same
// function of (Model, seed, id) at every entry point by construction.  No host includes: the header is handed to hiprtc as text.
//
// The noise of a draw.  The simulator's normal j is word pair (2j, 2j + 1) of the Philox blocks at counter (id_lo, id_hi, 0, b),
// b = 0 .. ceil(noise_dim / 4) - 1, under the caller's key (seed ^ GLABC_ABC_NOISE_KEY in the draw kernels, seed ^
// GLABC_PREDICTIVE_KEY in predictive_kernel), each pair through glabc_normal_pair: what glabc_model_simulate(eps = NULL) draws for
// row id.  A user's simulator (run-time compiled builds) declares how many normals it reads, the built-in ones read y_dim.
#pragma once

#include "glabc_device.h"

namespace glabc {

constexpr int DRAW_BLOCK = 256;                                // workgroups of 256 lanes, one draw per lane
constexpr int64_t DRAW_MAX_LAUNCH = (int64_t)1 << 30;          // draws per launch: the grid stays far inside 32 bits

// The fields AbcArgs and SmcArgs share, behind the Model block (and SMC's population).  A NULL output is not wanted
struct DrawArgs {
    const int64_t* ids;           // NULL: draw r has id row0 + r
    int64_t row0, first, n, stride;                             // this launch covers draws first .. n - 1
    uint32_t theta_lo, theta_hi, noise_lo, noise_hi, accept_lo, accept_hi;      // the three Philox keys; theta's: prior or proposal
    float* theta;
    float* y;
    float* dis;
    uint8_t* accept;
};

// the draw of this lane (the caller returns where it is not below d.n) and its id
GLABC_DEV int64_t draw_row(const DrawArgs& d) { return d.first + (int64_t)blockIdx.x * DRAW_BLOCK + threadIdx.x; }
GLABC_DEV uint64_t draw_id(const DrawArgs& d, int64_t r) { return (uint64_t)(d.ids ? d.ids[r] : d.row0 + r); }

// The specification is at the head of this file.  As a function of its own the block compiles to the kernels' instructions in another
// order (scalar loads earlier, a few encodings and s_nop apart); profiles/draw_header_device_code.txt has the comparison and the timings
template <int YD>
GLABC_DEV void draw_noise(uint64_t id, uint32_t key_lo, uint32_t key_hi, float (&eps)[NoiseDim<YD>::value])
{
    constexpr int ND = NoiseDim<YD>::value, NYB = (ND + 3) / 4;
    const uint32_t id_lo = (uint32_t)id, id_hi = (uint32_t)(id >> 32);
    float nrm[4 * NYB];
#pragma unroll
    for (int b = 0; b < NYB; ++b) {
        const glabc_u32x4 w = glabc_philox4x32_10(id_lo, id_hi, 0u, (uint32_t)b, key_lo, key_hi);
        glabc_normal_pair(w.v[0], w.v[1], &nrm[4 * b], &nrm[4 * b + 1]);
        glabc_normal_pair(w.v[2], w.v[3], &nrm[4 * b + 2], &nrm[4 * b + 3]);
    }
#pragma unroll
    for (int j = 0; j < ND; ++j) eps[j] = nrm[j];
}

// row r of a dimension-major output [N][stride], where it is wanted
template <int N>
GLABC_DEV void draw_store(float* out, const DrawArgs& d, int64_t r, const float (&v)[N])
{
    if (out) {
#pragma unroll
        for (int j = 0; j < N; ++j) out[(int64_t)j * d.stride + r] = v[j];
    }
}

// y: glabc_model_simulate(eps = NULL) of theta under the noise key, stored where it is wanted
template <int D, int YD>
GLABC_DEV void draw_simulate(const StepArgs<D, YD>& m, const DrawArgs& d, int64_t r, uint64_t id, const float (&theta)[D], float (&y)[YD])
{
    float eps[NoiseDim<YD>::value];
    draw_noise<YD>(id, d.noise_lo, d.noise_hi, eps);
    model_simulate<D, YD>(m, theta, eps, y);
    draw_store<YD>(d.y, d, r, y);
}

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

// The end of a draw: the distance stored, and the acceptance -- the uniform of word 0 of the Philox block (id, 0, 0) under the accept
// key against draw_accept_probability.  Its block and its exponential are skipped where accept is NULL
template <int D, int YD>
GLABC_DEV void draw_finish(const StepArgs<D, YD>& m, const DrawArgs& d, int64_t r, uint64_t id, float dis)
{
    if (d.dis) d.dis[r] = dis;
    if (!d.accept) return;
    const glabc_u32x4 w = glabc_philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), 0u, 0u, d.accept_lo, d.accept_hi);
    const float u = glabc_uniform_f32(w.v[0]);
    const float p = draw_accept_probability<D, YD>(m, dis);
    d.accept[r] = u < p ? (uint8_t)1 : (uint8_t)0;              // a NaN distance: p is NaN, the comparison false; +inf: p is 0
}

}  // namespace glabc
