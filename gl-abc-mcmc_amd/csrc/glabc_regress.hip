// glabc_regress.hip -- ABC regression adjustment: the weighted second moments of the kept draws (glabc_weighted_gram) and the row-wise
// correction (glabc_regression_apply) of include/glabc.h, which holds both specifications.
//
// gram_kernel<COLS>.  The specification cuts the rows into segments of 1024 = 16 steps of 64 columns and fixes the order of every
// sum by the rows alone: column l of a segment adds its 16 rows ascending, a butterfly over the 64 columns follows.  So a wavefront
// takes a segment and lane l is column l: every load is 64 consecutive floats, the column sums are registers, and the butterfly is
// six cross-lane adds per statistic, after which every lane holds the same bits and lane 0 stores them.  COLS = y_dim + theta_dim
// is the template parameter: the kernel reads COLS columns through COLS base pointers and subtracts COLS shifts (y_obs, and 0.0 for a
// theta column: x - 0.0 is x), so it never asks which column is theta, and z and the accumulators are indexed by unrolled counters only.
// The statistics are split.  (COLS + 1)(COLS + 2) / 2 + 1 double accumulators are 154 at COLS = 16, more than a lane holds: the
// workgroup has one wavefront per slice of at most GRAM_SLICE statistics, all of them on the same segment.  The slices of a segment
// read the same rows (from cache after the first) and each owns its statistics outright; a statistic's order of additions depends on
// the rows alone, so the split is invisible in the result.  The loads of GRAM_BATCH steps are issued together.
// A row of weight 0 is skipped by a branch, not multiplied by 0: its theta and y may hold anything.  Rows past n are not loaded.
//
// gram_finish_kernel.  One workgroup, lane q adds partial[s][q] over the segments ascending, the loads of 32 segments in flight.
//
// apply_kernel<TD, YD>.  One row per lane, beta and y_obs as kernel arguments; theta_r,j is read before out_r,j is written and no lane
// reads another's row, so `out` may be `theta`.
// profiles/regress_kernel_resources.txt holds the compiler's resource report.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

#include "glabc_check.h"
#include "glabc_dispatch.h"
#include "glabc_launch.h"

namespace glabc {

constexpr int GRAM_LANES = 64;          // columns of a segment: one wavefront wide
constexpr int GRAM_STEPS = 16;          // rows per column
constexpr int GRAM_SEGMENT = GRAM_LANES * GRAM_STEPS;
static_assert(GRAM_SEGMENT == GLABC_GRAM_SEGMENT, "the segment of the specification");
constexpr int GRAM_SLICE = 32;          // statistics per wavefront, at most: 64 VGPRs of accumulators
constexpr int GRAM_BATCH = 4;           // steps whose loads are in flight together: up to 4 x 18 floats
constexpr int GRAM_MAX_COLS = 2 * GLABC_MAX_DIM;
constexpr int GRAM_FINISH_LANES = 192;  // >= the 154 statistics of 16 columns

constexpr int gram_stats(int cols) { return (cols + 1) * (cols + 2) / 2 + 1; }
constexpr int gram_slices(int cols) { return (gram_stats(cols) + GRAM_SLICE - 1) / GRAM_SLICE; }
constexpr int gram_slice_size(int cols) { return (gram_stats(cols) + gram_slices(cols) - 1) / gram_slices(cols); }
static_assert(gram_stats(GRAM_MAX_COLS) == 154 && gram_stats(GRAM_MAX_COLS) <= GRAM_FINISH_LANES, "one finishing lane per statistic");
static_assert(gram_slices(2) == 1 && gram_slices(12) == 3 && gram_slices(16) == 5 && gram_slice_size(16) == 31, "the split");

struct GramArgs {
    const float* col[GRAM_MAX_COLS];    // column c of the design after the constant: y_0 .., theta_0 ..
    double shift[GRAM_MAX_COLS];        // y_obs_k of a y column, 0.0 of a theta column
    const float* dis;
    const float* weight;
    int64_t n;
    double delta;
    int32_t kind;
    double* partial;                    // [segment][statistic]
};

// w_r of the specification from the row's distance and weight
__device__ __forceinline__ double gram_weight(const GramArgs& a, float dis, float weight)
{
    double k = 1.0;
    if (a.dis) {
        const double d = (double)dis;
        if (a.kind == GLABC_GRAM_EPANECHNIKOV) {
            const double u = d / a.delta;
            k = d <= a.delta ? 1.0 - u * u : 0.0;
        } else {
            k = d <= a.delta ? 1.0 : 0.0;
        }
    }
    return a.weight ? k * (double)weight : k;
}

// statistics SLICE * gram_slice_size .. of segment `seg`, by one wavefront
template <int COLS, int SLICE>
__device__ __forceinline__ void gram_slice(const GramArgs& a, int64_t seg, unsigned lane)
{
    constexpr int P = COLS + 1, Q = gram_stats(COLS), QS = gram_slice_size(COLS);
    constexpr int Q0 = SLICE * QS, Q1 = Q0 + QS < Q ? Q0 + QS : Q;
    double acc[QS];
#pragma unroll
    for (int i = 0; i < QS; ++i) acc[i] = 0.0;

    const int64_t row0 = seg * GRAM_SEGMENT + lane;
#pragma unroll 1
    for (int t0 = 0; t0 < GRAM_STEPS; t0 += GRAM_BATCH) {
        float x[GRAM_BATCH][COLS], dis[GRAM_BATCH], weight[GRAM_BATCH];
#pragma unroll
        for (int b = 0; b < GRAM_BATCH; ++b) {
            const int64_t r = row0 + (int64_t)(t0 + b) * GRAM_LANES;
            const bool live = r < a.n;
            dis[b] = live && a.dis ? a.dis[r] : 0.0f;
            weight[b] = live && a.weight ? a.weight[r] : 0.0f;
#pragma unroll
            for (int c = 0; c < COLS; ++c) x[b][c] = live ? a.col[c][r] : 0.0f;
        }
#pragma unroll
        for (int b = 0; b < GRAM_BATCH; ++b) {
            const int64_t r = row0 + (int64_t)(t0 + b) * GRAM_LANES;
            const double w = gram_weight(a, dis[b], weight[b]);
            if (r < a.n && w != 0.0) {                  // a NaN weight is not 0: it propagates
                double z[P];
                z[0] = 1.0;
#pragma unroll
                for (int c = 0; c < COLS; ++c) z[c + 1] = (double)x[b][c] - a.shift[c];
#pragma unroll
                for (int i = 0, q = 0; i < P; ++i) {
                    const double wz = w * z[i];
#pragma unroll
                    for (int j = i; j < P; ++j, ++q)
                        if (q >= Q0 && q < Q1) acc[q - Q0] = acc[q - Q0] + wz * z[j];
                }
                if (Q - 1 >= Q0 && Q - 1 < Q1) acc[Q - 1 - Q0] = acc[Q - 1 - Q0] + w * w;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < Q1 - Q0; ++i) {
#pragma unroll
        for (int h = 1; h < GRAM_LANES; h *= 2) acc[i] = acc[i] + __shfl_xor(acc[i], h, GRAM_LANES);
    }
    if (lane == 0) {
        double* out = a.partial + seg * Q + Q0;
#pragma unroll
        for (int i = 0; i < Q1 - Q0; ++i) out[i] = acc[i];
    }
}

template <int COLS, int... Slices>
__device__ __forceinline__ void gram_slices_of(const GramArgs& a, int64_t seg, unsigned lane, int slice, std::integer_sequence<int, Slices...>)
{
    (void)((slice == Slices && (gram_slice<COLS, Slices>(a, seg, lane), true)) || ...);
}

// grid: the segments; block: (64, gram_slices(COLS)), wavefront threadIdx.y owns slice threadIdx.y
template <int COLS>
__global__ void __launch_bounds__(GRAM_LANES* gram_slices(COLS)) gram_kernel(const GramArgs a)
{
    const int slice = __builtin_amdgcn_readfirstlane((int)threadIdx.y);          // one value per wavefront
    gram_slices_of<COLS>(a, (int64_t)blockIdx.x, threadIdx.x, slice, std::make_integer_sequence<int, gram_slices(COLS)>{});
}

__global__ void __launch_bounds__(GRAM_FINISH_LANES)
    gram_finish_kernel(const double* __restrict__ partial, int64_t n_segments, int n_stats, double* __restrict__ gram)
{
    constexpr int AHEAD = 32;           // partial sums in flight: the pass is one dependent chain of additions, bound by the loads' latency
    const int q = threadIdx.x;
    if (q >= n_stats) return;
    double g = 0.0;
    const double* p = partial + q;
    int64_t s = 0;
    for (; s + AHEAD <= n_segments; s += AHEAD) {
        double v[AHEAD];
#pragma unroll
        for (int i = 0; i < AHEAD; ++i) v[i] = p[(s + i) * n_stats];
#pragma unroll
        for (int i = 0; i < AHEAD; ++i) g = g + v[i];
    }
    for (; s < n_segments; ++s) g = g + p[s * n_stats];
    gram[q] = g;
}

// ---- the correction ----------------------------------------------------------------------------------------------------------------
constexpr int APPLY_LANES = 256;

struct ApplyArgs {
    double beta[GLABC_MAX_DIM * GLABC_MAX_DIM];         // [k * TD + j]
    double y_obs[GLABC_MAX_DIM];
};

template <int TD, int YD>
__global__ void __launch_bounds__(APPLY_LANES)
    apply_kernel(const float* theta, int64_t stride_t, const float* __restrict__ y, int64_t stride_y, int64_t n, const ApplyArgs a, float* out,
                 int64_t stride_o)
{
    const int64_t r = (int64_t)blockIdx.x * APPLY_LANES + threadIdx.x;
    if (r >= n) return;
    double dy[YD];
#pragma unroll
    for (int k = 0; k < YD; ++k) dy[k] = (double)y[k * stride_y + r] - a.y_obs[k];
#pragma unroll
    for (int j = 0; j < TD; ++j) {
        double v = (double)theta[j * stride_t + r];
#pragma unroll
        for (int k = 0; k < YD; ++k) v = v - a.beta[k * TD + j] * dy[k];
        out[j * stride_o + r] = (float)v;
    }
}

}  // namespace glabc

using namespace glabc;

extern "C" {

__attribute__((visibility("default"))) int glabc_weighted_gram(const float* theta, int64_t stride_t, int32_t theta_dim, const float* y,
                                                               int64_t stride_y, int32_t y_dim, const float* dis, const float* weight, int64_t n,
                                                               const double* y_obs, double delta, int32_t kind, double* gram, double* workspace,
                                                               void* stream)
{
    if (int e = check_weighted_gram(theta, stride_t, theta_dim, y, stride_y, y_dim, n, y_obs, delta, kind, gram, workspace)) return e;
    hipStream_t s = (hipStream_t)stream;
    const int cols = y_dim + theta_dim;
    const int64_t n_segments = (n + GRAM_SEGMENT - 1) / GRAM_SEGMENT;
    GramArgs a;
    for (int c = 0; c < GRAM_MAX_COLS; ++c) {
        a.col[c] = c < y_dim ? y + c * stride_y : c < cols ? theta + (c - y_dim) * stride_t : nullptr;
        a.shift[c] = c < y_dim ? y_obs[c] : 0.0;
    }
    a.dis = dis, a.weight = weight, a.n = n, a.delta = delta, a.kind = kind, a.partial = workspace;
    if (n_segments > 0) {
        const int rc = dispatch_range<2, GRAM_MAX_COLS>(cols, GLABC_ERR_DIM, [&](auto c) {
            constexpr int COLS = decltype(c)::value;
            hipLaunchKernelGGL((gram_kernel<COLS>), dim3((unsigned)n_segments), dim3(GRAM_LANES, gram_slices(COLS)), 0, s, a);
            return launch_status();
        });
        if (rc) return rc;
    }
    hipLaunchKernelGGL(gram_finish_kernel, dim3(1), dim3(GRAM_FINISH_LANES), 0, s, workspace, n_segments, gram_stats(cols), gram);
    return launch_status();
}

__attribute__((visibility("default"))) int glabc_regression_apply(const float* theta, int64_t stride_t, int32_t theta_dim, const float* y,
                                                                  int64_t stride_y, int32_t y_dim, int64_t n, const double* y_obs,
                                                                  const double* beta, float* out, int64_t stride_o, void* stream)
{
    if (int e = check_regression_apply(theta, stride_t, theta_dim, y, stride_y, y_dim, n, y_obs, beta, out, stride_o)) return e;
    if (n == 0) return GLABC_OK;
    hipStream_t s = (hipStream_t)stream;
    ApplyArgs a = {};
    for (int i = 0; i < y_dim * theta_dim; ++i) a.beta[i] = beta[i];
    for (int k = 0; k < y_dim; ++k) a.y_obs[k] = y_obs[k];
    return dispatch_range<1, GLABC_MAX_DIM>(theta_dim, GLABC_ERR_DIM, [&](auto td) {
        return dispatch_range<1, GLABC_MAX_DIM>(y_dim, GLABC_ERR_DIM, [&](auto yd) {
            hipLaunchKernelGGL((apply_kernel<decltype(td)::value, decltype(yd)::value>), dim3(grid_for(n, APPLY_LANES)), dim3(APPLY_LANES), 0, s,
                               theta, stride_t, y, stride_y, n, a, out, stride_o);
            return launch_status();
        });
    });
}

}  // extern "C"
