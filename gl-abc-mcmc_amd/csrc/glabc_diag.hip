// glabc_diag.hip -- chain diagnostics from a chain-major history: per-chain means and lagged autocovariances in float64
// (glabc_autocov of include/glabc.h, which holds the numerical specification).  No template over theta_dim: the coordinate is
// a grid dimension and the row step a run-time integer.
//
// Kernels
//   mean_kernel              one work-item per (chain, coordinate): S += (double) x_t ascending, m = S / n_rows
//   autocov_kernel           one work-item per (chain, coordinate, block of LAGS lags)
//
// autocov_kernel.  Lanes run along the chain index, so every load is a row segment of 256 contiguous bytes per wavefront (as in
// esjd_kernel); blockIdx.y is the coordinate; the LAG_WAVES wavefronts of a workgroup hold LAG_WAVES consecutive lag blocks of the
// same 64 chains (they walk the same rows at about the same time, so all but one of them find a row in cache) and blockIdx.z
// counts the groups of LAG_WAVES lag blocks.  A work-item of lag block k0 = LAGS * b keeps
//   acc[l], l < LAGS          the running sums A_{k0 + l}
//   w[i],   i < LAGS          the centred values u_s of the last LAGS trailing rows s = t - k0, u_s at w[s % LAGS]
// in VGPRs: 2 x 2 x LAGS registers.  The time loop is unrolled by LAGS -- as fold expressions over integer sequences, not as
// `#pragma unroll` loops, which stay rolled past the compiler's budget -- so that s % LAGS and (s - l) % LAGS are compile-time
// numbers and neither array is ever indexed by a run-time value (such an array lives in scratch).  Every step loads the leading
// value x_t and the trailing value x_{t - k0} (the same address in lag block 0), centres both and adds u_t * u_{t - k} to every
// A_k of the block, t ascending per lag: the order of the specification, whatever the launch geometry.
//   first chunk (s < LAGS):   lag offset l has a partner from row s = l on, a compile-time condition
//   last chunk:               a row past n_rows - 1 reads the last row again and every sum keeps its bits (a select, not a
//                             product with zero: 0 * inf would be NaN where the specification has no term)
//   last lag block:           sums of lags past max_lag are formed from rows inside the history and not stored
// Loads.  A row segment is read by glabc_history.h's load_segment, a buffer descriptor over exactly its bytes: one scalar base and
// one 32-bit lane offset (with 64-bit per-lane pointers the compiler keeps an induction pointer per unrolled row in VGPRs,
// 4 x LAGS of them), and nothing behind the segment can be read.  The row pointers advance by one row per load
// for the same reason: LAGS multiples of the row step would be hoisted out of the loop and spill the scalar file.  The loads of
// ROW_BATCH rows are issued together; a scheduling barrier behind every row keeps the compiler from hoisting the loads of the
// whole chunk to its top, which spills.
// LAGS = 20: 80 VGPRs of state and 20 loaded values fit under the 128 VGPRs that four wavefronts per SIMD allow (24 lags spill,
// 32 would need 128 for the two arrays alone); max_lag = 128 is 7 blocks of 20 as it is 6 of 24, the same 140-odd lag slots.
// profiles/diag_kernel_resources.txt holds the compiler's resource report.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

#include "glabc_check.h"
#include "glabc_history.h"
#include "glabc_launch.h"

namespace glabc {

constexpr int DIAG_LANES = 64;          // chains per workgroup: one wavefront wide
constexpr int LAGS = 20;                // lags per work-item
constexpr int LAG_WAVES = 4;            // lag blocks (wavefronts) per workgroup
constexpr int ROW_BATCH = 10;           // rows whose loads are issued together
static_assert(LAGS % ROW_BATCH == 0, "a chunk is a whole number of load batches");

__global__ void __launch_bounds__(DIAG_LANES) mean_kernel(const float* __restrict__ hist, int64_t n_rows, int64_t row_step,
                                                          int64_t n_chains, int64_t stride, double* __restrict__ mean_out)
{
    const int64_t c = (int64_t)blockIdx.x * DIAG_LANES + threadIdx.x;
    if (c >= n_chains) return;
    const int j = blockIdx.y;
    const float* p = hist + j * stride + c;
    double s = 0.0;
#pragma unroll 8
    for (int64_t t = 0; t < n_rows; ++t) s = s + (double)p[t * row_step];
    mean_out[j * n_chains + c] = s / (double)n_rows;
}

// row I of a chunk: the trailing value enters the ring at w[I], the leading value meets the LAGS trailing values behind it.
// FIRST: lag offset L has a partner from row L on; live == false (a row past the end, LAST chunks only): every sum keeps its bits
template <bool FIRST, bool LAST, int I, int... L>
__device__ __forceinline__ void autocov_row(float xs, float xt, bool live, double m, double (&acc)[LAGS], double (&w)[LAGS],
                                            std::integer_sequence<int, L...>)
{
    w[I] = (double)xs - m;
    const double ut = (double)xt - m;
    ((!FIRST || L <= I ? (void)(acc[L] = !LAST || live ? acc[L] + ut * w[(I - L + LAGS) % LAGS] : acc[L]) : (void)0), ...);
    __builtin_amdgcn_sched_barrier(0);
}

// rows I0 .. I0 + sizeof...(B) - 1 of a chunk, their loads first; ps / pt are left on the row behind them.  LAST: the chunk has
// rows_left < LAGS rows; the pointers stop at the last of them, so a row past it reads that row again (inside the history)
template <bool FIRST, bool LAST, int I0, int... B>
__device__ __forceinline__ void autocov_rows(const float*& ps, const float*& pt, int64_t row_step, int64_t rows_left, int row_bytes,
                                             unsigned lane, double m, double (&acc)[LAGS], double (&w)[LAGS],
                                             std::integer_sequence<int, B...>)
{
    float xs[sizeof...(B)], xt[sizeof...(B)];
    ((xs[B] = load_segment(ps, row_bytes, lane), xt[B] = load_segment(pt, row_bytes, lane),
      ps += !LAST || I0 + B + 1 < rows_left ? row_step : 0, pt += !LAST || I0 + B + 1 < rows_left ? row_step : 0), ...);
    (autocov_row<FIRST, LAST, I0 + B>(xs[B], xt[B], I0 + B < rows_left, m, acc, w, std::make_integer_sequence<int, LAGS>{}), ...);
}

// LAGS rows from trailing row s0 on.  FIRST: s0 == 0
template <bool FIRST, bool LAST, int... Q>
__device__ __forceinline__ void autocov_chunk(const float*& ps, const float*& pt, int64_t row_step, int64_t rows_left, int row_bytes,
                                              unsigned lane, double m, double (&acc)[LAGS], double (&w)[LAGS],
                                              std::integer_sequence<int, Q...>)
{
    (autocov_rows<FIRST, LAST, Q * ROW_BATCH>(ps, pt, row_step, rows_left, row_bytes, lane, m, acc, w,
                                              std::make_integer_sequence<int, ROW_BATCH>{}),
     ...);
}

__global__ void __launch_bounds__(DIAG_LANES * LAG_WAVES, 4)
    autocov_kernel(const float* __restrict__ hist, int64_t n_rows, int64_t row_step, int64_t n_chains, int64_t stride, int32_t max_lag,
                   const double* __restrict__ mean, double* __restrict__ acov_out)
{
    const int64_t c = (int64_t)blockIdx.x * DIAG_LANES + threadIdx.x;
    const int k0 = ((int)blockIdx.z * LAG_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.y)) * LAGS;
    if (c >= n_chains || k0 > max_lag) return;
    const int j = blockIdx.y;
    const int64_t theta_dim = gridDim.y;
    const double m = mean[j * n_chains + c];
    const unsigned lane = threadIdx.x;
    const int64_t chain0 = (int64_t)blockIdx.x * DIAG_LANES;
    const int row_bytes = 4 * (int)(n_chains - chain0 < DIAG_LANES ? n_chains - chain0 : DIAG_LANES);
    const float* ps = hist + j * stride + chain0;                        // trailing row s, the workgroup's segment of it
    const float* pt = ps + (int64_t)k0 * row_step;                       // leading row t = s + k0
    double acc[LAGS], w[LAGS];
#pragma unroll
    for (int l = 0; l < LAGS; ++l) acc[l] = w[l] = 0.0;
    int64_t rows_left = n_rows - k0;                                     // leading rows still to come: >= 1
    constexpr std::make_integer_sequence<int, LAGS / ROW_BATCH> batches{};
    if (rows_left >= LAGS) {
        autocov_chunk<true, false>(ps, pt, row_step, rows_left, row_bytes, lane, m, acc, w, batches);
        for (rows_left -= LAGS; rows_left >= LAGS; rows_left -= LAGS)
            autocov_chunk<false, false>(ps, pt, row_step, rows_left, row_bytes, lane, m, acc, w, batches);
        if (rows_left > 0) autocov_chunk<false, true>(ps, pt, row_step, rows_left, row_bytes, lane, m, acc, w, batches);
    } else {
        autocov_chunk<true, true>(ps, pt, row_step, rows_left, row_bytes, lane, m, acc, w, batches);
    }
    const double nd = (double)n_rows;
#pragma unroll
    for (int l = 0; l < LAGS; ++l)
        if (k0 + l <= max_lag) acov_out[((int64_t)(k0 + l) * theta_dim + j) * n_chains + c] = acc[l] / nd;
}

}  // namespace glabc

using namespace glabc;

extern "C" {

__attribute__((visibility("default"))) int glabc_autocov(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains,
                                                         int64_t stride, int32_t max_lag, double* mean_out, double* acov_out,
                                                         void* stream)
{
    if (int e = check_autocov(history, n_rows, theta_dim, n_chains, stride, max_lag, mean_out, acov_out)) return e;
    if (n_chains == 0) return GLABC_OK;
    hipStream_t s = (hipStream_t)stream;
    const int64_t row_step = (int64_t)theta_dim * stride;
    const unsigned chain_blocks = grid_for(n_chains, DIAG_LANES);
    hipLaunchKernelGGL(mean_kernel, dim3(chain_blocks, theta_dim), dim3(DIAG_LANES), 0, s, history, n_rows, row_step, n_chains, stride,
                       mean_out);
    if (int e = launch_status()) return e;
    const unsigned lag_groups = grid_for((int64_t)max_lag + 1, LAGS * LAG_WAVES);
    hipLaunchKernelGGL(autocov_kernel, dim3(chain_blocks, theta_dim, lag_groups), dim3(DIAG_LANES, LAG_WAVES), 0, s, history, n_rows,
                       row_step, n_chains, stride, max_lag, mean_out, acov_out);
    return launch_status();
}

}  // extern "C"
