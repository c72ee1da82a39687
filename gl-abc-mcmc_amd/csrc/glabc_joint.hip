// glabc_joint.hip -- the joint posterior of a chain-major history: pair histograms (glabc_histogram2d) and per-chain cross moments
// (glabc_cross_moments) of include/glabc.h, which holds both specifications.
//
// joint_kernel.  glabc_quant.hip's count_kernel with a pair of coordinates where that has one: lanes run along the chain index,
// blockIdx.y is the pair; the walk over items of 64 chains x JOINT_ROWS rows, the guarded loads, the uint32 table in LDS, the grid
// rule and glabc_histogram's bin arithmetic are glabc_history.h's, which argues what cannot be read, that a slot is inside the table
// and that no counter wraps.  An item loads the row segments of both coordinates, all 2 x JOINT_ROWS loads issued together, and a
// lane outside the segment counts nothing.  Each value is binned on its own axis (axis_bin, glabc_slots.h) and the two bins make the slot: n_bins^2 + 2
// counters.  At 128 bins the table is 65 544 bytes: past what a launch gets unasked, so the launcher has the size granted
// (glabc_lds_grant.h) as the lane-group and the flow launchers do; two workgroups share a CU then.
// Contention.  One LDS atomic per draw.  A grid of bins spreads a posterior over far more counters than a level-0 digit table
// does: folding the run of equal slots along an item's rows into one add (count_kernel's COUNT_RUNS) was measured and did not
// pay, so it is not here.
//
// cross_kernel<D>.  One work-item per chain, lanes along the chain index, every load a row segment through the same kind of
// descriptor.  Two passes over the chain's rows: the D sums of the means, then the D (D + 1) / 2 sums of products of the centred
// values -- all of them in registers (72 VGPRs at D = 8), so the history is read twice, not once per pair of coordinates, and
// each sum runs t ascending as the specification says, whatever the launch geometry.  D is a template parameter
// (glabc_dispatch.h) and every loop over coordinates is unrolled: no array is indexed by a run-time value and nothing lives in
// scratch.  The loads of CROSS_LOADS / D rows are issued together: with one wavefront per SIMD at 65 536 chains the loads in
// flight, not the arithmetic, bound the kernel.
// profiles/joint_kernel_resources.txt holds the compiler's resource report.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "glabc_check.h"
#include "glabc_dispatch.h"
#include "glabc_history.h"
#include "glabc_launch.h"
#include "glabc_lds_grant.h"
#include "glabc_slots.h"

namespace glabc {

constexpr int JOINT_ROWS = 8;           // rows per item: the 16 loads of both coordinates in flight together, as count_kernel's 16
                                        // (16 rows are 32 descriptors, more than the scalar file holds without spilling)
constexpr int64_t JOINT_MAX_ITEMS_PER_WAVE = 1 << 19;    // x HISTORY_WAVES x JOINT_ROWS x HISTORY_LANES = 2^31 draws per workgroup

__global__ void __launch_bounds__(HISTORY_LANES* HISTORY_WAVES)
    joint_kernel(const float* __restrict__ hist, int64_t n_rows, int64_t row_step, int64_t n_chains, int64_t stride, const JointSlots slots,
                 unsigned long long* __restrict__ counts)
{
    extern __shared__ uint32_t table[];
    const int n_bins = slots.n_bins;
    const int n_slots = n_bins * n_bins + 2;
    table_zero(table, n_slots);

    const int pair = blockIdx.y;
    const int ja = slots.a[pair], jb = slots.b[pair];
    const BinAxis axis_a{slots.lo[ja], slots.hi[ja], slots.scale[ja]}, axis_b{slots.lo[jb], slots.hi[jb], slots.scale[jb]};
    const unsigned lane = threadIdx.x;
    const Walk<JOINT_ROWS> walk(n_rows, n_chains);
    for (int64_t item = walk.first; item < walk.n_items; item += walk.n_waves) {
        const Item it = walk.item(item);
        const float* pa = hist + it.row0 * row_step + ja * stride + it.chain0;
        const float* pb = hist + it.row0 * row_step + jb * stride + it.chain0;
        float xa[JOINT_ROWS], xb[JOINT_ROWS];
#pragma unroll
        for (int r = 0; r < JOINT_ROWS; ++r) {
            xa[r] = load_segment(pa, it.bytes(r), lane);
            xb[r] = load_segment(pb, it.bytes(r), lane);
            pa += it.step(r, row_step);
            pb += it.step(r, row_step);
        }
        const bool inside = (int)lane < it.live;
#pragma unroll
        for (int r = 0; r < JOINT_ROWS; ++r)
            lds_add(table, inside && r < it.rows ? joint_slot(axis_bin(xa[r], axis_a, n_bins), axis_bin(xb[r], axis_b, n_bins), n_bins) : -1, 1u);
    }
    table_flush(table, n_slots, counts + (int64_t)pair * n_slots);
}

// workgroups per pair (history_grid): the part's fill is shared among the n_pairs pairs of gridDim.y
constexpr unsigned joint_grid(int64_t n_rows, int32_t n_pairs, int64_t n_chains, size_t lds_bytes)
{
    return history_grid(history_items(n_rows, n_chains, JOINT_ROWS), HISTORY_WAVES, JOINT_MAX_ITEMS_PER_WAVE,
                        (HISTORY_CUS * workgroups_per_cu(lds_bytes) + n_pairs - 1) / n_pairs);
}
// ... pinned at what joint_grid's own arithmetic gave before it called history_grid
static_assert(joint_grid(1, 1, 1, 12) == 1 && joint_grid(8, 28, 64, 65544) == 1 && joint_grid(8, 1, 7 * 64, 4104) == 1 &&
                  joint_grid(8, 1, 9 * 64, 4104) == 2, "one item, HISTORY_WAVES - 1 and + 1 items");
static_assert(joint_grid(1 << 20, 1, 65536, 65544) == 512 && joint_grid(1 << 20, 28, 65536, 65544) == 32, "128 bins, the largest table");
static_assert(joint_grid(1 << 20, 1, 65536, 4104) == 1024 && joint_grid(1 << 20, 28, 65536, 4104) == 37, "32 bins, 1 and 28 pairs");
static_assert(joint_grid(1 << 20, 3, 65536, 40008) == 342 && joint_grid(1 << 20, 3, 65536, 53832) == 256 &&
                  joint_grid(1 << 20, 3, 65536, 54764) == 171, "100, 116 and 117 bins: four, three and two workgroups per CU");
static_assert(joint_grid(1 << 18, 28, 1 << 20, 65544) == 128 && joint_grid(1 << 18, 1, 1 << 24, 4104) == 2048, "the counters' bound wins");

inline int launch_joint(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride, int32_t n_pairs,
                        const int32_t* pairs, int32_t n_bins, const double* lo, const double* hi, uint64_t* counts, hipStream_t s)
{
    const JointSlots j = joint_slots(n_pairs, pairs, n_bins, lo, hi);
    const size_t lds_bytes = ((size_t)n_bins * n_bins + 2) * sizeof(uint32_t);
    static LdsGrant grant;                               // per device
    if (!grant_dynamic_lds(grant, (const void*)joint_kernel, lds_bytes)) return GLABC_ERR_LAUNCH;
    const unsigned g = joint_grid(n_rows, n_pairs, n_chains, lds_bytes);
    hipLaunchKernelGGL(joint_kernel, dim3(g, n_pairs), dim3(HISTORY_LANES, HISTORY_WAVES), lds_bytes, s, history, n_rows,
                       (int64_t)theta_dim * stride, n_chains, stride, j, (unsigned long long*)counts);
    return launch_status();
}

// ---- cross moments ---------------------------------------------------------------------------------------------------------------
constexpr int CROSS_LANES = 64;         // chains per workgroup: one wavefront wide
constexpr int CROSS_LOADS = 32;         // loads in flight per work-item: CROSS_LOADS / D rows of D coordinates

template <int D>
__global__ void __launch_bounds__(CROSS_LANES)
    cross_kernel(const float* __restrict__ hist, int64_t n_rows, int64_t row_step, int64_t n_chains, int64_t stride,
                 double* __restrict__ mean_out, double* __restrict__ cov_out)
{
    constexpr int BATCH = CROSS_LOADS / D;
    constexpr int PAIRS = D * (D + 1) / 2;
    const unsigned lane = threadIdx.x;
    const int64_t chain0 = (int64_t)blockIdx.x * CROSS_LANES;
    const int64_t c = chain0 + lane;
    const int bytes = 4 * (int)(n_chains - chain0 < CROSS_LANES ? n_chains - chain0 : CROSS_LANES);
    const int64_t n_batched = n_rows / BATCH * BATCH;

    double m[D];
    {
        double s[D];
#pragma unroll
        for (int j = 0; j < D; ++j) s[j] = 0.0;
        const float* p = hist + chain0;
        for (int64_t t = 0; t < n_batched; t += BATCH) {
            float x[BATCH][D];
#pragma unroll
            for (int r = 0; r < BATCH; ++r) {
#pragma unroll
                for (int j = 0; j < D; ++j) x[r][j] = load_segment(p + j * stride, bytes, lane);
                p += row_step;
            }
#pragma unroll
            for (int r = 0; r < BATCH; ++r)
#pragma unroll
                for (int j = 0; j < D; ++j) s[j] = s[j] + (double)x[r][j];
        }
        for (int64_t t = n_batched; t < n_rows; ++t) {
#pragma unroll
            for (int j = 0; j < D; ++j) s[j] = s[j] + (double)load_segment(p + j * stride, bytes, lane);
            p += row_step;
        }
        const double nd = (double)n_rows;
#pragma unroll
        for (int j = 0; j < D; ++j) m[j] = s[j] / nd;
    }

    double acc[PAIRS];
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) acc[q] = 0.0;
    const float* p = hist + chain0;
    for (int64_t t = 0; t < n_batched; t += BATCH) {
        float x[BATCH][D];
#pragma unroll
        for (int r = 0; r < BATCH; ++r) {
#pragma unroll
            for (int j = 0; j < D; ++j) x[r][j] = load_segment(p + j * stride, bytes, lane);
            p += row_step;
        }
#pragma unroll
        for (int r = 0; r < BATCH; ++r) {
            double u[D];
#pragma unroll
            for (int j = 0; j < D; ++j) u[j] = (double)x[r][j] - m[j];
#pragma unroll
            for (int i = 0, q = 0; i < D; ++i)
#pragma unroll
                for (int j = i; j < D; ++j, ++q) acc[q] = acc[q] + u[i] * u[j];
        }
    }
    for (int64_t t = n_batched; t < n_rows; ++t) {
        double u[D];
#pragma unroll
        for (int j = 0; j < D; ++j) u[j] = (double)load_segment(p + j * stride, bytes, lane) - m[j];
#pragma unroll
        for (int i = 0, q = 0; i < D; ++i)
#pragma unroll
            for (int j = i; j < D; ++j, ++q) acc[q] = acc[q] + u[i] * u[j];
        p += row_step;
    }
    if (c >= n_chains) return;
    const double nd = (double)n_rows;
#pragma unroll
    for (int j = 0; j < D; ++j) mean_out[j * n_chains + c] = m[j];
#pragma unroll
    for (int q = 0; q < PAIRS; ++q) cov_out[q * n_chains + c] = acc[q] / nd;
}

}  // namespace glabc

using namespace glabc;

extern "C" {

__attribute__((visibility("default"))) int glabc_histogram2d(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains,
                                                             int64_t stride, int32_t n_pairs, const int32_t* pairs, int32_t n_bins,
                                                             const double* lo, const double* hi, uint64_t* counts, void* stream)
{
    if (int e = check_histogram2d(history, n_rows, theta_dim, n_chains, stride, n_pairs, pairs, n_bins, lo, hi, counts)) return e;
    if (n_chains == 0) return GLABC_OK;
    return launch_joint(history, n_rows, theta_dim, n_chains, stride, n_pairs, pairs, n_bins, lo, hi, counts, (hipStream_t)stream);
}

__attribute__((visibility("default"))) int glabc_cross_moments(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains,
                                                               int64_t stride, double* mean_out, double* cov_out, void* stream)
{
    if (int e = check_cross_moments(history, n_rows, theta_dim, n_chains, stride, mean_out, cov_out)) return e;
    if (n_chains == 0) return GLABC_OK;
    hipStream_t s = (hipStream_t)stream;
    return dispatch_range<1, GLABC_MAX_DIM>(theta_dim, GLABC_ERR_DIM, [&](auto d) {
        hipLaunchKernelGGL((cross_kernel<decltype(d)::value>), dim3(grid_for(n_chains, CROSS_LANES)), dim3(CROSS_LANES), 0, s, history, n_rows,
                           (int64_t)theta_dim * stride, n_chains, stride, mean_out, cov_out);
        return launch_status();
    });
}

}  // extern "C"
