// glabc_joint.hip -- the joint posterior of a chain-major history: pair histograms (glabc_histogram2d) and per-chain cross moments
// (glabc_cross_moments) of include/glabc.h, which holds both specifications.
//
// joint_kernel.  The counting skeleton of glabc_quant.hip's count_kernel with a pair of coordinates where that has one: lanes run
// along the chain index, blockIdx.y is the pair, a pair's work is cut into items of 64 chains x JOINT_ROWS rows that the
// JOINT_WAVES wavefronts of the gridDim.x workgroups take round-robin.  An item loads the row segments of both coordinates, all
// 2 x JOINT_ROWS loads issued together, every one through a buffer descriptor over exactly the segment's bytes: a padding column,
// the bytes behind a ragged last segment and a row past the end cannot be read, whatever the base's alignment, and a lane outside
// the segment counts nothing.  Each value is binned on its own axis by glabc_histogram's double arithmetic (axis_bin; the object
// is built with -ffp-contract=off) and the two bins make the slot.
// Counters.  uint32 in LDS, n_bins^2 + 2 of them, zeroed at the start; at its end a workgroup adds its non-zero counters to `counts`
// with 64-bit integer atomics, so the table is the same bits in every order and for every grid.  joint_grid sizes the grid so
// that no workgroup counts 2^32 or more draws.  At 128 bins the table is 65 544 bytes: past what a launch gets unasked, so the
// launcher has the size granted (glabc_lds_grant.h) as the lane-group and the flow launchers do; two workgroups share a CU then.
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
#include "glabc_launch.h"
#include "glabc_lds_grant.h"

namespace glabc {

constexpr int JOINT_LANES = 64;         // chains per item: one wavefront wide
constexpr int JOINT_WAVES = 8;          // wavefronts per workgroup, sharing one table of counters
constexpr int JOINT_ROWS = 8;           // rows per item: the 16 loads of both coordinates in flight together, as count_kernel's 16
                                        // (16 rows are 32 descriptors, more than the scalar file holds without spilling)
constexpr int JOINT_CUS = 256;          // MI355X; sizes the grid only
constexpr int64_t JOINT_LDS_PER_CU = 160 * 1024;
constexpr int64_t JOINT_MAX_ITEMS_PER_WAVE = 1 << 19;    // x JOINT_WAVES x JOINT_ROWS x JOINT_LANES = 2^31 draws per workgroup

constexpr int AXIS_OUTSIDE = -1, AXIS_NAN = -2;

struct JointSlots {
    double lo[GLABC_MAX_DIM], hi[GLABC_MAX_DIM], scale[GLABC_MAX_DIM];
    int32_t n_bins;
    uint8_t a[GLABC_MAX_PAIRS], b[GLABC_MAX_PAIRS];
};

struct Axis {
    double lo, hi, scale;
    // the bin of a value on this axis, glabc_histogram's rule; AXIS_OUTSIDE below lo or above hi, AXIS_NAN
    __device__ int bin(float xf, int n_bins) const
    {
        const double x = (double)xf;
        if (x != x) return AXIS_NAN;
        if (x < lo || x > hi) return AXIS_OUTSIDE;
        if (x == hi) return n_bins - 1;
        const double u = (x - lo) * scale;                        // two rounded operations: -ffp-contract=off
        const int b = (int)__builtin_floor(u);                    // 0 <= u <= n_bins (1 + 2^-52): inside int32
        return b < n_bins - 1 ? b : n_bins - 1;
    }
};

// a NaN on either axis before a value outside on either axis before the cell
__device__ __forceinline__ int joint_slot(int bin_a, int bin_b, int n_bins)
{
    const int least = bin_a < bin_b ? bin_a : bin_b;
    const int cells = n_bins * n_bins;
    return least >= 0 ? bin_a * n_bins + bin_b : least == AXIS_NAN ? cells + 1 : cells;
}

// element `lane` of the row segment at the wave-uniform address `row`: nothing behind its `bytes` bytes can be read
__device__ __forceinline__ float load_segment(const float* row, int bytes, unsigned lane)
{
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row), 0, bytes, 0x00020000);
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, lane * 4u, 0, 0));
}

// slot < 0: nothing to add.  The table has n_bins^2 + 2 counters and joint_slot returns an index below that
__device__ __forceinline__ void lds_add(uint32_t* table, int slot, uint32_t n)
{
    if (slot >= 0) atomicAdd(&table[slot], n);
}

__global__ void __launch_bounds__(JOINT_LANES* JOINT_WAVES)
    joint_kernel(const float* __restrict__ hist, int64_t n_rows, int64_t row_step, int64_t n_chains, int64_t stride, const JointSlots slots,
                 unsigned long long* __restrict__ counts)
{
    extern __shared__ uint32_t table[];
    const int n_bins = slots.n_bins;
    const int n_slots = n_bins * n_bins + 2;
    const int tid = threadIdx.y * JOINT_LANES + threadIdx.x;
    for (int i = tid; i < n_slots; i += JOINT_LANES * JOINT_WAVES) table[i] = 0u;
    __syncthreads();

    const int pair = blockIdx.y;
    const int ja = slots.a[pair], jb = slots.b[pair];
    const Axis axis_a{slots.lo[ja], slots.hi[ja], slots.scale[ja]}, axis_b{slots.lo[jb], slots.hi[jb], slots.scale[jb]};
    const unsigned lane = threadIdx.x;
    const int64_t n_segments = (n_chains + JOINT_LANES - 1) / JOINT_LANES;
    const int64_t n_items = n_segments * ((n_rows + JOINT_ROWS - 1) / JOINT_ROWS);
    const int64_t n_waves = (int64_t)gridDim.x * JOINT_WAVES;
    const int64_t wave = (int64_t)blockIdx.x * JOINT_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    for (int64_t item = wave; item < n_items; item += n_waves) {
        const int64_t chain0 = item % n_segments * JOINT_LANES;
        const int64_t row0 = item / n_segments * JOINT_ROWS;
        const int live = (int)(n_chains - chain0 < JOINT_LANES ? n_chains - chain0 : JOINT_LANES);           // lanes inside the segment
        const int rows = (int)(n_rows - row0 < JOINT_ROWS ? n_rows - row0 : JOINT_ROWS);                       // rows inside the history
        const float* pa = hist + row0 * row_step + ja * stride + chain0;
        const float* pb = hist + row0 * row_step + jb * stride + chain0;
        float xa[JOINT_ROWS], xb[JOINT_ROWS];
#pragma unroll
        for (int r = 0; r < JOINT_ROWS; ++r) {                    // a row past the end: the last row's address and no bytes
            xa[r] = load_segment(pa, r < rows ? 4 * live : 0, lane);
            xb[r] = load_segment(pb, r < rows ? 4 * live : 0, lane);
            pa += r + 1 < rows ? row_step : 0;
            pb += r + 1 < rows ? row_step : 0;
        }
        const bool inside = (int)lane < live;
#pragma unroll
        for (int r = 0; r < JOINT_ROWS; ++r)
            lds_add(table, inside && r < rows ? joint_slot(axis_a.bin(xa[r], n_bins), axis_b.bin(xb[r], n_bins), n_bins) : -1, 1u);
    }
    __syncthreads();
    unsigned long long* out = counts + (int64_t)pair * n_slots;
    for (int i = tid; i < n_slots; i += JOINT_LANES * JOINT_WAVES) {
        const uint32_t c = table[i];
        if (c) atomicAdd(&out[i], (unsigned long long)c);
    }
}

// workgroups per pair: enough to fill the part (as many workgroups per CU as its LDS and its 32 wavefronts hold), no more than
// there are items, and -- the bound the uint32 counters need -- at least so many that a wavefront takes at most
// JOINT_MAX_ITEMS_PER_WAVE items: a workgroup then counts at most 2^19 x 8 x 8 x 64 = 2^31 draws between zeroing and flush
inline unsigned joint_grid(int64_t n_rows, int32_t n_pairs, int64_t n_chains, size_t lds_bytes)
{
    const int64_t n_items = ((n_chains + JOINT_LANES - 1) / JOINT_LANES) * ((n_rows + JOINT_ROWS - 1) / JOINT_ROWS);
    int64_t per_cu = JOINT_LDS_PER_CU / (int64_t)lds_bytes;
    if (per_cu > 32 / JOINT_WAVES) per_cu = 32 / JOINT_WAVES;
    int64_t g = (JOINT_CUS * per_cu + n_pairs - 1) / n_pairs;
    const int64_t most = (n_items + JOINT_WAVES - 1) / JOINT_WAVES;
    if (g > most) g = most;
    const int64_t least = (n_items + JOINT_WAVES * JOINT_MAX_ITEMS_PER_WAVE - 1) / (JOINT_WAVES * JOINT_MAX_ITEMS_PER_WAVE);
    if (g < least) g = least;
    return (unsigned)g;
}

inline int launch_joint(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride, int32_t n_pairs,
                        const int32_t* pairs, int32_t n_bins, const double* lo, const double* hi, uint64_t* counts, hipStream_t s)
{
    JointSlots j;
    for (int q = 0; q < GLABC_MAX_DIM; ++q) j.lo[q] = 0.0, j.hi[q] = 1.0, j.scale[q] = 1.0;          // a coordinate no pair uses
    for (int p = 0; p < GLABC_MAX_PAIRS; ++p) {
        j.a[p] = (uint8_t)(p < n_pairs ? pairs[2 * p] : 0);
        j.b[p] = (uint8_t)(p < n_pairs ? pairs[2 * p + 1] : 0);
    }
    for (int q = 0; q < 2 * n_pairs; ++q) {
        const int c = pairs[q];
        j.lo[c] = lo[c], j.hi[c] = hi[c];
        const double width = j.hi[c] - j.lo[c];
        j.scale[c] = (double)n_bins / width;
    }
    j.n_bins = n_bins;
    const size_t lds_bytes = ((size_t)n_bins * n_bins + 2) * sizeof(uint32_t);
    static LdsGrant grant;                               // per device
    if (!grant_dynamic_lds(grant, (const void*)joint_kernel, lds_bytes)) return GLABC_ERR_LAUNCH;
    const unsigned g = joint_grid(n_rows, n_pairs, n_chains, lds_bytes);
    hipLaunchKernelGGL(joint_kernel, dim3(g, n_pairs), dim3(JOINT_LANES, JOINT_WAVES), lds_bytes, s, history, n_rows,
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
