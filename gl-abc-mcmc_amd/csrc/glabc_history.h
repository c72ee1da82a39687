// glabc_history.h -- what the kernels that walk a chain-major history share: the guarded row-segment load (glabc_diag.hip,
// glabc_quant.hip, glabc_joint.hip, glabc_predictive.hip) and, for the three that count into a uint32 table in LDS, the order-preserving
// key, glabc_histogram's bin arithmetic, the walk over items of 64 chains x ROWS rows, the table's zeroing and flush, and the grid
// rule.  Host and device, and handed to hiprtc as text with glabc_predictive.h (a run-time compiled predictive program).  The counting
// kernels' three safety arguments are made here, once: nothing behind a segment's bytes can be read (load_segment, Item), a slot is
// below the table's size (bin_inside, lds_add), no counter wraps (history_grid).
#pragma once
#if !defined(__HIPCC_RTC__)          // hiprtc (glabc_rtc.hip) brings the HIP device declarations and the fixed-width types itself
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#endif

namespace glabc {

constexpr int HISTORY_LANES = 64;       // chains per item: one wavefront wide
constexpr int HISTORY_WAVES = 8;        // wavefronts per workgroup, sharing one table of counters
constexpr int HISTORY_CUS = 256;        // MI355X; sizes the grid only
constexpr int64_t HISTORY_LDS_PER_CU = 160 * 1024;

// element `lane` of the row segment at the wave-uniform address `row`, through a buffer descriptor over exactly the segment's `bytes`
// bytes: one scalar base and one 32-bit lane offset, whatever the history's size and the base's alignment, and a lane whose offset is
// not below `bytes` gets 0 without a memory access.  So a padding column, the bytes behind a ragged last segment and -- with
// bytes == 0 -- a whole row cannot be read
__device__ __forceinline__ float load_segment(const float* row, int bytes, unsigned lane)
{
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row), 0, bytes, 0x00020000);
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, lane * 4u, 0, 0));
}

// the order-preserving key of glabc_key_counts (include/glabc.h): -0 is +0, every NaN is the largest key
__host__ __device__ inline uint32_t float_key(float x)
{
    uint32_t u = __builtin_bit_cast(uint32_t, x);
    if (x != x) return 0xFFFFFFFFu;
    if (x == 0.0f) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- glabc_histogram's bins: part of its numerical contract, which glabc_histogram2d's margins and glabc_predictive_counts meet bit
// for bit because this is the one text
struct BinAxis { double lo, hi, scale; };
inline BinAxis bin_axis(double lo, double hi, int32_t n_bins)
{
    const double width = hi - lo;
    return BinAxis{lo, hi, (double)n_bins / width};
}

// the bin of x, which the caller knows to be no NaN and inside [lo, hi]: a number in 0 .. n_bins - 1
__device__ __forceinline__ int bin_inside(double x, const BinAxis& a, int n_bins)
{
    if (x == a.hi) return n_bins - 1;
    const double u = (x - a.lo) * a.scale;                        // two rounded operations: the objects are built with -ffp-contract=off
    const int b = (int)__builtin_floor(u);                        // 0 <= u <= n_bins (1 + 2^-52): inside int32
    return b < n_bins - 1 ? b : n_bins - 1;
}

// the slot of a value among the n_bins + 3 of glabc_histogram and glabc_predictive_counts: below lo, above hi and NaN behind the bins
__device__ __forceinline__ int hist_slot(float xf, const BinAxis& a, int n_bins)
{
    const double x = (double)xf;
    if (x != x) return n_bins + 2;
    if (x < a.lo) return n_bins;
    if (x > a.hi) return n_bins + 1;
    return bin_inside(x, a, n_bins);
}

// ---- the walk: a history of n_rows x n_chains is cut into items of 64 chains x ROWS rows, which the 8 wavefronts of the
// gridDim.x workgroups take round-robin, neighbouring wavefronts neighbouring row segments of the same rows.  All wave-uniform
constexpr int64_t history_items(int64_t n_rows, int64_t n_chains, int rows)
{
    return ((n_chains + HISTORY_LANES - 1) / HISTORY_LANES) * ((n_rows + rows - 1) / rows);
}

struct Item {
    int64_t chain0, row0;
    int live, rows;                     // lanes inside the segment, rows inside the history
    // row r of the item is loaded with bytes(r) bytes at a pointer that then moves on by step(r, row_step): a row past the end has the
    // last row's address and no bytes, and only a lane below `live` may count what it loaded
    __device__ int bytes(int r) const { return r < rows ? 4 * live : 0; }
    __device__ int64_t step(int r, int64_t row_step) const { return r + 1 < rows ? row_step : 0; }
};

template <int ROWS>
struct Walk {
    const int64_t n_rows, n_chains;
    const int64_t n_segments = (n_chains + HISTORY_LANES - 1) / HISTORY_LANES;
    const int64_t n_items = history_items(n_rows, n_chains, ROWS);
    const int64_t n_waves = (int64_t)gridDim.x * HISTORY_WAVES;
    const int64_t first = (int64_t)blockIdx.x * HISTORY_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.y);          // this wavefront's

    __device__ Walk(int64_t rows, int64_t chains) : n_rows(rows), n_chains(chains) {}
    __device__ Item item(int64_t i) const
    {
        const int64_t chain0 = i % n_segments * HISTORY_LANES, row0 = i / n_segments * ROWS;
        return Item{chain0, row0, (int)(n_chains - chain0 < HISTORY_LANES ? n_chains - chain0 : HISTORY_LANES),
                    (int)(n_rows - row0 < ROWS ? n_rows - row0 : ROWS)};
    }
};

// ---- the table: n_slots uint32 counters in LDS, zeroed at a workgroup's start; at its end the workgroup adds its non-zero counters
// to `out` with 64-bit integer atomics.  Integer adds commute: the table is the same bits in every order and for every grid
__device__ __forceinline__ void table_zero(uint32_t* table, int n_slots)
{
    const int tid = threadIdx.y * HISTORY_LANES + threadIdx.x;
    for (int i = tid; i < n_slots; i += HISTORY_LANES * HISTORY_WAVES) table[i] = 0u;
    __syncthreads();
}

// slot < 0: nothing to add.  A caller's slot function returns an index below the n_slots the table was launched with
__device__ __forceinline__ void lds_add(uint32_t* table, int slot, uint32_t n)
{
    if (slot >= 0) atomicAdd(&table[slot], n);
}

__device__ __forceinline__ void table_flush(const uint32_t* table, int n_slots, unsigned long long* out)
{
    __syncthreads();
    const int tid = threadIdx.y * HISTORY_LANES + threadIdx.x;
    for (int i = tid; i < n_slots; i += HISTORY_LANES * HISTORY_WAVES) {
        const uint32_t c = table[i];
        if (c) atomicAdd(&out[i], (unsigned long long)c);
    }
}

// ---- the grid.  Workgroups per CU: as many as its 160 KB of LDS and its 32 wavefronts hold; no table: the wavefronts alone decide.
// (The same number as thresholds at 40 KB and 53 KB give, but for tables of 54 273 to 54 613 bytes, and a table is 4 x n_prefixes x 2^10
// or 2^11 bytes, 4 (n_bins + 3) <= 16 396, 4 (n_bins^2 + 2) with 116 and 117 bins either side of that range, or at most 36 972 bytes.)
constexpr int64_t workgroups_per_cu(size_t lds_bytes)
{
    constexpr int64_t most = 32 / HISTORY_WAVES;
    return (int64_t)lds_bytes > HISTORY_LDS_PER_CU / most ? HISTORY_LDS_PER_CU / (int64_t)lds_bytes : most;
}

// workgroups along x: `fill` (what fills the part), no more than there are items to give every wavefront one, and -- the bound the
// uint32 counters need -- at least so many that a wavefront takes at most max_items_per_wave items.  A caller chooses that number so
// that max_items_per_wave x waves x ROWS x 64 = 2^31: a workgroup counts at most 2^31 values between zeroing and flush
constexpr unsigned history_grid(int64_t n_items, int waves, int64_t max_items_per_wave, int64_t fill)
{
    const int64_t most = (n_items + waves - 1) / waves;
    const int64_t least = (n_items + waves * max_items_per_wave - 1) / (waves * max_items_per_wave);
    const int64_t g = fill > most ? most : fill;
    return (unsigned)(g < least ? least : g);
}

}  // namespace glabc
