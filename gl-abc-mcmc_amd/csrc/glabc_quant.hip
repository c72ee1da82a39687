// glabc_quant.hip -- integer counts over a chain-major history: the digit counts of a radix selection (glabc_key_counts) and
// marginal histograms (glabc_histogram) of include/glabc.h, which holds the specification.  One counting skeleton, the slot
// function (which counter a value adds to, or none) as a template parameter.  No template over theta_dim: the coordinate is a
// grid dimension, as in glabc_diag.hip.
//
// count_kernel.  Lanes run along the chain index and blockIdx.y is the coordinate.  A coordinate's work is cut into items of
// 64 chains x CHUNK_ROWS rows; the WAVES wavefronts of the gridDim.x workgroups take them round-robin, neighbouring wavefronts
// neighbouring row segments of the same rows.  The CHUNK_ROWS loads of an item are issued together; every load goes through a
// buffer descriptor over exactly the segment's bytes (one scalar base, one 32-bit lane offset, whatever the history's size and
// whatever the base's alignment), so a padding column, the bytes behind a ragged last segment and a row past the end cannot be
// read -- and a lane outside the segment counts nothing, whatever the load returned.
// Counters.  uint32 in LDS, n_slots of them (at most 8 prefixes x 2048 digits = 64 KB: two workgroups per CU), zeroed at the start;
// at its end a workgroup adds its non-zero counters to `counts` with 64-bit integer atomics.  Integer adds commute: the table
// is the same bits in every order and for every grid.  glabc_key_counts / glabc_histogram size the grid so that no workgroup
// counts 2^32 or more values (count_grid below).
// Contention.  A posterior puts most of its mass into a handful of level-0 digits (sign, exponent, two mantissa bits), so many
// lanes of a wavefront add to one LDS address.  MODE says what a wavefront does about it:
//   COUNT_DIRECT   one LDS atomic per value
//   COUNT_RUNS     a lane folds the run of equal slots along the CHUNK_ROWS rows of an item into one add
// DESIGN.md 4.5 has what each measured (and a third, combining equal slots across the wavefront, that was dropped); LEVEL0_MODE and
// COUNT_MODE below are the choice.
// profiles/quant_kernel_resources.txt holds the compiler's resource report.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "glabc_check.h"
#include "glabc_launch.h"

namespace glabc {

constexpr int QUANT_LANES = 64;         // chains per item: one wavefront wide
constexpr int QUANT_WAVES = 8;          // wavefronts per workgroup, sharing one table of counters
constexpr int CHUNK_ROWS = 16;          // rows per item, their loads in flight together
constexpr int QUANT_CUS = 256;          // MI355X; sizes the grid only
constexpr int64_t MAX_ITEMS_PER_WAVE = 1 << 18;          // x QUANT_WAVES x CHUNK_ROWS x QUANT_LANES = 2^31 values per workgroup

enum CountMode { COUNT_DIRECT = 0, COUNT_RUNS = 1 };

// ---- slot functions: value -> index of its counter in the coordinate's table, or -1 -------------------------------------------
__host__ __device__ inline uint32_t float_key(float x)
{
    uint32_t u = __builtin_bit_cast(uint32_t, x);
    if (x != x) return 0xFFFFFFFFu;
    if (x == 0.0f) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// NP: 0 at level 0, where every value belongs and nothing is compared; otherwise the prefixes compared per value -- n_prefixes
// rounded up to 1, 2, 4 or 8, the slots past n_prefixes unused.  Two vector instructions per prefix and value: the kernel is bound
// by its vector instructions before it is bound by HBM, so a launch pays for the prefixes it has
template <int NP>
struct KeySlots {
    uint32_t prefix[GLABC_MAX_DIM][NP ? NP : 1];
    int32_t n_prefixes, prefix_shift, digit_shift, digit_bits;   // prefix_shift: 32 - prefix_bits

    __device__ int n_slots() const { return n_prefixes << digit_bits; }
    // the coordinate's prefixes, from the kernel arguments into scalar registers
    struct Local {
        uint32_t p[NP ? NP : 1];
        int32_t prefix_shift, digit_shift, digit_bits;
        __device__ int operator()(float x) const
        {
            const uint32_t k = float_key(x);
            const int digit = (int)((k >> digit_shift) & ((1u << digit_bits) - 1u));
            if (NP == 0) return digit;
            const uint32_t mine = k >> prefix_shift;
            int slot = -1;
#pragma unroll
            for (int s = 0; s < NP; ++s) slot = mine == p[s] ? s : slot;          // an unused slot matches no prefix
            return slot < 0 ? -1 : (slot << digit_bits) | digit;
        }
    };
    __device__ Local local(int j) const
    {
        Local l;
#pragma unroll
        for (int s = 0; s < (NP ? NP : 1); ++s) l.p[s] = prefix[j][s];
        l.prefix_shift = prefix_shift, l.digit_shift = digit_shift, l.digit_bits = digit_bits;
        return l;
    }
};

struct HistSlots {
    double lo[GLABC_MAX_DIM], hi[GLABC_MAX_DIM], scale[GLABC_MAX_DIM];
    int32_t n_bins;

    __device__ int n_slots() const { return n_bins + 3; }
    struct Local {
        double lo, hi, scale;
        int32_t n_bins;
        __device__ int operator()(float xf) const
        {
            const double x = (double)xf;
            if (x != x) return n_bins + 2;
            if (x < lo) return n_bins;
            if (x > hi) return n_bins + 1;
            if (x == hi) return n_bins - 1;
            const double u = (x - lo) * scale;                    // two rounded operations: the object is built with -ffp-contract=off
            const int b = (int)__builtin_floor(u);                // 0 <= u <= n_bins (1 + 2^-52): inside int32
            return b < n_bins - 1 ? b : n_bins - 1;
        }
    };
    __device__ Local local(int j) const { return Local{lo[j], hi[j], scale[j], n_bins}; }
};

// element `lane` of the row segment at the wave-uniform address `row`: nothing behind its `bytes` bytes can be read
__device__ __forceinline__ float load_segment(const float* row, int bytes, unsigned lane)
{
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row), 0, bytes, 0x00020000);
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, lane * 4u, 0, 0));
}

// slot < 0: nothing to add.  The table has n_slots counters and every slot function returns an index below that
__device__ __forceinline__ void lds_add(uint32_t* table, int slot, uint32_t n)
{
    if (slot >= 0) atomicAdd(&table[slot], n);
}

template <class Slots, int MODE>
__global__ void __launch_bounds__(QUANT_LANES* QUANT_WAVES)
    count_kernel(const float* __restrict__ hist, int64_t n_rows, int64_t row_step, int64_t n_chains, int64_t stride, const Slots slots,
                 unsigned long long* __restrict__ counts)
{
    extern __shared__ uint32_t table[];
    const int n_slots = slots.n_slots();
    const int tid = threadIdx.y * QUANT_LANES + threadIdx.x;
    for (int i = tid; i < n_slots; i += QUANT_LANES * QUANT_WAVES) table[i] = 0u;
    __syncthreads();

    const int j = blockIdx.y;
    const typename Slots::Local slot_of = slots.local(j);
    const unsigned lane = threadIdx.x;
    const int64_t n_segments = (n_chains + QUANT_LANES - 1) / QUANT_LANES;
    const int64_t n_items = n_segments * ((n_rows + CHUNK_ROWS - 1) / CHUNK_ROWS);
    const int64_t n_waves = (int64_t)gridDim.x * QUANT_WAVES;
    const int64_t wave = (int64_t)blockIdx.x * QUANT_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.y);
    for (int64_t item = wave; item < n_items; item += n_waves) {
        const int64_t chain0 = item % n_segments * QUANT_LANES;
        const int64_t row0 = item / n_segments * CHUNK_ROWS;
        const int live = (int)(n_chains - chain0 < QUANT_LANES ? n_chains - chain0 : QUANT_LANES);           // lanes inside the segment
        const int rows = (int)(n_rows - row0 < CHUNK_ROWS ? n_rows - row0 : CHUNK_ROWS);                       // rows inside the history
        const float* p = hist + row0 * row_step + j * stride + chain0;
        float x[CHUNK_ROWS];
#pragma unroll
        for (int r = 0; r < CHUNK_ROWS; ++r) {                    // a row past the end: the last row's address and no bytes
            x[r] = load_segment(p, r < rows ? 4 * live : 0, lane);
            p += r + 1 < rows ? row_step : 0;
        }
        const bool inside = (int)lane < live;
        if (MODE == COUNT_RUNS) {
            int run_slot = -1;
            uint32_t run = 0;
#pragma unroll
            for (int r = 0; r < CHUNK_ROWS; ++r) {
                const int s = inside && r < rows ? slot_of(x[r]) : -1;
                if (s != run_slot) {
                    lds_add(table, run_slot, run);
                    run_slot = s, run = 0;
                }
                ++run;
            }
            lds_add(table, run_slot, run);
        } else {
#pragma unroll
            for (int r = 0; r < CHUNK_ROWS; ++r) lds_add(table, inside && r < rows ? slot_of(x[r]) : -1, 1u);
        }
    }
    __syncthreads();
    unsigned long long* out = counts + (int64_t)j * n_slots;
    for (int i = tid; i < n_slots; i += QUANT_LANES * QUANT_WAVES) {
        const uint32_t c = table[i];
        if (c) atomicAdd(&out[i], (unsigned long long)c);
    }
}

// workgroups per coordinate: enough to fill the part (as many workgroups per CU as the LDS and the 32 wavefronts of a CU hold), no
// more than there are items, and -- the bound the uint32 counters need -- at least so many that a wavefront takes at most
// MAX_ITEMS_PER_WAVE items: a workgroup then counts at most 2^18 x 8 x 16 x 64 = 2^31 values between zeroing and flush
inline unsigned count_grid(int64_t n_rows, int32_t theta_dim, int64_t n_chains, size_t lds_bytes)
{
    const int64_t n_items = ((n_chains + QUANT_LANES - 1) / QUANT_LANES) * ((n_rows + CHUNK_ROWS - 1) / CHUNK_ROWS);
    const int64_t per_cu = lds_bytes > 40 * 1024 ? (lds_bytes > 53 * 1024 ? 2 : 3) : 4;
    int64_t g = (QUANT_CUS * per_cu + theta_dim - 1) / theta_dim;
    const int64_t most = (n_items + QUANT_WAVES - 1) / QUANT_WAVES;
    if (g > most) g = most;
    const int64_t least = (n_items + QUANT_WAVES * MAX_ITEMS_PER_WAVE - 1) / (QUANT_WAVES * MAX_ITEMS_PER_WAVE);
    if (g < least) g = least;
    return (unsigned)g;
}

template <class Slots, int MODE>
inline int launch_count(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride, const Slots& slots,
                        int n_slots, uint64_t* counts, hipStream_t s)
{
    const size_t lds_bytes = (size_t)n_slots * sizeof(uint32_t);
    const unsigned g = count_grid(n_rows, theta_dim, n_chains, lds_bytes);
    hipLaunchKernelGGL((count_kernel<Slots, MODE>), dim3(g, theta_dim), dim3(QUANT_LANES, QUANT_WAVES), lds_bytes, s, history, n_rows,
                       (int64_t)theta_dim * stride, n_chains, stride, slots, (unsigned long long*)counts);
    return launch_status();
}

template <int NP>
inline KeySlots<NP> key_slots(int32_t theta_dim, int32_t level, int32_t n_prefixes, const uint32_t* prefixes)
{
    KeySlots<NP> k;
    for (int j = 0; j < GLABC_MAX_DIM; ++j)
        for (int s = 0; s < (NP ? NP : 1); ++s)
            k.prefix[j][s] = NP && j < theta_dim && s < n_prefixes ? prefixes[j * n_prefixes + s] : KEY_UNUSED_SLOT;
    k.n_prefixes = n_prefixes;
    k.prefix_shift = 32 - key_prefix_bits(level);               // level 0 (NP == 0) never shifts by it
    k.digit_bits = key_digit_bits(level);
    k.digit_shift = 32 - key_prefix_bits(level) - k.digit_bits;
    return k;
}

// what a wavefront does about equal slots: folding runs pays at level 0 alone, where a chain stays on one digit
// for rows on end; at levels 1 and 2, where few values belong to a prefix, the two modes take the same time
constexpr int COUNT_MODE = COUNT_DIRECT;
constexpr int LEVEL0_MODE = COUNT_RUNS;

template <int MODE, int NP>
inline int key_counts_np(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride, int32_t level,
                         int32_t n_prefixes, const uint32_t* prefixes, uint64_t* counts, hipStream_t s)
{
    return launch_count<KeySlots<NP>, MODE>(history, n_rows, theta_dim, n_chains, stride, key_slots<NP>(theta_dim, level, n_prefixes, prefixes),
                                            n_prefixes << key_digit_bits(level), counts, s);
}

template <int MODE>
inline int key_counts_as(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride, int32_t level,
                         int32_t n_prefixes, const uint32_t* prefixes, uint64_t* counts, hipStream_t s)
{
    if (level == 0) return key_counts_np<MODE, 0>(history, n_rows, theta_dim, n_chains, stride, level, n_prefixes, prefixes, counts, s);
    if (n_prefixes == 1) return key_counts_np<MODE, 1>(history, n_rows, theta_dim, n_chains, stride, level, n_prefixes, prefixes, counts, s);
    if (n_prefixes == 2) return key_counts_np<MODE, 2>(history, n_rows, theta_dim, n_chains, stride, level, n_prefixes, prefixes, counts, s);
    if (n_prefixes <= 4) return key_counts_np<MODE, 4>(history, n_rows, theta_dim, n_chains, stride, level, n_prefixes, prefixes, counts, s);
    return key_counts_np<MODE, 8>(history, n_rows, theta_dim, n_chains, stride, level, n_prefixes, prefixes, counts, s);
}

}  // namespace glabc

using namespace glabc;

extern "C" {

__attribute__((visibility("default"))) int glabc_key_counts(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains,
                                                            int64_t stride, int32_t level, int32_t n_prefixes, const uint32_t* prefixes,
                                                            uint64_t* counts, void* stream)
{
    if (int e = check_key_counts(history, n_rows, theta_dim, n_chains, stride, level, n_prefixes, prefixes, counts)) return e;
    if (n_chains == 0) return GLABC_OK;
    hipStream_t s = (hipStream_t)stream;
    if (level == 0) return key_counts_np<LEVEL0_MODE, 0>(history, n_rows, theta_dim, n_chains, stride, level, n_prefixes, prefixes, counts, s);
    return key_counts_as<COUNT_MODE>(history, n_rows, theta_dim, n_chains, stride, level, n_prefixes, prefixes, counts, s);
}

__attribute__((visibility("default"))) int glabc_histogram(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains,
                                                           int64_t stride, int32_t n_bins, const double* lo, const double* hi,
                                                           uint64_t* counts, void* stream)
{
    if (int e = check_histogram(history, n_rows, theta_dim, n_chains, stride, n_bins, lo, hi, counts)) return e;
    if (n_chains == 0) return GLABC_OK;
    HistSlots h;
    for (int j = 0; j < GLABC_MAX_DIM; ++j) {
        h.lo[j] = j < theta_dim ? lo[j] : 0.0;
        h.hi[j] = j < theta_dim ? hi[j] : 1.0;
        const double width = h.hi[j] - h.lo[j];
        h.scale[j] = (double)n_bins / width;
    }
    h.n_bins = n_bins;
    return launch_count<HistSlots, COUNT_MODE>(history, n_rows, theta_dim, n_chains, stride, h, n_bins + 3, counts, (hipStream_t)stream);
}

}  // extern "C"
