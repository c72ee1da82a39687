// glabc_quant.hip -- integer counts over a chain-major history: the digit counts of a radix selection (glabc_key_counts) and
// marginal histograms (glabc_histogram) of include/glabc.h, which holds the specification.  One counting skeleton, the slot
// function (which counter a value adds to, or none; glabc_slots.h) as a template parameter.  No template over theta_dim: the coordinate is a
// grid dimension, as in glabc_diag.hip.
//
// count_kernel.  Lanes run along the chain index and blockIdx.y is the coordinate.  The walk over items of 64 chains x CHUNK_ROWS
// rows, the guarded loads, the uint32 table in LDS (n_slots counters, at most 8 prefixes x 2048 digits = 64 KB: two workgroups per CU)
// and the grid rule are glabc_history.h's, which argues what cannot be read, that a slot is inside the table and that no counter
// wraps.  The CHUNK_ROWS loads of an item are issued together, and a lane outside the segment counts nothing, whatever the load returned.
// Contention.  A posterior puts most of its mass into a handful of level-0 digits (sign, exponent, two mantissa bits), so many
// lanes of a wavefront add to one LDS address.  MODE says what a wavefront does about it:
//   COUNT_DIRECT   one LDS atomic per value
//   COUNT_RUNS     a lane folds the run of equal slots along the CHUNK_ROWS rows of an item into one add
// DESIGN.md 4.5 has what each measured (and a third, combining equal slots across the wavefront, that was dropped); LEVEL0_MODE and
// COUNT_MODE below are the choice.  profiles/quant_kernel_resources.txt holds the compiler's resource report.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "glabc_check.h"
#include "glabc_history.h"
#include "glabc_launch.h"
#include "glabc_slots.h"

namespace glabc {

constexpr int CHUNK_ROWS = 16;          // rows per item, their loads in flight together
constexpr int64_t MAX_ITEMS_PER_WAVE = 1 << 18;          // x HISTORY_WAVES x CHUNK_ROWS x HISTORY_LANES = 2^31 values per workgroup

enum CountMode { COUNT_DIRECT = 0, COUNT_RUNS = 1 };

template <class Slots, int MODE>
__global__ void __launch_bounds__(HISTORY_LANES* HISTORY_WAVES)
    count_kernel(const float* __restrict__ hist, int64_t n_rows, int64_t row_step, int64_t n_chains, int64_t stride, const Slots slots,
                 unsigned long long* __restrict__ counts)
{
    extern __shared__ uint32_t table[];
    const int n_slots = slots.n_slots();
    table_zero(table, n_slots);

    const int j = blockIdx.y;
    const typename Slots::Local slot_of = slots.local(j);
    const unsigned lane = threadIdx.x;
    const Walk<CHUNK_ROWS> walk(n_rows, n_chains);
    for (int64_t item = walk.first; item < walk.n_items; item += walk.n_waves) {
        const Item it = walk.item(item);
        const float* p = hist + it.row0 * row_step + j * stride + it.chain0;
        float x[CHUNK_ROWS];
#pragma unroll
        for (int r = 0; r < CHUNK_ROWS; ++r) {
            x[r] = load_segment(p, it.bytes(r), lane);
            p += it.step(r, row_step);
        }
        const bool inside = (int)lane < it.live;
        if (MODE == COUNT_RUNS) {
            int run_slot = -1;
            uint32_t run = 0;
#pragma unroll
            for (int r = 0; r < CHUNK_ROWS; ++r) {
                const int s = inside && r < it.rows ? slot_of(x[r]) : -1;
                if (s != run_slot) {
                    lds_add(table, run_slot, run);
                    run_slot = s, run = 0;
                }
                ++run;
            }
            lds_add(table, run_slot, run);
        } else {
#pragma unroll
            for (int r = 0; r < CHUNK_ROWS; ++r) lds_add(table, inside && r < it.rows ? slot_of(x[r]) : -1, 1u);
        }
    }
    table_flush(table, n_slots, counts + (int64_t)j * n_slots);
}

// workgroups per coordinate (history_grid): the part's fill is shared among the theta_dim coordinates of gridDim.y
constexpr unsigned count_grid(int64_t n_rows, int32_t theta_dim, int64_t n_chains, size_t lds_bytes)
{
    return history_grid(history_items(n_rows, n_chains, CHUNK_ROWS), HISTORY_WAVES, MAX_ITEMS_PER_WAVE,
                        (HISTORY_CUS * workgroups_per_cu(lds_bytes) + theta_dim - 1) / theta_dim);
}
// ... pinned at what count_grid's own arithmetic gave before it called history_grid
static_assert(count_grid(1, 1, 1, 16) == 1 && count_grid(16, 8, 64, 8192) == 1 && count_grid(16, 1, 7 * 64, 8192) == 1 &&
                  count_grid(16, 1, 9 * 64, 8192) == 2, "one item, HISTORY_WAVES - 1 and + 1 items");
static_assert(count_grid(1 << 20, 1, 65536, 65536) == 512 && count_grid(1 << 20, 8, 65536, 65536) == 64, "the largest key table");
static_assert(count_grid(1 << 20, 1, 65536, 16396) == 1024 && count_grid(1 << 20, 8, 65536, 16396) == 128, "the largest histogram");
static_assert(count_grid(1 << 20, 3, 65536, 40960) == 342 && count_grid(1 << 20, 3, 65536, 49152) == 256 &&
                  count_grid(1 << 20, 3, 65536, 57344) == 171, "four, three and two workgroups per CU");
static_assert(count_grid(1 << 18, 8, 1 << 20, 65536) == 128 && count_grid(1 << 18, 1, 1 << 24, 8192) == 2048, "the counters' bound wins");

template <class Slots, int MODE>
inline int launch_count(const float* history, int64_t n_rows, int32_t theta_dim, int64_t n_chains, int64_t stride, const Slots& slots,
                        int n_slots, uint64_t* counts, hipStream_t s)
{
    const size_t lds_bytes = (size_t)n_slots * sizeof(uint32_t);
    const unsigned g = count_grid(n_rows, theta_dim, n_chains, lds_bytes);
    hipLaunchKernelGGL((count_kernel<Slots, MODE>), dim3(g, theta_dim), dim3(HISTORY_LANES, HISTORY_WAVES), lds_bytes, s, history, n_rows,
                       (int64_t)theta_dim * stride, n_chains, stride, slots, (unsigned long long*)counts);
    return launch_status();
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
    return launch_count<HistSlots, COUNT_MODE>(history, n_rows, theta_dim, n_chains, stride, hist_slots(theta_dim, n_bins, lo, hi), n_bins + 3, counts,
                                               (hipStream_t)stream);
}

}  // extern "C"
