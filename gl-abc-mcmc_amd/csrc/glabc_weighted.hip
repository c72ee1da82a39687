// glabc_weighted.hip -- integer counts over weighted draws: glabc_weighted_key_counts, glabc_weighted_histogram and
// glabc_weighted_histogram2d of include/glabc.h, which holds the specification.  Each is its unweighted twin (glabc_quant.hip,
// glabc_joint.hip) on the one-row history [1][dim][stride], with a draw adding its quantised weight m (weight_multiplicity,
// glabc_weighted_walk.h) where the twin adds 1; the slot functions are the twins' own text (glabc_slots.h), so the key, the levels, the prefix
// rules, the bin arithmetic and the slot layouts cannot differ.
//
// weighted_count_kernel<Slots> / weighted_joint_kernel.  Lanes run along the draws and blockIdx.y is the coordinate (the pair).  The
// draws are cut into items of 64 x WEIGHTED_SEGMENTS consecutive draws, which the 8 wavefronts of the gridDim.x workgroups take
// round-robin (the walk, the 64-bit table helpers and the quantised weight are glabc_weighted_walk.h's, which
// glabc_weighted_predictive.h shares).  Every 64-draw segment of an item, the weights' included, is loaded through load_segment (glabc_history.h) with a
// descriptor over exactly its bytes: a padding column, the floats behind the last draw and -- with no bytes -- a whole segment past
// the end cannot be read, whatever the base's alignment.  The loads of an item are issued together, and a lane outside its segment
// adds nothing, whatever the load returned.  A draw of multiplicity 0 is skipped before its value is looked at: a NaN that carries
// no weight does not reach the NaN slot.
// Table.  `unsigned long long` counters in LDS (ds_add_u64), zeroed at the workgroup's start; the non-zero ones are added to the
// caller's table with 64-bit global atomics at its end.  uint32 counters would not do: two draws of multiplicity 2^31 wrap one.  A
// 64-bit counter cannot wrap: n <= 2^31 draws of at most 2^32 - 1 each stay below 2^63, so unlike history_grid the grid rule needs no
// lower bound.  The largest tables -- 8 prefixes x 2^11 digits = 131 072 bytes, 128^2 + 2 cells = 131 088 bytes -- are past what a
// launch gets unasked, so the launchers have the size granted (glabc_lds_grant.h); one workgroup then has a CU's LDS to itself, and
// the grid is sized from the real table (workgroups_per_cu).
// Contention.  One LDS atomic per draw of positive multiplicity, as the twins' COUNT_DIRECT.  COUNT_RUNS folds along the rows of an
// item and has no analogue at one row; combining equal slots across the lanes of a wavefront was dropped for counts
// and is not here.  Integer adds commute: the counts are the same bits either way, in every launch geometry.
// profiles/weighted_kernel_resources.txt holds the compiler's resource report.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "glabc_check.h"
#include "glabc_history.h"
#include "glabc_launch.h"
#include "glabc_lds_grant.h"
#include "glabc_slots.h"
#include "glabc_weighted_walk.h"

namespace glabc {

constexpr int WEIGHTED_SEGMENTS = 4;    // 64-draw segments per item: 8 (one coordinate) or 12 (a pair) loads in flight together
constexpr int64_t WEIGHTED_ITEM = (int64_t)HISTORY_LANES * WEIGHTED_SEGMENTS;

// ---- the walk over the draws (glabc_weighted_walk.h) at WEIGHTED_SEGMENTS segments per item; the 64-bit table helpers and
// lane_multiplicity are that header's too
constexpr int64_t weighted_items(int64_t n) { return draw_items<WEIGHTED_SEGMENTS>(n); }
using DrawItem = DrawItemOf<WEIGHTED_SEGMENTS>;
using DrawWalk = DrawWalkOf<WEIGHTED_SEGMENTS>;

template <class Slots>
__global__ void __launch_bounds__(HISTORY_LANES* HISTORY_WAVES)
    weighted_count_kernel(const float* __restrict__ x, int64_t stride, const float* __restrict__ w, int64_t n, double scale, const Slots slots,
                          unsigned long long* __restrict__ counts)
{
    extern __shared__ unsigned long long count_table[];
    const int n_slots = slots.n_slots();
    table_zero(count_table, n_slots);

    const int j = blockIdx.y;
    const typename Slots::Local slot_of = slots.local(j);
    const unsigned lane = threadIdx.x;
    const float* xj = x + j * stride;
    const DrawWalk walk(n);
    for (int64_t item = walk.first; item < walk.n_items; item += walk.n_waves) {
        const DrawItem it = walk.item(item);
        float xv[WEIGHTED_SEGMENTS], wv[WEIGHTED_SEGMENTS];
#pragma unroll
        for (int r = 0; r < WEIGHTED_SEGMENTS; ++r) {
            xv[r] = load_segment(xj + it.at(r), it.bytes(r), lane);
            wv[r] = load_segment(w + it.at(r), it.bytes(r), lane);
        }
#pragma unroll
        for (int r = 0; r < WEIGHTED_SEGMENTS; ++r) {
            const unsigned long long m = lane_multiplicity(it, r, lane, wv[r], scale);
            lds_add(count_table, m ? slot_of(xv[r]) : -1, m);
        }
    }
    table_flush(count_table, n_slots, counts + (int64_t)j * n_slots);
}

__global__ void __launch_bounds__(HISTORY_LANES* HISTORY_WAVES)
    weighted_joint_kernel(const float* __restrict__ x, int64_t stride, const float* __restrict__ w, int64_t n, double scale, const JointSlots slots,
                          unsigned long long* __restrict__ counts)
{
    extern __shared__ unsigned long long joint_table[];
    const int n_bins = slots.n_bins;
    const int n_slots = n_bins * n_bins + 2;
    table_zero(joint_table, n_slots);

    const int pair = blockIdx.y;
    const int ja = slots.a[pair], jb = slots.b[pair];
    const BinAxis axis_a{slots.lo[ja], slots.hi[ja], slots.scale[ja]}, axis_b{slots.lo[jb], slots.hi[jb], slots.scale[jb]};
    const unsigned lane = threadIdx.x;
    const float* xa = x + ja * stride;
    const float* xb = x + jb * stride;
    const DrawWalk walk(n);
    for (int64_t item = walk.first; item < walk.n_items; item += walk.n_waves) {
        const DrawItem it = walk.item(item);
        float va[WEIGHTED_SEGMENTS], vb[WEIGHTED_SEGMENTS], wv[WEIGHTED_SEGMENTS];
#pragma unroll
        for (int r = 0; r < WEIGHTED_SEGMENTS; ++r) {
            va[r] = load_segment(xa + it.at(r), it.bytes(r), lane);
            vb[r] = load_segment(xb + it.at(r), it.bytes(r), lane);
            wv[r] = load_segment(w + it.at(r), it.bytes(r), lane);
        }
#pragma unroll
        for (int r = 0; r < WEIGHTED_SEGMENTS; ++r) {
            const unsigned long long m = lane_multiplicity(it, r, lane, wv[r], scale);
            lds_add(joint_table, m ? joint_slot(axis_bin(va[r], axis_a, n_bins), axis_bin(vb[r], axis_b, n_bins), n_bins) : -1, m);
        }
    }
    table_flush(joint_table, n_slots, counts + (int64_t)pair * n_slots);
}

// workgroups per coordinate or pair: what fills the part -- as many workgroups per CU as the real table lets in, shared among the
// n_tables tables of gridDim.y -- and no more than there are items to give every wavefront one.  No lower bound: a 64-bit counter
// cannot wrap (above)
constexpr unsigned weighted_grid(int64_t n, int32_t n_tables, size_t lds_bytes)
{
    const int64_t most = (weighted_items(n) + HISTORY_WAVES - 1) / HISTORY_WAVES;
    const int64_t fill = (HISTORY_CUS * workgroups_per_cu(lds_bytes) + n_tables - 1) / n_tables;
    return (unsigned)(fill > most ? most : fill);
}
static_assert(weighted_grid(1, 1, 16) == 1 && weighted_grid(8 * WEIGHTED_ITEM, 8, 16384) == 1 && weighted_grid(8 * WEIGHTED_ITEM + 1, 1, 16384) == 2 &&
                  weighted_grid(7 * WEIGHTED_ITEM + 1, 28, 131088) == 1, "one item, one workgroup's first round and one draw more");
static_assert(weighted_grid(int64_t(1) << 31, 1, 131072) == 256 && weighted_grid(int64_t(1) << 31, 8, 131072) == 32, "the largest key table");
static_assert(weighted_grid(int64_t(1) << 31, 1, 131088) == 256 && weighted_grid(int64_t(1) << 31, 28, 131088) == 10, "128 bins, the largest grid");
static_assert(weighted_grid(int64_t(1) << 31, 1, 32792) == 1024 && weighted_grid(int64_t(1) << 31, 3, 65536) == 171 &&
                  weighted_grid(int64_t(1) << 31, 3, 49152) == 256, "the largest histogram; two and three workgroups per CU");
static_assert(weighted_grid(65536, 1, 16384) == 32 && weighted_grid(65536, 4, 16384) == 32, "a small population: the items decide");

template <class Slots>
inline int launch_weighted_count(const float* x, int64_t stride, int32_t dim, const float* w, int64_t n, double scale, const Slots& slots,
                                 int n_slots, uint64_t* counts, hipStream_t s)
{
    const size_t lds_bytes = (size_t)n_slots * sizeof(unsigned long long);
    static LdsGrant grant;                               // per instantiation and per device
    if (!grant_dynamic_lds(grant, (const void*)weighted_count_kernel<Slots>, lds_bytes)) return GLABC_ERR_LAUNCH;
    const unsigned g = weighted_grid(n, dim, lds_bytes);
    hipLaunchKernelGGL((weighted_count_kernel<Slots>), dim3(g, dim), dim3(HISTORY_LANES, HISTORY_WAVES), lds_bytes, s, x, stride, w, n, scale,
                       slots, (unsigned long long*)counts);
    return launch_status();
}

template <int NP>
inline int weighted_key_counts_np(const float* x, int64_t stride, int32_t dim, const float* w, int64_t n, double scale, int32_t level,
                                  int32_t n_prefixes, const uint32_t* prefixes, uint64_t* counts, hipStream_t s)
{
    return launch_weighted_count<KeySlots<NP>>(x, stride, dim, w, n, scale, key_slots<NP>(dim, level, n_prefixes, prefixes),
                                               n_prefixes << key_digit_bits(level), counts, s);
}

}  // namespace glabc

using namespace glabc;

extern "C" {

__attribute__((visibility("default"))) int glabc_weighted_key_counts(const float* x, int64_t stride, int32_t dim, const float* w, int64_t n,
                                                                     double scale, int32_t level, int32_t n_prefixes,
                                                                     const uint32_t* prefixes, uint64_t* counts, void* stream)
{
    if (int e = check_weighted_key_counts(x, stride, dim, w, n, scale, level, n_prefixes, prefixes, counts)) return e;
    if (n == 0) return GLABC_OK;
    hipStream_t s = (hipStream_t)stream;
    if (level == 0) return weighted_key_counts_np<0>(x, stride, dim, w, n, scale, level, n_prefixes, prefixes, counts, s);
    if (n_prefixes == 1) return weighted_key_counts_np<1>(x, stride, dim, w, n, scale, level, n_prefixes, prefixes, counts, s);
    if (n_prefixes == 2) return weighted_key_counts_np<2>(x, stride, dim, w, n, scale, level, n_prefixes, prefixes, counts, s);
    if (n_prefixes <= 4) return weighted_key_counts_np<4>(x, stride, dim, w, n, scale, level, n_prefixes, prefixes, counts, s);
    return weighted_key_counts_np<8>(x, stride, dim, w, n, scale, level, n_prefixes, prefixes, counts, s);
}

__attribute__((visibility("default"))) int glabc_weighted_histogram(const float* x, int64_t stride, int32_t dim, const float* w, int64_t n,
                                                                    double scale, int32_t n_bins, const double* lo, const double* hi,
                                                                    uint64_t* counts, void* stream)
{
    if (int e = check_weighted_histogram(x, stride, dim, w, n, scale, n_bins, lo, hi, counts)) return e;
    if (n == 0) return GLABC_OK;
    return launch_weighted_count<HistSlots>(x, stride, dim, w, n, scale, hist_slots(dim, n_bins, lo, hi), n_bins + 3, counts,
                                            (hipStream_t)stream);
}

__attribute__((visibility("default"))) int glabc_weighted_histogram2d(const float* x, int64_t stride, int32_t dim, const float* w, int64_t n,
                                                                      double scale, int32_t n_pairs, const int32_t* pairs, int32_t n_bins,
                                                                      const double* lo, const double* hi, uint64_t* counts, void* stream)
{
    if (int e = check_weighted_histogram2d(x, stride, dim, w, n, scale, n_pairs, pairs, n_bins, lo, hi, counts)) return e;
    if (n == 0) return GLABC_OK;
    const size_t lds_bytes = ((size_t)n_bins * n_bins + 2) * sizeof(unsigned long long);
    static LdsGrant grant;                               // per device
    if (!grant_dynamic_lds(grant, (const void*)weighted_joint_kernel, lds_bytes)) return GLABC_ERR_LAUNCH;
    const unsigned g = weighted_grid(n, n_pairs, lds_bytes);
    hipLaunchKernelGGL(weighted_joint_kernel, dim3(g, n_pairs), dim3(HISTORY_LANES, HISTORY_WAVES), lds_bytes, (hipStream_t)stream, x, stride, w,
                       n, scale, joint_slots(n_pairs, pairs, n_bins, lo, hi), (unsigned long long*)counts);
    return launch_status();
}

}  // extern "C"
