// glabc_weighted_walk.h -- what the kernels over weighted draws share (glabc_weighted.hip, glabc_weighted_predictive.h): the quantised
// weight of include/glabc.h, the walk over items of 64 x S consecutive draws, and glabc_history.h's three table helpers on 64-bit
// counters in LDS.  Host and device, no host includes: handed to hiprtc as text with glabc_weighted_predictive.h (a run-time compiled
// weighted predictive program); glabc_slots.h includes it for the host's side of the quantised weight.
#pragma once

#include "glabc_history.h"

namespace glabc {

// ---- the quantised weight of the weighted entry points (include/glabc.h): the multiplicity a draw of float32 weight w counts
// with.  One rounded product (the objects are built with -ffp-contract=off), ties to even; zero, negative and NaN weights count
// nothing, and the clamp keeps a multiplicity inside 32 bits so that 2^31 of them cannot wrap a uint64
__host__ __device__ inline uint64_t weight_multiplicity(float w, double scale)
{
    const double v = (double)w * scale;
    if (!(w > 0.0f)) return 0u;
    if (v >= 4294967295.0) return 0xFFFFFFFFull;
    return (uint64_t)(uint32_t)__builtin_rint(v);
}

// ---- the walk over the draws: item i holds draws [i * 64 S, min(n, (i + 1) * 64 S)), S 64-draw segments.  All wave-uniform
template <int S>
constexpr int64_t draw_items(int64_t n)
{
    return (n + (int64_t)HISTORY_LANES * S - 1) / ((int64_t)HISTORY_LANES * S);
}

template <int S>
struct DrawItemOf {
    int64_t draw0;
    int draws;                          // draws inside the item: 1 .. 64 S
    // segment r is loaded with bytes(r) bytes at offset at(r) from the item's first draw: a segment past the end has the item's own
    // address and no bytes, and only a lane below live(r) may count what it loaded
    __device__ int live(int r) const
    {
        const int left = draws - r * HISTORY_LANES;
        return left < 0 ? 0 : left < HISTORY_LANES ? left : HISTORY_LANES;
    }
    __device__ int bytes(int r) const { return 4 * live(r); }
    __device__ int64_t at(int r) const { return draw0 + (live(r) ? r * HISTORY_LANES : 0); }
};

template <int S>
struct DrawWalkOf {
    static constexpr int64_t ITEM = (int64_t)HISTORY_LANES * S;
    const int64_t n;
    const int64_t n_items = draw_items<S>(n);
    const int64_t n_waves = (int64_t)gridDim.x * HISTORY_WAVES;
    const int64_t first = (int64_t)blockIdx.x * HISTORY_WAVES + __builtin_amdgcn_readfirstlane((int)threadIdx.y);          // this wavefront's

    __device__ explicit DrawWalkOf(int64_t draws) : n(draws) {}
    __device__ DrawItemOf<S> item(int64_t i) const
    {
        const int64_t draw0 = i * ITEM;
        return DrawItemOf<S>{draw0, (int)(n - draw0 < ITEM ? n - draw0 : ITEM)};
    }
};

// ---- the table: glabc_history.h's three helpers on 64-bit counters; every LDS store of the weighted kernels goes through them
__device__ __forceinline__ void table_zero(unsigned long long* table, int n_slots)
{
    const int tid = threadIdx.y * HISTORY_LANES + threadIdx.x;
    for (int i = tid; i < n_slots; i += HISTORY_LANES * HISTORY_WAVES) table[i] = 0ull;
    __syncthreads();
}

// slot < 0: nothing to add.  A caller's slot function returns an index below the n_slots the table was launched with
__device__ __forceinline__ void lds_add(unsigned long long* table, int slot, unsigned long long m)
{
    if (slot >= 0) atomicAdd(&table[slot], m);
}

__device__ __forceinline__ void table_flush(const unsigned long long* table, int n_slots, unsigned long long* out)
{
    __syncthreads();
    const int tid = threadIdx.y * HISTORY_LANES + threadIdx.x;
    for (int i = tid; i < n_slots; i += HISTORY_LANES * HISTORY_WAVES) {
        const unsigned long long c = table[i];
        if (c) atomicAdd(&out[i], c);
    }
}

// the multiplicity lane `lane` of segment r counts with: 0 outside the segment, whatever the load returned
template <int S>
__device__ __forceinline__ unsigned long long lane_multiplicity(const DrawItemOf<S>& it, int r, unsigned lane, float w, double scale)
{
    return (int)lane < it.live(r) ? (unsigned long long)weight_multiplicity(w, scale) : 0ull;
}

}  // namespace glabc
