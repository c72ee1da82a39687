// glabc_weighted_predictive_pack.h -- the host side of weighted_predictive_kernel (glabc_weighted_predictive.h): the record of a call,
// the argument block from the descriptors of include/glabc.h and the bytes of the LDS table.  The built-in entry point
// (glabc_weighted_predictive.hip) and the launch of a run-time compiled weighted predictive program (glabc_rtc.hip) both go through
// this text, so they cannot drift apart.  Host only, never handed to hiprtc.
#pragma once

#include <cstdint>
#include <cstring>

#include "glabc_draws_pack.h"
#include "glabc_weighted_predictive.h"

namespace glabc {

// What glabc_weighted_predictive_counts and its run-time compiled twin are called with
struct WeightedPredCall {
    const glabc_model* model;
    const float* x;
    int64_t stride;
    const float* w;
    int64_t n;
    double scale;
    uint64_t seed;
    int64_t id0;
    int32_t n_bins;
    const double* lo;
    const double* hi;
    const float* threshold;
    uint64_t* counts;
    uint64_t* tails;
    uint32_t* extremes;
};

template <int D, int YD>
inline WeightedPredArgs<D, YD> pack_weighted_pred_args(const WeightedPredCall& c)
{
    constexpr int K = YD + 1;
    WeightedPredArgs<D, YD> a;
    std::memset(&a, 0, sizeof a);
    a.s = pack_draw_model<D, YD>(c.model);
    a.x = c.x, a.w = c.w;
    a.n = c.n, a.stride = c.stride, a.id0 = c.id0;
    a.w_scale = c.scale;
    split_key(c.seed ^ GLABC_PREDICTIVE_KEY, &a.key_lo, &a.key_hi);
    a.counts = (unsigned long long*)c.counts, a.tails = (unsigned long long*)c.tails, a.extremes = c.extremes;
    a.n_bins = c.counts ? c.n_bins : 1;
    for (int k = 0; k < K; ++k) {
        const BinAxis ax = c.counts ? bin_axis(c.lo[k], c.hi[k], a.n_bins) : bin_axis(0.0, 1.0, a.n_bins);
        a.lo[k] = ax.lo, a.hi[k] = ax.hi, a.scale[k] = ax.scale;
        a.thr[k] = c.tails ? c.threshold[k] : 0.0f;
    }
    return a;
}

// the dynamic LDS of a launch: the kernel's own count of its counters (weighted_pred_slots), 8 bytes each
inline size_t weighted_pred_lds_bytes(const WeightedPredCall& c, int y_dim)
{
    return (size_t)weighted_pred_slots(y_dim + 1, c.counts ? c.n_bins : 1, c.counts != nullptr, c.tails != nullptr) *
           sizeof(unsigned long long);
}
static_assert(weighted_pred_slots(GLABC_MAX_DIM + 1, GLABC_MAX_WEIGHTED_PREDICTIVE_BINS, true, true) * sizeof(unsigned long long) == 37368 &&
                  37368 <= 48 * 1024, "the largest table is what a launch gets without a grant");

}  // namespace glabc
