// glabc_predictive_pack.h -- the host side of predictive_kernel (glabc_predictive.h): the record of a call, the argument block from
// the descriptors of include/glabc.h and the bytes of the LDS table.  The built-in entry points (glabc_predictive.hip) and the launch
// of a run-time compiled predictive program (glabc_rtc.hip) both go through this text, so they cannot drift apart.  Host only, never
// handed to hiprtc.
#pragma once

#include <cstdint>
#include <cstring>

#include "glabc_draws_pack.h"
#include "glabc_predictive.h"

namespace glabc {

// What glabc_predictive_draws / glabc_predictive_counts and their run-time compiled twins are called with
struct PredCall {
    const glabc_model* model;
    const float* history;
    int64_t n_rows, n_chains, stride;
    uint64_t seed;
    int64_t id0, id_step;
    float* y;
    float* dis;
    int64_t y_stride, dis_stride;
    int32_t n_bins;
    const double* lo;
    const double* hi;
    const float* threshold;
    uint64_t* counts;
    uint64_t* tails;
    uint32_t* extremes;
};

template <int D, int YD>
inline PredArgs<D, YD> pack_pred_args(const PredCall& c)
{
    constexpr int K = YD + 1;
    PredArgs<D, YD> a;
    std::memset(&a, 0, sizeof a);
    a.s = pack_draw_model<D, YD>(c.model);
    a.hist = c.history;
    a.n_rows = c.n_rows, a.row_step = (int64_t)D * c.stride, a.n_chains = c.n_chains, a.stride = c.stride;
    a.id0 = c.id0, a.id_step = c.id_step;
    split_key(c.seed ^ GLABC_PREDICTIVE_KEY, &a.key_lo, &a.key_hi);
    a.y = c.y, a.dis = c.dis, a.y_stride = c.y_stride, a.dis_stride = c.dis_stride;
    a.counts = (unsigned long long*)c.counts, a.tails = (unsigned long long*)c.tails, a.extremes = c.extremes;
    a.n_bins = c.counts ? c.n_bins : 1;
    for (int k = 0; k < K; ++k) {
        const BinAxis ax = c.counts ? bin_axis(c.lo[k], c.hi[k], a.n_bins) : bin_axis(0.0, 1.0, a.n_bins);
        a.lo[k] = ax.lo, a.hi[k] = ax.hi, a.scale[k] = ax.scale;
        a.thr[k] = c.tails ? c.threshold[k] : 0.0f;
    }
    return a;
}

// the dynamic LDS of a launch: the K tables of a call that asks for counts, nothing otherwise
inline size_t pred_lds_bytes(const PredCall& c, int y_dim)
{
    return c.counts ? (size_t)(y_dim + 1) * (c.n_bins + 3) * sizeof(uint32_t) : 0;
}

}  // namespace glabc
