// glabc_weighted_predictive.h -- weighted_predictive_kernel<D, YD, S>: the posterior predictive check of weighted draws, as
// glabc_weighted_predictive.hip instantiates it for the built-in simulators (glabc_weighted_predictive_counts) and as hiprtc
// instantiates it around a user's simulator (glabc_rtc_compile_weighted_predictive, glabc_rtc_kernel.h).  include/glabc.h holds the
// specification.  No host includes: the header is handed to hiprtc as text.
//
// predictive_kernel's draw (glabc_predictive.h) inside glabc_weighted.hip's counting: lanes run along the draws; the walk over items of
// S consecutive 64-draw segments, the 64-bit LDS counters and the quantised weight are glabc_weighted_walk.h's, the guarded load, the
// key and the bin arithmetic glabc_history.h's.  An item loads the D theta segments and the weight segment of each of its S segments,
// (D + 1) S loads all issued together, each through a descriptor over exactly the segment's bytes: a padding column, the floats
// behind the last draw and a whole segment past the end cannot be read.  Then, per segment:
//   m = the lane's multiplicity (0 outside the segment, whatever the load returned)
//   no lane of the wavefront with m != 0: the segment is left before any noise is drawn (wave-uniform; it saves work only, a lane
//   with m == 0 adds nothing anywhere below either)
//   otherwise draw_noise under the predictive key with the id id0 + i, model_simulate, model_discrepancy_rows: the very calls of
//   predictive_kernel on the history [1][D][stride], which is what makes a draw the same bits as the unweighted twin's
// Outputs.  Which are wanted is wave-uniform (a NULL pointer in the argument block):
//   counts     K = YD + 1 tables of n_bins + 3 `unsigned long long` counters in LDS, one LDS atomic per statistic and draw of m != 0
//   tails      four more LDS counters per statistic behind the counts' (slot k * 4 + s), one LDS atomic of m per statistic and draw.
//              predictive_kernel's ballot and population count does not carry over to sums of m; per-lane accumulators would be
//              3 K + 1 64-bit sums, 56 vector registers at K = 9 held across the simulator, where the LDS slots cost none
//              (profiles/weighted_predictive_kernel_resources.txt)
//   extremes   the smallest and largest key per lane over draws with m != 0 that are no NaN, reduced across the wavefront at the end
// The table is at most 9 x (512 + 3 + 4) x 8 = 37 368 bytes (GLABC_MAX_WEIGHTED_PREDICTIVE_BINS): what a launch gets unasked.
// Safety.  A count's slot is k (n_bins + 3) + hist_slot < K (n_bins + 3), a tail's K (n_bins + 3) + 4 k + s with s < 4: inside the
// n_slots the host sized the LDS from (weighted_pred_slots, one function for both).  A counter cannot wrap: n <= 2^31 draws of at
// most 2^32 - 1 each stay below 2^63.  Integer adds, minima and maxima commute: the tables are the same bits for every grid and S.
#pragma once

#include "glabc_device.h"
#include "glabc_draw.h"
#include "glabc_history.h"
#include "glabc_predictive.h"          // PRED_LOADS and pred_rows: the built-in kernels' segments per item are its rows per item
#include "glabc_weighted_walk.h"

namespace glabc {

template <int D, int YD>
struct WeightedPredArgs {
    StepArgs<D, YD> s;            // the Model as the samplers' kernels see it: simulator, y_obs
    const float* x;               // [D][stride]
    const float* w;
    int64_t n, stride, id0;
    double w_scale;
    uint32_t key_lo, key_hi;      // seed ^ GLABC_PREDICTIVE_KEY
    unsigned long long* counts;
    unsigned long long* tails;
    uint32_t* extremes;
    int32_t n_bins;
    double lo[YD + 1], hi[YD + 1], scale[YD + 1];
    float thr[YD + 1];
};

// the LDS counters of a launch: the K tables of a call that asks for counts, then four per statistic of a call that asks for tails
constexpr int weighted_pred_slots(int n_stats, int n_bins, bool counts, bool tails)
{
    return (counts ? n_stats * (n_bins + 3) : 0) + (tails ? n_stats * 4 : 0);
}

template <int D, int YD, int S>
__global__ void __launch_bounds__(HISTORY_LANES* HISTORY_WAVES) weighted_predictive_kernel(const WeightedPredArgs<D, YD> a)
{
    static_assert(S >= 1 && S * (D + 1) <= 2 * PRED_LOADS, "the loads of an item are all in flight together");
    constexpr int K = YD + 1;
    extern __shared__ unsigned long long weighted_pred_table[];
    const int n_bins = a.n_bins;
    const int n_count_slots = weighted_pred_slots(K, n_bins, a.counts != nullptr, false);
    const int n_slots = weighted_pred_slots(K, n_bins, a.counts != nullptr, a.tails != nullptr);
    unsigned long long* const tail_table = weighted_pred_table + n_count_slots;
    table_zero(weighted_pred_table, n_slots);

    uint32_t key_min[K], key_max[K];                              // per lane
#pragma unroll
    for (int k = 0; k < K; ++k) key_min[k] = 0xFFFFFFFFu, key_max[k] = 0u;

    const unsigned lane = threadIdx.x;
    const DrawWalkOf<S> walk(a.n);
    for (int64_t item = walk.first; item < walk.n_items; item += walk.n_waves) {
        const DrawItemOf<S> it = walk.item(item);
        float x[S][D], wv[S];
#pragma unroll
        for (int r = 0; r < S; ++r) {
#pragma unroll
            for (int j = 0; j < D; ++j) x[r][j] = load_segment(a.x + j * a.stride + it.at(r), it.bytes(r), lane);
            wv[r] = load_segment(a.w + it.at(r), it.bytes(r), lane);
        }
#pragma unroll
        for (int r = 0; r < S; ++r) {
            const unsigned long long m = lane_multiplicity(it, r, lane, wv[r], a.w_scale);
            if (__ballot(m != 0ull) != 0ull) {                    // wave-uniform: a segment of no weight draws no noise
                const uint64_t id = (uint64_t)a.id0 + (uint64_t)(it.draw0 + r * HISTORY_LANES + lane);      // id0 + i

                // predictive_kernel's draw: glabc_model_simulate(eps = NULL) under the predictive key, then the distance
                float eps[NoiseDim<YD>::value], theta[D], v[K];   // v: the statistics, y and then the distance
                draw_noise<YD>(id, a.key_lo, a.key_hi, eps);
#pragma unroll
                for (int j = 0; j < D; ++j) theta[j] = x[r][j];
                {
                    float y[YD];
                    model_simulate<D, YD>(a.s, theta, eps, y);
#pragma unroll
                    for (int j = 0; j < YD; ++j) v[j] = y[j];
                    v[YD] = model_discrepancy_rows<YD>(y, a.s.y_obs);
                }
                if (a.counts) {
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const int slot = hist_slot(v[k], BinAxis{a.lo[k], a.hi[k], a.scale[k]}, n_bins);      // below n_bins + 3
                        lds_add(weighted_pred_table, m ? k * (n_bins + 3) + slot : -1, m);
                    }
                }
                if (a.tails) {
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const int s = v[k] < a.thr[k] ? 0 : v[k] == a.thr[k] ? 1 : v[k] > a.thr[k] ? 2 : 3;
                        lds_add(tail_table, m ? k * 4 + s : -1, m);
                    }
                }
                if (a.extremes) {
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const uint32_t key = float_key(v[k]);
                        const bool counted = m != 0ull && key != 0xFFFFFFFFu;      // m != 0 only inside the segment
                        key_min[k] = counted && key < key_min[k] ? key : key_min[k];
                        key_max[k] = counted && key > key_max[k] ? key : key_max[k];
                    }
                }
            }
        }
    }

    if (a.extremes) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uint32_t lo = key_min[k], hi = key_max[k];
#pragma unroll
            for (int d = HISTORY_LANES / 2; d >= 1; d >>= 1) {
                const uint32_t other_lo = (uint32_t)__shfl_xor((int)lo, d), other_hi = (uint32_t)__shfl_xor((int)hi, d);
                lo = other_lo < lo ? other_lo : lo;
                hi = other_hi > hi ? other_hi : hi;
            }
            if (lane == 0 && lo != 0xFFFFFFFFu) {                 // a wavefront that met a counted value that is no NaN
                atomicMin(&a.extremes[2 * k], lo);
                atomicMax(&a.extremes[2 * k + 1], hi);
            }
        }
    }
    if (n_slots == 0) return;                                     // wave-uniform, the whole grid alike
    if (a.counts) table_flush(weighted_pred_table, n_count_slots, a.counts);
    if (a.tails) table_flush(tail_table, n_slots - n_count_slots, a.tails);
}

// workgroups: glabc_weighted.hip's weighted_grid at one table and items of S segments -- what fills the part, as many workgroups per
// CU as the table lets in, and no more than there are items to give every wavefront one.  No lower bound: a 64-bit counter cannot wrap
constexpr unsigned weighted_predictive_grid(int64_t n, int segments, size_t lds_bytes)
{
    const int64_t item = (int64_t)HISTORY_LANES * segments;
    const int64_t most = ((n + item - 1) / item + HISTORY_WAVES - 1) / HISTORY_WAVES;
    const int64_t fill = HISTORY_CUS * workgroups_per_cu(lds_bytes);
    return (unsigned)(fill > most ? most : fill);
}

}  // namespace glabc
