// glabc_predictive.h -- predictive_kernel<D, YD, R>: the kernel of the posterior predictive checks, as glabc_predictive.hip instantiates
// it for the built-in simulators (glabc_predictive_draws / glabc_predictive_counts) and as hiprtc instantiates it around a user's simulator
// (glabc_rtc_compile_predictive, glabc_rtc_kernel.h).  include/glabc.h holds the specification of a predictive draw and of the three
// integer tables.  No host includes: the header is handed to hiprtc as text.
//
// glabc_joint.hip's joint_kernel around the draw of glabc_abc.h's abc_draws_kernel: lanes run along the chain index; the walk over
// items of 64 chains x R rows, the guarded loads, the uint32 table in LDS, the grid rule, the key and glabc_histogram's bin arithmetic
// are glabc_history.h's, which argues what cannot be read, that a slot is inside the table and that no counter wraps.  An item loads the
// D row segments of its R rows, all issued together; a lane outside the segment stores and counts nothing.  Then, per lane and row: the
// noise of a draw (draw_noise of glabc_draw.h, what abc_draws_kernel calls) under the predictive key, model_simulate and
// model_discrepancy_rows of glabc_device.h -- the functions glabc_model_simulate / glabc_model_discrepancy inline, which is what makes the
// bits agree with their composition.  In a run-time compiled build these three are the user's: NoiseDim is GLABC_USER_NOISE_DIM,
// model_simulate calls glabc_user_simulate, and model_discrepancy_rows the user's distance where the source announces
// GLABC_USER_DISCREPANCY, as in abc_draws_kernel.
//
// Rows per item.  R is a template parameter, and every row's draw is inlined: R copies of the simulator.  The built-in kernels take
// R = pred_rows(D) = 16 / D (about 16 loads in flight per item around a simulator of a few hundred instructions); a run-time compiled
// program takes R = 1 whatever the source (glabc_rtc_predictive_kernels.h, profiles/rtc_predictive_kernel_resources.txt).  x[r][j] is
// indexed by unrolled loop counters only.  A draw's bits do not depend on R: its id is id0 + t id_step + c.
// Outputs.  Which are wanted is wave-uniform (a NULL pointer in the argument block), as in abc_draws_kernel:
//   y, dis     plain stores in the history's layout (glabc_predictive_draws)
//   counts     K = YD + 1 tables of n_bins + 3 uint32 counters in LDS (at most 9 x 1027 x 4 = 36 972 bytes: what a launch gets
//              unasked), one LDS atomic per statistic and draw
//   tails      three ballots and population counts per statistic and row into wave-uniform counters, flushed once per wavefront; the
//              NaN slot is the wavefront's draws less the three
//   extremes   the smallest and largest key per lane, reduced across the wavefront at the end, one atomicMin / atomicMax per
//              wavefront and statistic
// Integer adds, minima and maxima commute: the tables are the same bits in every order and for every grid.
// The by-value argument arrays are indexed by unrolled loop counters only, so the block stays in scalar registers;
// profiles/predictive_kernel_resources.txt holds the compiler's resource report.
#pragma once

#include "glabc_device.h"
#include "glabc_draw.h"
#include "glabc_history.h"

namespace glabc {

constexpr int PRED_LOADS = 16;          // loads in flight per item, as count_kernel's and joint_kernel's 16
constexpr int64_t PRED_MAX_ITEMS_PER_WAVE = 1 << 18;     // x HISTORY_WAVES x 16 rows x HISTORY_LANES = 2^31 draws per workgroup

// rows per item of the built-in kernels: 16, 8, 5, 4, 3, 2, 2, 2 at D = 1 .. 8
constexpr int pred_rows(int D) { return PRED_LOADS / D; }

template <int D, int YD>
struct PredArgs {
    StepArgs<D, YD> s;            // the Model as the samplers' kernels see it: simulator, y_obs
    const float* hist;
    int64_t n_rows, row_step, n_chains, stride;
    int64_t id0, id_step;
    uint32_t key_lo, key_hi;      // seed ^ GLABC_PREDICTIVE_KEY
    float* y;                     // glabc_predictive_draws
    float* dis;
    int64_t y_stride, dis_stride;
    unsigned long long* counts;   // glabc_predictive_counts
    unsigned long long* tails;
    uint32_t* extremes;
    int32_t n_bins;
    double lo[YD + 1], hi[YD + 1], scale[YD + 1];
    float thr[YD + 1];
};

template <int D, int YD, int R>
__global__ void __launch_bounds__(HISTORY_LANES* HISTORY_WAVES) predictive_kernel(const PredArgs<D, YD> a)
{
    static_assert(R >= 1 && R <= PRED_LOADS, "PRED_MAX_ITEMS_PER_WAVE bounds a workgroup's draws for items of at most 16 rows");
    constexpr int K = YD + 1;
    extern __shared__ uint32_t table[];
    const int n_bins = a.n_bins;
    const int n_slots = a.counts ? K * (n_bins + 3) : 0;          // no counts: no LDS was asked for
    // table_zero's text, not a call of it, which changes the scalar code around the select above (profiles/history_header_device_code.txt)
    for (int i = threadIdx.y * HISTORY_LANES + threadIdx.x; i < n_slots; i += HISTORY_LANES * HISTORY_WAVES) table[i] = 0u;
    __syncthreads();

    const bool want_stats = a.counts || a.tails || a.extremes;
    const bool want_dis = a.dis || want_stats;                   // else (y alone) the distance is not formed
    uint32_t tail[K][3];                                          // wave-uniform: x < thr, x == thr, x > thr
    uint32_t key_min[K], key_max[K];                              // per lane
#pragma unroll
    for (int k = 0; k < K; ++k) {
        tail[k][0] = tail[k][1] = tail[k][2] = 0u;
        key_min[k] = 0xFFFFFFFFu, key_max[k] = 0u;
    }
    uint32_t n_live = 0u;                                         // wave-uniform: the draws this wavefront has made

    const unsigned lane = threadIdx.x;
    const Walk<R> walk(a.n_rows, a.n_chains);
    for (int64_t item = walk.first; item < walk.n_items; item += walk.n_waves) {
        const Item it = walk.item(item);
        const float* p = a.hist + it.row0 * a.row_step + it.chain0;
        float x[R][D];
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int j = 0; j < D; ++j) x[r][j] = load_segment(p + j * a.stride, it.bytes(r), lane);
            p += it.step(r, a.row_step);
        }
        const bool inside = (int)lane < it.live;
        const int64_t c = it.chain0 + lane;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (r < it.rows) {                                    // wave-uniform
                const int64_t t = it.row0 + r;
                const uint64_t id = (uint64_t)(a.id0 + t * a.id_step + c);

                // y: glabc_model_simulate(eps = NULL) under the predictive key, the noise of a draw (glabc_draw.h)
                float eps[NoiseDim<YD>::value], theta[D], v[K];   // v: the statistics, y and then the distance
                draw_noise<YD>(id, a.key_lo, a.key_hi, eps);
#pragma unroll
                for (int j = 0; j < D; ++j) theta[j] = x[r][j];
                {
                    float y[YD];
                    model_simulate<D, YD>(a.s, theta, eps, y);
                    if (a.y && inside) {
#pragma unroll
                        for (int j = 0; j < YD; ++j) a.y[(t * YD + j) * a.y_stride + c] = y[j];
                    }
#pragma unroll
                    for (int j = 0; j < YD; ++j) v[j] = y[j];
                    if (want_dis) v[YD] = model_discrepancy_rows<YD>(y, a.s.y_obs);
                }
                if (a.dis && inside) a.dis[t * a.dis_stride + c] = v[YD];
                if (want_stats) n_live += (uint32_t)it.live;
                if (a.counts) {
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const int slot = hist_slot(v[k], BinAxis{a.lo[k], a.hi[k], a.scale[k]}, n_bins);      // below n_bins + 3
                        if (inside) atomicAdd(&table[k * (n_bins + 3) + slot], 1u);
                    }
                }
                if (a.tails) {
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        tail[k][0] += (uint32_t)__builtin_popcountll(__ballot(inside && v[k] < a.thr[k]));
                        tail[k][1] += (uint32_t)__builtin_popcountll(__ballot(inside && v[k] == a.thr[k]));
                        tail[k][2] += (uint32_t)__builtin_popcountll(__ballot(inside && v[k] > a.thr[k]));
                    }
                }
                if (a.extremes) {
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const uint32_t key = float_key(v[k]);
                        const bool counted = inside && key != 0xFFFFFFFFu;
                        key_min[k] = counted && key < key_min[k] ? key : key_min[k];
                        key_max[k] = counted && key > key_max[k] ? key : key_max[k];
                    }
                }
            }
        }
    }

    if (a.tails && lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const uint32_t n_nan = n_live - tail[k][0] - tail[k][1] - tail[k][2];
#pragma unroll
            for (int s = 0; s < 3; ++s)
                if (tail[k][s]) atomicAdd(&a.tails[k * 4 + s], (unsigned long long)tail[k][s]);
            if (n_nan) atomicAdd(&a.tails[k * 4 + 3], (unsigned long long)n_nan);
        }
    }
    if (a.extremes) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            uint32_t lo = key_min[k], hi = key_max[k];
#pragma unroll
            for (int m = HISTORY_LANES / 2; m >= 1; m >>= 1) {
                const uint32_t other_lo = (uint32_t)__shfl_xor((int)lo, m), other_hi = (uint32_t)__shfl_xor((int)hi, m);
                lo = other_lo < lo ? other_lo : lo;
                hi = other_hi > hi ? other_hi : hi;
            }
            if (lane == 0 && lo != 0xFFFFFFFFu) {                 // a wavefront that met a value that is no NaN
                atomicMin(&a.extremes[2 * k], lo);
                atomicMax(&a.extremes[2 * k + 1], hi);
            }
        }
    }
    if (!a.counts) return;                                        // wave-uniform, the whole grid alike
    table_flush(table, n_slots, a.counts);
}

// workgroups (history_grid); its bound on a wavefront's items is what the uint32 tails and n_live need too
constexpr unsigned predictive_grid(int64_t n_rows, int64_t n_chains, int rows_per_item, size_t lds_bytes)
{
    return history_grid(history_items(n_rows, n_chains, rows_per_item), HISTORY_WAVES, PRED_MAX_ITEMS_PER_WAVE,
                        HISTORY_CUS * workgroups_per_cu(lds_bytes));
}

}  // namespace glabc
