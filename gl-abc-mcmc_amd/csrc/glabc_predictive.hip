// glabc_predictive.hip -- posterior predictive checks: glabc_predictive_draws and glabc_predictive_counts of include/glabc.h, which
// holds the specification of a predictive draw and of the three integer tables.
//
// predictive_kernel<D, YD, R> is glabc_predictive.h's, which hiprtc instantiates around a user's simulator too (glabc_rtc.hip); this
// object instantiates it for the built-in simulators at R = pred_rows(D) rows per item, through the packer both share
// (glabc_predictive_pack.h).  profiles/predictive_kernel_resources.txt holds the compiler's resource report.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "glabc_check.h"
#include "glabc_device.h"
#include "glabc_dispatch.h"
#include "glabc_draws_pack.h"
#include "glabc_history.h"
#include "glabc_launch.h"
#include "glabc_predictive.h"
#include "glabc_predictive_pack.h"

namespace glabc {

// the grid rule (glabc_predictive.h), pinned at what predictive_grid's own arithmetic gave before it called history_grid (four workgroups per CU, whatever the table)
static_assert(predictive_grid(1, 1, 16, 0) == 1 && predictive_grid(2, 64, 2, 36972) == 1 && predictive_grid(16, 7 * 64, 16, 16) == 1 &&
                  predictive_grid(16, 9 * 64, 16, 16) == 2, "one item, HISTORY_WAVES - 1 and + 1 items");
static_assert(predictive_grid(1 << 20, 65536, 16, 36972) == 1024 && predictive_grid(1 << 20, 65536, 2, 36972) == 1024 &&
                  predictive_grid(1 << 20, 65536, 5, 0) == 1024 && predictive_grid(1 << 20, 65536, 4, 144) == 1024,
              "theta_dim 1 and 8 with the largest table, no table, the smallest");
static_assert(predictive_grid(1 << 19, 1ll << 26, 16, 36972) == 16384 && predictive_grid(1 << 16, 1ll << 26, 2, 0) == 16384,
              "the counters' bound wins");

template <int D, int YD>
inline int launch_predictive(const PredCall& c, hipStream_t s)
{
    const PredArgs<D, YD> a = pack_pred_args<D, YD>(c);
    const size_t lds_bytes = pred_lds_bytes(c, YD);
    const unsigned g = predictive_grid(c.n_rows, c.n_chains, pred_rows(D), lds_bytes);
    hipLaunchKernelGGL((predictive_kernel<D, YD, pred_rows(D)>), dim3(g), dim3(HISTORY_LANES, HISTORY_WAVES), lds_bytes, s, a);
    return launch_status();
}

inline int dispatch_predictive(const PredCall& c, hipStream_t s)
{
    if (c.model->sim_kind == GLABC_SIM_GK) return launch_predictive<4, 8>(c, s);
    return dispatch_range<1, 8>(c.model->theta_dim, GLABC_ERR_DIM, [&](auto d) {
        constexpr int D = decltype(d)::value;
        return launch_predictive<D, D>(c, s);
    });
}

}  // namespace glabc

using namespace glabc;

extern "C" {

__attribute__((visibility("default"))) int glabc_predictive_draws(const glabc_model* model, const float* history, int64_t n_rows,
                                                                  int32_t theta_dim, int64_t n_chains, int64_t stride, uint64_t seed,
                                                                  int64_t id0, int64_t id_step, float* y_out, int64_t y_stride,
                                                                  float* dis_out, int64_t dis_stride, void* stream)
{
    if (int e = check_predictive_draws(model, history, n_rows, theta_dim, n_chains, stride, id0, id_step, y_out, y_stride, dis_out, dis_stride))
        return e;
    if (n_chains == 0) return GLABC_OK;
    const PredCall c{model, history, n_rows, n_chains, stride, seed, id0, id_step, y_out, dis_out, y_stride, dis_stride,
                     0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return dispatch_predictive(c, (hipStream_t)stream);
}

__attribute__((visibility("default"))) int glabc_predictive_counts(const glabc_model* model, const float* history, int64_t n_rows,
                                                                   int32_t theta_dim, int64_t n_chains, int64_t stride, uint64_t seed,
                                                                   int64_t id0, int64_t id_step, int32_t n_bins, const double* lo,
                                                                   const double* hi, const float* threshold, uint64_t* counts,
                                                                   uint64_t* tails, uint32_t* extremes, void* stream)
{
    if (int e = check_predictive_counts(model, history, n_rows, theta_dim, n_chains, stride, id0, id_step, n_bins, lo, hi, threshold, counts,
                                        tails, extremes))
        return e;
    if (n_chains == 0) return GLABC_OK;
    const PredCall c{model, history, n_rows, n_chains, stride, seed, id0, id_step, nullptr, nullptr, 0, 0,
                     n_bins, lo, hi, threshold, counts, tails, extremes};
    return dispatch_predictive(c, (hipStream_t)stream);
}

}  // extern "C"
