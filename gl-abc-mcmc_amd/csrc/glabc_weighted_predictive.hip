// glabc_weighted_predictive.hip -- posterior predictive checks of weighted draws: glabc_weighted_predictive_counts of include/glabc.h,
// which holds the specification.
//
// weighted_predictive_kernel<D, YD, S> is glabc_weighted_predictive.h's, which hiprtc instantiates around a user's simulator too
// (glabc_rtc.hip); this object instantiates it for the built-in simulators at S = pred_rows(D) segments per item, through the packer
// both share (glabc_weighted_predictive_pack.h).  profiles/weighted_predictive_kernel_resources.txt holds the compiler's resource report.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "glabc_check.h"
#include "glabc_device.h"
#include "glabc_dispatch.h"
#include "glabc_draws_pack.h"
#include "glabc_history.h"
#include "glabc_launch.h"
#include "glabc_weighted_predictive.h"
#include "glabc_weighted_predictive_pack.h"

namespace glabc {

// the grid rule (glabc_weighted_predictive.h): weighted_grid's at one table, items of `segments` 64-draw segments
static_assert(weighted_predictive_grid(1, 16, 0) == 1 && weighted_predictive_grid(8 * 64 * 16, 16, 37368) == 1 &&
                  weighted_predictive_grid(8 * 64 * 16 + 1, 16, 37368) == 2 && weighted_predictive_grid(8 * 64 * 2 + 1, 2, 0) == 2 &&
                  weighted_predictive_grid(8 * 64 + 1, 1, 32) == 2,
              "one item, one workgroup's first round and one draw more");
static_assert(weighted_predictive_grid(int64_t(1) << 31, 16, 37368) == 1024 && weighted_predictive_grid(int64_t(1) << 31, 1, 0) == 1024 &&
                  weighted_predictive_grid(int64_t(1) << 31, 2, 37368) == 1024,
              "the most draws: four workgroups per CU, whatever the table (at most 37 368 bytes)");
static_assert(weighted_predictive_grid(65536, 8, 1560) == 16 && weighted_predictive_grid(65536, 1, 1560) == 128 &&
                  weighted_predictive_grid(1 << 21, 8, 1560) == 512,
              "a small population: the items decide");

template <int D, int YD>
inline int launch_weighted_predictive(const WeightedPredCall& c, hipStream_t s)
{
    const WeightedPredArgs<D, YD> a = pack_weighted_pred_args<D, YD>(c);
    const size_t lds_bytes = weighted_pred_lds_bytes(c, YD);
    const unsigned g = weighted_predictive_grid(c.n, pred_rows(D), lds_bytes);
    hipLaunchKernelGGL((weighted_predictive_kernel<D, YD, pred_rows(D)>), dim3(g), dim3(HISTORY_LANES, HISTORY_WAVES), lds_bytes, s, a);
    return launch_status();
}

inline int dispatch_weighted_predictive(const WeightedPredCall& c, hipStream_t s)
{
    if (c.model->sim_kind == GLABC_SIM_GK) return launch_weighted_predictive<4, 8>(c, s);
    return dispatch_range<1, 8>(c.model->theta_dim, GLABC_ERR_DIM, [&](auto d) {
        constexpr int D = decltype(d)::value;
        return launch_weighted_predictive<D, D>(c, s);
    });
}

}  // namespace glabc

using namespace glabc;

extern "C" {

__attribute__((visibility("default"))) int glabc_weighted_predictive_counts(const glabc_model* model, const float* x, int64_t stride,
                                                                            int32_t theta_dim, const float* w, int64_t n, double scale,
                                                                            uint64_t seed, int64_t id0, int32_t n_bins, const double* lo,
                                                                            const double* hi, const float* threshold, uint64_t* counts,
                                                                            uint64_t* tails, uint32_t* extremes, void* stream)
{
    if (int e = check_weighted_predictive_counts(model, x, stride, theta_dim, w, n, scale, id0, n_bins, lo, hi, threshold, counts, tails,
                                                 extremes))
        return e;
    if (n == 0) return GLABC_OK;
    const WeightedPredCall c{model, x, stride, w, n, scale, seed, id0, n_bins, lo, hi, threshold, counts, tails, extremes};
    return dispatch_weighted_predictive(c, (hipStream_t)stream);
}

}  // extern "C"
