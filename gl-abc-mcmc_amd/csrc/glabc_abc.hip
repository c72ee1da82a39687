// glabc_abc.hip -- plain rejection ABC: glabc_abc_draws of include/glabc.h, which holds the specification of a draw.
//
// The kernel, abc_draws_kernel<D, YD>, lives in glabc_abc.h (a run-time compiled draws program instantiates it too, glabc_rtc.hip);
// this file holds its nine built-in instantiations -- |theta| + noise at theta_dim 1 .. 8 and g-and-k --, the launcher and the entry point.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "glabc_abc.h"
#include "glabc_check.h"
#include "glabc_dispatch.h"
#include "glabc_draws_pack.h"
#include "glabc_launch.h"

namespace glabc {

template <int D, int YD>
inline int launch_abc(const glabc_model* m, uint64_t seed, int64_t row0, const int64_t* ids, int64_t n, int64_t stride, float* theta,
                      float* y, float* dis, uint8_t* accept, hipStream_t s)
{
    AbcArgs<D, YD> a = pack_abc_args<D, YD>(m, seed, row0, ids, n, stride, theta, y, dis, accept);
    for (a.first = 0; a.first < n; a.first += ABC_MAX_LAUNCH) {
        const int64_t part = n - a.first < ABC_MAX_LAUNCH ? n - a.first : ABC_MAX_LAUNCH;
        hipLaunchKernelGGL((abc_draws_kernel<D, YD>), dim3(grid_for(part, ABC_BLOCK)), dim3(ABC_BLOCK), 0, s, a);
        if (int e = launch_status()) return e;
    }
    return GLABC_OK;
}

}  // namespace glabc

using namespace glabc;

extern "C" {

__attribute__((visibility("default"))) int glabc_abc_draws(const glabc_model* model, uint64_t seed, int64_t row0, const int64_t* ids,
                                                           int64_t n, int64_t stride, float* theta_out, float* y_out, float* dis_out,
                                                           uint8_t* accept_out, void* stream)
{
    if (int e = check_abc_draws(model, row0, ids, n, stride, theta_out, y_out, dis_out, accept_out)) return e;
    if (n == 0) return GLABC_OK;
    hipStream_t s = (hipStream_t)stream;
    if (model->sim_kind == GLABC_SIM_GK)
        return launch_abc<4, 8>(model, seed, row0, ids, n, stride, theta_out, y_out, dis_out, accept_out, s);
    return dispatch_range<1, 8>(model->theta_dim, GLABC_ERR_DIM, [&](auto d) {
        constexpr int D = decltype(d)::value;
        return launch_abc<D, D>(model, seed, row0, ids, n, stride, theta_out, y_out, dis_out, accept_out, s);
    });
}

}  // extern "C"
