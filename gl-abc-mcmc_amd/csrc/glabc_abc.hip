// glabc_abc.hip -- plain rejection ABC: glabc_abc_draws of include/glabc.h, which holds the specification of a draw.
//
// The kernel, abc_draws_kernel<D, YD>, lives in glabc_abc.h (a run-time compiled draws program instantiates it too, glabc_rtc.hip);
// this file holds its nine built-in instantiations -- |theta| + noise at theta_dim 1 .. 8 and g-and-k -- and the entry point.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "glabc_abc.h"
#include "glabc_check.h"
#include "glabc_dispatch.h"
#include "glabc_draws_pack.h"

using namespace glabc;

extern "C" {

__attribute__((visibility("default"))) int glabc_abc_draws(const glabc_model* model, uint64_t seed, int64_t row0, const int64_t* ids,
                                                           int64_t n, int64_t stride, float* theta_out, float* y_out, float* dis_out,
                                                           uint8_t* accept_out, void* stream)
{
    if (int e = check_abc_draws(model, row0, ids, n, stride, theta_out, y_out, dis_out, accept_out)) return e;
    if (n == 0) return GLABC_OK;
    const DrawsCall c{model, nullptr, seed, row0, ids, n, stride, theta_out, y_out, dis_out, nullptr, accept_out};
    hipStream_t s = (hipStream_t)stream;
    if (model->sim_kind == GLABC_SIM_GK) return launch_builtin_draws(abc_draws_kernel<4, 8>, pack_abc_args<4, 8>(c), s);
    return dispatch_range<1, 8>(model->theta_dim, GLABC_ERR_DIM, [&](auto d) {
        constexpr int D = decltype(d)::value;
        return launch_builtin_draws(abc_draws_kernel<D, D>, pack_abc_args<D, D>(c), s);
    });
}

}  // extern "C"
