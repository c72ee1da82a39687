// glabc_smc.hip -- ABC-SMC proposals: glabc_smc_draws of include/glabc.h, which holds the specification of a draw.
//
// The kernel, smc_draws_kernel<D, YD>, lives in glabc_smc.h (a run-time compiled draws program instantiates it too, glabc_rtc.hip);
// this file holds its nine built-in instantiations -- |theta| + noise at theta_dim 1 .. 8 and g-and-k -- and the entry point, and the
// same nine of smc_draws_kernel<D, YD, true>, its twin under a full-covariance perturbation kernel (glabc_smc_draws_full).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "glabc_check.h"
#include "glabc_dispatch.h"
#include "glabc_draws_pack.h"
#include "glabc_smc.h"

using namespace glabc;

extern "C" {

__attribute__((visibility("default"))) int glabc_smc_draws(const glabc_model* model, const glabc_kde* population, uint64_t seed,
                                                           int64_t row0, const int64_t* ids, int64_t n, int64_t stride, float* theta_out,
                                                           float* y_out, float* dis_out, float* log_prior_out, uint8_t* accept_out,
                                                           void* stream)
{
    if (int e = check_smc_draws(model, population, row0, ids, n, stride, theta_out, y_out, dis_out, log_prior_out, accept_out)) return e;
    if (n == 0) return GLABC_OK;
    const DrawsCall c{model, population, seed, row0, ids, n, stride, theta_out, y_out, dis_out, log_prior_out, accept_out};
    hipStream_t s = (hipStream_t)stream;
    if (model->sim_kind == GLABC_SIM_GK) return launch_builtin_draws(smc_draws_kernel<4, 8>, pack_smc_args<4, 8>(c), s);
    return dispatch_range<1, 8>(model->theta_dim, GLABC_ERR_DIM, [&](auto d) {
        constexpr int D = decltype(d)::value;
        return launch_builtin_draws(smc_draws_kernel<D, D>, pack_smc_args<D, D>(c), s);
    });
}

// ... and under a full-covariance perturbation kernel: smc_draws_kernel<D, YD, true>, the same text with theta = x_j + L nrm
__attribute__((visibility("default"))) int glabc_smc_draws_full(const glabc_model* model, const glabc_kde* population, const float* chol,
                                                                uint64_t seed, int64_t row0, const int64_t* ids, int64_t n, int64_t stride,
                                                                float* theta_out, float* y_out, float* dis_out, float* log_prior_out,
                                                                uint8_t* accept_out, void* stream)
{
    if (int e = check_smc_draws_full(model, population, chol, row0, ids, n, stride, theta_out, y_out, dis_out, log_prior_out, accept_out))
        return e;
    if (n == 0) return GLABC_OK;
    const DrawsCall c{model, population, seed, row0, ids, n, stride, theta_out, y_out, dis_out, log_prior_out, accept_out, chol};
    hipStream_t s = (hipStream_t)stream;
    if (model->sim_kind == GLABC_SIM_GK) return launch_builtin_draws(smc_draws_kernel<4, 8, true>, pack_smc_full_args<4, 8>(c), s);
    return dispatch_range<1, 8>(model->theta_dim, GLABC_ERR_DIM, [&](auto d) {
        constexpr int D = decltype(d)::value;
        return launch_builtin_draws(smc_draws_kernel<D, D, true>, pack_smc_full_args<D, D>(c), s);
    });
}

}  // extern "C"
