// glabc_mix_dim.hip -- instantiates the GaussianMixture variant of sampler_kernel (VAR_MIX) for ONE theta_dim
// (-DGLABC_DIM=d [-DGLABC_YDIM=yd]): GLMCMC for batch sizes 1..GLABC_MAX_BATCH and GlobalMCMC, one lane per chain, and the
// init-weights kernel.  Its own translation units: the objects of the other variants do not change.
#include "glabc_dispatch.h"
#include "glabc_launch.h"
#include "glabc_mix.h"

#ifndef GLABC_DIM
#error "compile with -DGLABC_DIM=<theta_dim> [-DGLABC_YDIM=<y_dim>]"
#endif
#ifndef GLABC_YDIM
#define GLABC_YDIM GLABC_DIM
#endif

namespace glabc {

template <int D, int YD>
__global__ void __launch_bounds__(BLOCK) init_weights_mix_kernel(const MixStepArgs<D, YD> a)
{
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= a.n_chains) return;
    Chain<D, YD> c;
#pragma unroll
    for (int j = 0; j < D; ++j) c.theta[j] = a.theta[j * a.stride + i];
#pragma unroll
    for (int j = 0; j < YD; ++j) c.y[j] = a.y[j * a.stride + i];
    c.prior = model_prior<D, YD, false, false>(a, c.theta);
    c.kern = model_log_kernel<D, YD>(a, c.y);
    c.q = dist_mix_log_prob<D>(mix_of<D, YD>(a), c.theta);
    a.log_w[i] = (c.prior + c.kern) - c.q;                         // GLMCMC.py:52-55
    a.flags[i] = a.flags[i] | GLABC_FLAG_LOCAL;                    // GLMCMC.py:50
}

template <int ALGO, int D, int YD, int N>
static int launch_one(const MixStepArgs<D, YD>& a, hipStream_t s)
{
    hipLaunchKernelGGL((sampler_kernel<ALGO, D, YD, N, 1, VAR_MIX, SCHED_DEFAULT>), dim3(grid_for(a.n_chains, BLOCK)), dim3(BLOCK), 0, s, a);
    return launch_status();
}

template <>
int launch_mix_dim<GLABC_DIM, GLABC_YDIM>(int algo, int n_batch, const MixStepArgs<GLABC_DIM, GLABC_YDIM>& a, hipStream_t s)
{
    constexpr int D = GLABC_DIM, YD = GLABC_YDIM;
    if (algo == ALGO_GLOBAL) return launch_one<ALGO_GLOBAL, D, YD, 1>(a, s);
    return dispatch_range<1, GLABC_MAX_BATCH>(n_batch, GLABC_ERR_ARG, [&](auto n) { return launch_one<ALGO_GLMCMC, D, YD, decltype(n)::value>(a, s); });
}

template <>
int launch_init_weights_mix_dim<GLABC_DIM, GLABC_YDIM>(const MixStepArgs<GLABC_DIM, GLABC_YDIM>& a, hipStream_t s)
{
    hipLaunchKernelGGL((init_weights_mix_kernel<GLABC_DIM, GLABC_YDIM>), dim3(grid_for(a.n_chains, BLOCK)), dim3(BLOCK), 0, s, a);
    return launch_status();
}

}  // namespace glabc
