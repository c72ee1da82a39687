// glabc_mix.hip -- GaussianMixture (distribution.py:206-293; the specification is in include/glabc.h): the row-wise kernels
// glabc_mixture_log_prob / glabc_mixture_forward and the C entry points of the samplers' mixture variant, whose kernels live
// in glabc_mix_dim.hip (one lane per chain, default schedule) and glabc_wide_mix.hip (lane groups, batch sizes above
// GLABC_MAX_BATCH).  The entry point names the kernel: these entry points do not go through the launch plan.
#include <hip/hip_runtime.h>

#include <cstring>

#include "glabc_check.h"
#include "glabc_dispatch.h"
#include "glabc_launch.h"
#include "glabc_mix.h"
#include "glabc_pack.h"

namespace glabc {

template <int D>
struct MixRowArgs {
    MixArgs<D> g;
    const double* z;             // log_prob: [n][D] in
    double* z_out;               // forward: [n][D] out
    double* out;                 // [n]
    int64_t n, row0;
    uint32_t seed_lo, seed_hi;
};

// one row per lane, tail lanes masked
template <int D>
__global__ void __launch_bounds__(256) mixture_log_prob_kernel(const MixRowArgs<D> a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    double z[D];
#pragma unroll
    for (int q = 0; q < D; ++q) z[q] = a.z[i * D + q];
    a.out[i] = mix_log_prob<D>(a.g, z);
}

// row r reads Philox(seed; id lo, id hi, 0, b): the mode uniform from words 0-1 of block 0, the normals from words 2-3 of
// block 0, then blocks 1 and up (the layout of glabc_kde_sample)
template <int D>
__global__ void __launch_bounds__(256) mixture_forward_kernel(const MixRowArgs<D> a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t gid = (uint64_t)(a.row0 + i);
    constexpr int NB = (D + 2 + 3) / 4;
    float nrm[4 * NB], eps[D];
    double u = 0.0;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const glabc_u32x4 w = glabc_philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), 0u, (uint32_t)b, a.seed_lo, a.seed_hi);
        if (b == 0) {
            u = glabc_uniform_f64(w.v[0], w.v[1]);
            glabc_normal_pair(w.v[2], w.v[3], &nrm[0], &nrm[1]);
        } else {
            glabc_normal_pair(w.v[0], w.v[1], &nrm[4 * b - 2], &nrm[4 * b - 1]);
            glabc_normal_pair(w.v[2], w.v[3], &nrm[4 * b], &nrm[4 * b + 1]);
        }
    }
#pragma unroll
    for (int q = 0; q < D; ++q) eps[q] = nrm[q];
    double z[D];
    mix_draw<D>(a.g, u, eps, z);
#pragma unroll
    for (int q = 0; q < D; ++q) a.z_out[i * D + q] = z[q];
    a.out[i] = mix_log_prob<D>(a.g, z);
}

}  // namespace glabc

using namespace glabc;

static int run_mix_sampler(int algo, const glabc_model* m, const glabc_dist* local, const glabc_mixture* g, const glabc_chains* c,
                           const glabc_run* r, void* stream)
{
    if (int e = check_mix_run(m, local, g, c, r, algo == ALGO_GLMCMC)) return e;
    if (c->n_chains == 0 || r->n_steps == 0) return GLABC_OK;
    hipStream_t s = (hipStream_t)stream;
    if (m->sim_kind == GLABC_SIM_GK) return launch_mix_dim<4, 8>(algo, r->batch_size, pack_mix_args<4, 8>(m, local, g, c, r), s);
    return dispatch_range<1, 4>(m->theta_dim, GLABC_ERR_KIND, [&](auto d) {
        constexpr int D = decltype(d)::value;
        return launch_mix_dim<D, D>(algo, r->batch_size, pack_mix_args<D, D>(m, local, g, c, r), s);
    });
}

// batch sizes beyond the register kernels: lane groups of a wavefront share a chain's candidates (glabc_wide_mix.hip)
static int run_mix_wide(const glabc_model* m, const glabc_dist* local, const glabc_mixture* g, const glabc_chains* c, const glabc_run* r,
                        void* stream)
{
    if (int e = check_mix_wide_run(m, local, g, c, r)) return e;
    if (c->n_chains == 0 || r->n_steps == 0) return GLABC_OK;
    hipStream_t s = (hipStream_t)stream;
    const int N = r->batch_size, lanes = r->lanes_per_chain ? r->lanes_per_chain : wide_default_lanes(N);
    if (m->sim_kind == GLABC_SIM_GK) return launch_wide_mix<4, 8>(pack_mix_args<4, 8>(m, local, g, c, r), N, lanes, s);
    return dispatch_range<1, 4>(m->theta_dim, GLABC_ERR_KIND, [&](auto d) {
        constexpr int D = decltype(d)::value;
        return launch_wide_mix<D, D>(pack_mix_args<D, D>(m, local, g, c, r), N, lanes, s);
    });
}

template <bool FORWARD>
static int run_mix_rows(const glabc_mixture* g, const double* z, int64_t n, uint64_t seed, int64_t row0, double* z_out, double* out,
                        void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    return dispatch_range<1, GLABC_MAX_DIM>(g->dim, GLABC_ERR_DIM, [&](auto d) {
        constexpr int D = decltype(d)::value;
        MixRowArgs<D> a;
        std::memset(&a, 0, sizeof a);
        a.g = pack_mixture<D>(g);
        a.z = z; a.z_out = z_out; a.out = out;
        a.n = n; a.row0 = row0; a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32);
        if constexpr (FORWARD)
            hipLaunchKernelGGL((mixture_forward_kernel<D>), dim3(grid_for(n, 256)), dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL((mixture_log_prob_kernel<D>), dim3(grid_for(n, 256)), dim3(256), 0, s, a);
        return launch_status();
    });
}

extern "C" {

__attribute__((visibility("default"))) int glabc_mixture_log_prob(const glabc_mixture* dist, const double* z, int64_t n, double* out,
                                                                  void* stream)
{
    if (int e = check_mixture(dist, 0)) return e;
    if (!z || !out) return GLABC_ERR_NULL;
    if (n < 0) return GLABC_ERR_ARG;
    if (n == 0) return GLABC_OK;
    return run_mix_rows<false>(dist, z, n, 0, 0, nullptr, out, stream);
}

__attribute__((visibility("default"))) int glabc_mixture_forward(const glabc_mixture* dist, int64_t n, uint64_t seed, int64_t row0,
                                                                 double* z_out, double* log_p_out, void* stream)
{
    if (int e = check_mixture(dist, 0)) return e;
    if (!z_out || !log_p_out) return GLABC_ERR_NULL;
    if (n < 0 || row0 < 0) return GLABC_ERR_ARG;
    if (n == 0) return GLABC_OK;
    return run_mix_rows<true>(dist, nullptr, n, seed, row0, z_out, log_p_out, stream);
}

__attribute__((visibility("default"))) int glabc_init_weights_mix(const glabc_model* model, const glabc_mixture* importance,
                                                                  const glabc_chains* c, void* stream)
{
    if (int e = check_mix_model(model, importance)) return e;
    if (int e = check_chain_pointers(c, CHAINS_ISIR)) return e;
    if (c->n_chains < 0 || c->stride < c->n_chains) return GLABC_ERR_ARG;      // chain0 is not read
    if (c->n_chains == 0) return GLABC_OK;
    hipStream_t s = (hipStream_t)stream;
    if (model->sim_kind == GLABC_SIM_GK)
        return launch_init_weights_mix_dim<4, 8>(pack_mix_args<4, 8>(model, nullptr, importance, c, nullptr), s);
    return dispatch_range<1, 4>(model->theta_dim, GLABC_ERR_KIND, [&](auto d) {
        constexpr int D = decltype(d)::value;
        return launch_init_weights_mix_dim<D, D>(pack_mix_args<D, D>(model, nullptr, importance, c, nullptr), s);
    });
}

__attribute__((visibility("default"))) int glabc_glmcmc_mix_steps(const glabc_model* model, const glabc_dist* local,
                                                                  const glabc_mixture* importance, const glabc_chains* chains,
                                                                  const glabc_run* run, void* stream)
{
    return run_mix_sampler(ALGO_GLMCMC, model, local, importance, chains, run, stream);
}

__attribute__((visibility("default"))) int glabc_glmcmc_mix_wide_steps(const glabc_model* model, const glabc_dist* local,
                                                                       const glabc_mixture* importance, const glabc_chains* chains,
                                                                       const glabc_run* run, void* stream)
{
    return run_mix_wide(model, local, importance, chains, run, stream);
}

__attribute__((visibility("default"))) int glabc_globalmcmc_mix_steps(const glabc_model* model, const glabc_dist* local,
                                                                      const glabc_mixture* global, const glabc_chains* chains,
                                                                      const glabc_run* run, void* stream)
{
    return run_mix_sampler(ALGO_GLOBAL, model, local, global, chains, run, stream);
}

}  // extern "C"
