// glabc_draws_pack.h -- the argument blocks of abc_draws_kernel (glabc_abc.h) and smc_draws_kernel (glabc_smc.h) from the descriptors
// of include/glabc.h: what the launchers of the built-in kernels (glabc_abc.hip, glabc_smc.hip) and the launch of a run-time
// compiled draws program (glabc_rtc.hip) both fill, so the two cannot drift apart.  `first` stays 0: the launcher walks it over the
// launches of at most 2^30 draws.  Host only, never handed to hiprtc.
#pragma once

#include <cstdint>
#include <cstring>

#include "glabc_abc.h"
#include "glabc_pack.h"
#include "glabc_smc.h"

namespace glabc {

template <int D, int YD>
inline AbcArgs<D, YD> pack_abc_args(const glabc_model* m, uint64_t seed, int64_t row0, const int64_t* ids, int64_t n, int64_t stride,
                                    float* theta, float* y, float* dis, uint8_t* accept)
{
    glabc_chains none;
    std::memset(&none, 0, sizeof none);
    AbcArgs<D, YD> a;
    std::memset(&a, 0, sizeof a);
    a.s = pack_args_rinv<D, YD>(m, nullptr, &m->prior, &none, nullptr, 0.0f);
    a.ids = ids;
    a.row0 = row0, a.n = n, a.stride = stride;
    const uint64_t kn = seed ^ GLABC_ABC_NOISE_KEY, ka = seed ^ GLABC_ABC_ACCEPT_KEY;
    a.prior_lo = (uint32_t)seed, a.prior_hi = (uint32_t)(seed >> 32);
    a.noise_lo = (uint32_t)kn, a.noise_hi = (uint32_t)(kn >> 32);
    a.accept_lo = (uint32_t)ka, a.accept_hi = (uint32_t)(ka >> 32);
    a.theta = theta, a.y = y, a.dis = dis, a.accept = accept;
    return a;
}

template <int D, int YD>
inline SmcArgs<D, YD> pack_smc_args(const glabc_model* m, const glabc_kde* k, uint64_t seed, int64_t row0, const int64_t* ids, int64_t n,
                                    int64_t stride, float* theta, float* y, float* dis, float* log_prior, uint8_t* accept)
{
    glabc_chains none;
    std::memset(&none, 0, sizeof none);
    SmcArgs<D, YD> a;
    std::memset(&a, 0, sizeof a);
    a.s = pack_args_rinv<D, YD>(m, nullptr, &m->prior, &none, nullptr, 0.0f);
    a.x = k->x, a.cum_q = k->cum_q, a.S = k->n_samples;
    for (int d = 0; d < D; ++d) a.bw[d] = k->bandwidth[d];
    a.ids = ids;
    a.row0 = row0, a.n = n, a.stride = stride;
    const uint64_t kn = seed ^ GLABC_ABC_NOISE_KEY, ka = seed ^ GLABC_ABC_ACCEPT_KEY;
    a.prop_lo = (uint32_t)seed, a.prop_hi = (uint32_t)(seed >> 32);
    a.noise_lo = (uint32_t)kn, a.noise_hi = (uint32_t)(kn >> 32);
    a.accept_lo = (uint32_t)ka, a.accept_hi = (uint32_t)(ka >> 32);
    a.theta = theta, a.y = y, a.dis = dis, a.log_prior = log_prior, a.accept = accept;
    return a;
}

}  // namespace glabc
