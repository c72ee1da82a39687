// glabc_draws_pack.h -- the host side of the draw kernels (abc_draws_kernel of glabc_abc.h, smc_draws_kernel of glabc_smc.h): the
// record of a call, the argument blocks from the descriptors of include/glabc.h and the loop over the launches.  The built-in entry
// points (glabc_abc.hip, glabc_smc.hip) and the launch of a run-time compiled draws program (glabc_rtc.hip) all go through this text, so
// they cannot drift apart; glabc_predictive.hip takes its Model block and its key from it.  Host only, never handed to hiprtc.
#pragma once

#include <cstdint>
#include <cstring>

#include "glabc_abc.h"
#include "glabc_launch.h"
#include "glabc_pack.h"
#include "glabc_smc.h"

namespace glabc {

// What glabc_abc_draws / glabc_smc_draws and their run-time compiled twins are called with
struct DrawsCall {
    const glabc_model* m;
    const glabc_kde* pop;                            // null: abc_draws_kernel
    uint64_t seed;
    int64_t row0;
    const int64_t* ids;
    int64_t n, stride;
    float* theta;
    float* y;
    float* dis;
    float* log_prior;                                // smc_draws_kernel only
    uint8_t* accept;
    const float* chol;                               // smc_draws_kernel<.., true> only: the packed lower factor, a HOST array; else null
};

// The Model block of a kernel that makes draws: no chains, no proposals, no run
template <int D, int YD>
inline StepArgs<D, YD> pack_draw_model(const glabc_model* m)
{
    glabc_chains none;
    std::memset(&none, 0, sizeof none);
    return pack_args_rinv<D, YD>(m, nullptr, &m->prior, &none, nullptr, 0.0f);
}

inline void split_key(uint64_t key, uint32_t* lo, uint32_t* hi) { *lo = (uint32_t)key, *hi = (uint32_t)(key >> 32); }

// What the two blocks have in common: the Model, the three keys -- theta's is the seed itself --, the range and the outputs.  `first`
// stays 0: launch_draws walks it
template <int D, int YD>
inline void pack_draw_common(const DrawsCall& c, StepArgs<D, YD>* s, DrawArgs* d)
{
    *s = pack_draw_model<D, YD>(c.m);
    d->ids = c.ids;
    d->row0 = c.row0, d->n = c.n, d->stride = c.stride;
    split_key(c.seed, &d->theta_lo, &d->theta_hi);
    split_key(c.seed ^ GLABC_ABC_NOISE_KEY, &d->noise_lo, &d->noise_hi);
    split_key(c.seed ^ GLABC_ABC_ACCEPT_KEY, &d->accept_lo, &d->accept_hi);
    d->theta = c.theta, d->y = c.y, d->dis = c.dis, d->accept = c.accept;
}

template <int D, int YD>
inline AbcArgs<D, YD> pack_abc_args(const DrawsCall& c)
{
    AbcArgs<D, YD> a;
    std::memset(&a, 0, sizeof a);
    pack_draw_common<D, YD>(c, &a.s, &a.d);
    return a;
}

// The population's part of SmcArgs / SmcFullArgs: the same fields under the same names
template <int D, int YD, class Args>
inline Args pack_smc_block(const DrawsCall& c)
{
    Args a;
    std::memset(&a, 0, sizeof a);
    pack_draw_common<D, YD>(c, &a.s, &a.d);
    a.x = c.pop->x, a.cum_q = c.pop->cum_q, a.S = c.pop->n_samples;
    for (int d = 0; d < D; ++d) a.bw[d] = c.pop->bandwidth[d];
    a.log_prior = c.log_prior;
    return a;
}

template <int D, int YD>
inline SmcArgs<D, YD> pack_smc_args(const DrawsCall& c)
{
    return pack_smc_block<D, YD, SmcArgs<D, YD>>(c);
}

template <int D, int YD>
inline SmcFullArgs<D, YD> pack_smc_full_args(const DrawsCall& c)
{
    SmcFullArgs<D, YD> a = pack_smc_block<D, YD, SmcFullArgs<D, YD>>(c);
    for (int i = 0; i < D * (D + 1) / 2; ++i) a.chol[i] = c.chol[i];
    return a;
}

// n draws in launches of at most DRAW_MAX_LAUNCH: launch(first, grid) starts the kernel on draws first .. and returns its status
template <class Launch>
inline int launch_draws(int64_t n, Launch&& launch)
{
    for (int64_t first = 0; first < n; first += DRAW_MAX_LAUNCH) {
        const int64_t part = n - first < DRAW_MAX_LAUNCH ? n - first : DRAW_MAX_LAUNCH;
        if (int e = launch(first, grid_for(part, DRAW_BLOCK))) return e;
    }
    return GLABC_OK;
}

// ... of a built-in kernel on its block
template <class Args>
inline int launch_builtin_draws(void (*kernel)(Args), Args a, hipStream_t s)
{
    return launch_draws(a.d.n, [&](int64_t first, unsigned grid) {
        a.d.first = first;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(DRAW_BLOCK), 0, s, a);
        return launch_status();
    });
}

}  // namespace glabc
