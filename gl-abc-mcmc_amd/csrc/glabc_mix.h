// glabc_mix.h -- host side of the GaussianMixture variant (VAR_MIX, glabc_device.h): the per-dimension launchers of
// glabc_mix_dim.hip and the packing of a glabc_mixture into the kernels' argument block.  Never handed to hiprtc.
#pragma once

#include <cstring>

#include "glabc_pack.h"
#include "glabc_sampler.h"

namespace glabc {

// the mixture's tables compacted to the D coordinates in use
template <int D>
inline MixArgs<D> pack_mixture(const glabc_mixture* g)
{
    MixArgs<D> o;
    std::memset(&o, 0, sizeof o);
    o.n_modes = g->n_modes;
    o.c0 = g->c0;
    for (int k = 0; k < GLABC_MAX_MODES; ++k) {
        o.log_weight[k] = g->log_weight[k];
        o.cum_weight[k] = g->cum_weight[k];
        o.sum_log_scale[k] = g->sum_log_scale[k];
        for (int q = 0; q < D; ++q) {
            o.loc[k][q] = g->loc[k][q];
            o.scale[k][q] = g->scale[k][q];
            o.inv_scale[k][q] = g->inv_scale[k][q];
        }
    }
    return o;
}

// a DiagGaussian placeholder in StepArgs.global: the mixture variant never reads it (its kind only says that a global
// candidate's proposal draws are normals)
inline glabc_dist placeholder_global(int dim)
{
    glabc_dist g;
    std::memset(&g, 0, sizeof g);
    g.kind = GLABC_DIST_DIAG_GAUSS;
    g.dim = dim;
    for (int j = 0; j < GLABC_MAX_DIM; ++j) g.p2[j] = 1.0f;
    return g;
}

// the argument block of the mixture kernels, built-in (glabc_mix.hip) and run-time compiled (glabc_rtc.hip): one packer
template <int D, int YD>
inline MixStepArgs<D, YD> pack_mix_args(const glabc_model* m, const glabc_dist* local, const glabc_mixture* g, const glabc_chains* c,
                                        const glabc_run* r)
{
    const glabc_dist ph = placeholder_global(m->theta_dim);
    MixStepArgs<D, YD> a;
    std::memset(&a, 0, sizeof a);
    static_cast<StepArgs<D, YD>&>(a) = pack_args_rinv<D, YD>(m, local, &ph, c, r, 0.0f);
    a.mix = pack_mixture<D>(g);
    return a;
}

// GLMCMC (n_batch 1..GLABC_MAX_BATCH) or GlobalMCMC at one lane per chain, default schedule; defined in glabc_mix_dim.hip
// (one TU per theta_dim and for the g-and-k shape).  Returns a glabc_status.
template <int D, int YD>
int launch_mix_dim(int algo, int n_batch, const MixStepArgs<D, YD>& a, hipStream_t stream);

// GLMCMC at n_batch GLABC_MAX_BATCH + 1..GLABC_MAX_BATCH_WIDE: the lane-group kernel's mixture variant (glabc_wide.h) at
// lanes = 8 / 16 / 32 / 64 lanes per chain; defined in glabc_wide_mix.hip.  GLABC_ERR_LAUNCH where the device cannot give a
// workgroup its LDS rows (nothing is launched).
template <int D, int YD>
int launch_wide_mix(const MixStepArgs<D, YD>& a, int n_batch, int lanes, hipStream_t stream);

// GLMCMC.py:52-55 with the mixture as the importance proposal
template <int D, int YD>
int launch_init_weights_mix_dim(const MixStepArgs<D, YD>& a, hipStream_t stream);

}  // namespace glabc
