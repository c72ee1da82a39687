// glabc_forward.h -- the variates of one row of BaseDistribution.forward drawn on the device (distribution.py:165-173, 73-78), shared
// by glabc_dist_forward (glabc_hip.hip) and glabc_abc_draws (glabc_abc.hip), so that a rejection draw's theta is row `id` of
// glabc_dist_forward by construction.
#pragma once

#include "glabc_device.h"

namespace glabc {

// e[i], i < dim: the Philox blocks (key; id_lo, id_hi, 0, b), b < ceil(D / 4) -- DiagGaussian: Box-Muller pairs of words (2i, 2i + 1);
// Uniform: one float32 uniform per word (the kind is wave-uniform).  The caller forms z_j = p0_j + p2_j * e_j
template <int D>
GLABC_DEV void dist_forward_variates(const DistArgs<D>& g, uint64_t id, uint32_t key_lo, uint32_t key_hi, float (&e)[4 * ((D + 3) / 4)])
{
    const bool uni = g.kind == GLABC_DIST_UNIFORM;
#pragma unroll
    for (int b = 0; b < (D + 3) / 4; ++b) {
        const glabc_u32x4 w = glabc_philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), 0u, (uint32_t)b, key_lo, key_hi);
        if (uni) {
#pragma unroll
            for (int t = 0; t < 4; ++t) e[4 * b + t] = glabc_uniform_f32(w.v[t]);
        } else {
            glabc_normal_pair(w.v[0], w.v[1], &e[4 * b], &e[4 * b + 1]);
            glabc_normal_pair(w.v[2], w.v[3], &e[4 * b + 2], &e[4 * b + 3]);
        }
    }
}

}  // namespace glabc
