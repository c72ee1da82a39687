// glabc_mala_mix_dim.hip -- instantiates the GaussianMixture variant of the GLMALA kernels (MX, glabc_mala.h) for ONE theta_dim
// (-DGLABC_DIM=d), batch sizes 1..GLABC_MAX_BATCH.  Its own translation units: the objects of glabc_mala_dim.hip do not change.
#include "glabc_dispatch.h"
#include "glabc_launch.h"
#include "glabc_mala.h"

#ifndef GLABC_DIM
#error "compile with -DGLABC_DIM=<theta_dim>"
#endif

namespace glabc {

// the geometry is launch_mala's (glabc_mala_dim.hip): theta_dim 2 below two wavefronts per SIMD runs as teams of two
template <int D, int N>
static int launch_mala_mix(const MalaMixArgs<D>& mm, hipStream_t s)
{
    const MalaArgs<D>& m = mm.m;
    const unsigned grid = grid_for(m.s.n_chains, 64);
    if constexpr (D == 2) {
        const int nw = m.lanes ? m.lanes : (grid < 2048u ? 2 : 1);
        if (nw == 2) {
            if (m.s.y_obs_away) hipLaunchKernelGGL((glmala_team_kernel<N, true, 2, true>), dim3(grid), dim3(128), 0, s, mm);
            else hipLaunchKernelGGL((glmala_team_kernel<N, false, 2, true>), dim3(grid), dim3(128), 0, s, mm);
            return launch_status();
        }
    }
    if (m.s.y_obs_away)
        hipLaunchKernelGGL((glmala_kernel<D, N, true, true>), dim3(grid), dim3(64), 0, s, mm);
    else
        hipLaunchKernelGGL((glmala_kernel<D, N, false, true>), dim3(grid), dim3(64), 0, s, mm);
    return launch_status();
}

template <>
int launch_glmala_mix_dim<GLABC_DIM>(int n_batch, const MalaMixArgs<GLABC_DIM>& m, hipStream_t s)
{
    constexpr int D = GLABC_DIM;
    return dispatch_range<1, GLABC_MAX_BATCH>(n_batch, GLABC_ERR_ARG, [&](auto n) { return launch_mala_mix<D, decltype(n)::value>(m, s); });
}

}  // namespace glabc
