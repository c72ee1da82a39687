// glabc_team_dim.hip -- instantiates team_sampler_kernel (glabc_team.h) for ONE theta_dim (-DGLABC_DIM=d [-DGLABC_YDIM=yd]),
// batch sizes 2..GLABC_MAX_BATCH as far as a workgroup's two candidate buffers fit the LDS budget.
#include "glabc_dispatch.h"
#include "glabc_launch.h"
#include "glabc_pack.h"
#include "glabc_team.h"

#ifndef GLABC_DIM
#error "compile with -DGLABC_DIM=<theta_dim> [-DGLABC_YDIM=<y_dim>]"
#endif
#ifndef GLABC_YDIM
#define GLABC_YDIM GLABC_DIM
#endif

namespace glabc {

template <int D, int YD, int N, int NW, bool FAST>
static int launch_team(const StepArgs<D, YD>& a, int prio, hipStream_t s)
{
    if constexpr (team_config_ok(D, YD, N, NW) && (!FAST || YD == D)) {
        const unsigned grid = grid_for(a.n_chains, 64);
        if (a.prior.kind == GLABC_DIST_GAMMA || a.global.kind == GLABC_DIST_GAMMA) {
            // VAR_GAMMA (float64 draws and densities): teams of two and three wavefronts, exact arithmetic
            if constexpr (NW <= 3 && !FAST)
                hipLaunchKernelGGL((team_sampler_kernel<D, YD, N, VAR_GAMMA, NW, false>), dim3(grid), dim3(64 * NW), 0, s, a, prio);
            else
                return GLABC_ERR_ARG;
        } else if (gauss_unit_config<D, YD>(a))
            hipLaunchKernelGGL((team_sampler_kernel<D, YD, N, (YD == D ? VAR_GAUSS_UNIT : VAR_GENERIC), NW, FAST>), dim3(grid), dim3(64 * NW), 0, s, a, prio);
        else
            hipLaunchKernelGGL((team_sampler_kernel<D, YD, N, VAR_GENERIC, NW, FAST>), dim3(grid), dim3(64 * NW), 0, s, a, prio);
        return launch_status();
    } else {
        return GLABC_ERR_ARG;
    }
}

template <int D, int YD, int N>
static int launch_team_nw(int nw, const StepArgs<D, YD>& a, int prio, bool fast, hipStream_t s)
{
    if (fast)                                               // GLABC_MATH_FAST: teams of two or three wavefronts
        return dispatch_range<2, 3>(nw, GLABC_ERR_ARG, [&](auto w) { return launch_team<D, YD, N, decltype(w)::value, true>(a, prio, s); });
    return dispatch_range<2, 4>(nw, GLABC_ERR_ARG, [&](auto w) { return launch_team<D, YD, N, decltype(w)::value, false>(a, prio, s); });
}

template <>
int launch_team_dim<GLABC_DIM, GLABC_YDIM>(int n_batch, int nw, const StepArgs<GLABC_DIM, GLABC_YDIM>& a, int prio, bool fast, hipStream_t s)
{
    constexpr int D = GLABC_DIM, YD = GLABC_YDIM;
    return dispatch_range<2, 16>(n_batch, GLABC_ERR_ARG, [&](auto n) { return launch_team_nw<D, YD, decltype(n)::value>(nw, a, prio, fast, s); });
}

template <int NW>
static int launch_global_team(const StepArgs<GLABC_DIM, GLABC_YDIM>& a, int prio, hipStream_t s)
{
    constexpr int D = GLABC_DIM, YD = GLABC_YDIM;
    const unsigned grid = grid_for(a.n_chains, 64);
    if (YD == D && gauss_unit_config<D, YD>(a))
        hipLaunchKernelGGL((global_team_kernel<D, YD, (YD == D ? VAR_GAUSS_UNIT : VAR_GENERIC), NW>), dim3(grid), dim3(64 * NW), 0, s, a, prio);
    else
        hipLaunchKernelGGL((global_team_kernel<D, YD, VAR_GENERIC, NW>), dim3(grid), dim3(64 * NW), 0, s, a, prio);
    return launch_status();
}

template <>
int launch_global_team_dim<GLABC_DIM, GLABC_YDIM>(int nw, const StepArgs<GLABC_DIM, GLABC_YDIM>& a, int prio, hipStream_t s)
{
    if (a.prior.kind == GLABC_DIST_GAMMA || a.global.kind == GLABC_DIST_GAMMA) return GLABC_ERR_ARG;      // one lane per chain
    return nw == 3 ? launch_global_team<3>(a, prio, s) : launch_global_team<2>(a, prio, s);
}

}  // namespace glabc
