// glabc_wide.hip -- host launchers of the lane-group GLMCMC kernel (glabc_wide.h) and its instantiations for the built-in
// Models: one per (theta_dim, y_dim) the library ships, L = 8 / 16 / 32 / 64 lanes per chain, with and without the Gamma
// importance proposal / prior.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "glabc_dispatch.h"
#include "glabc_launch.h"
#include "glabc_lds_grant.h"
#include "glabc_wide.h"

namespace glabc {

template <int D, int YD, int L, bool GM>
static int launch_wide_lg(const StepArgs<D, YD>& a, int N, hipStream_t s)
{
    constexpr int GROUPS = WIDE_BLOCK / L;
    const size_t lds = (size_t)wide_lds_bytes(L, N);
    static LdsGrant grant;                               // per instantiation, per device
    if (!grant_dynamic_lds(grant, (const void*)wide_kernel<D, YD, L, GM>, lds)) return GLABC_ERR_LAUNCH;
    const unsigned grid = grid_for(a.n_chains, GROUPS);
    hipLaunchKernelGGL((wide_kernel<D, YD, L, GM>), dim3(grid), dim3(WIDE_BLOCK), lds, s, a, N);
    return launch_status();
}

template <int D, int YD, int L>
static int launch_wide_l(const StepArgs<D, YD>& a, int N, hipStream_t s)
{
    if (a.prior.kind == GLABC_DIST_GAMMA || a.global.kind == GLABC_DIST_GAMMA)        // Gamma importance proposal / prior
        return launch_wide_lg<D, YD, L, true>(a, N, s);
    return launch_wide_lg<D, YD, L, false>(a, N, s);
}

// lanes: one of WIDE_LANES, from the launch plan (glabc_plan.h: the caller's choice or wide_default_lanes)
template <int D, int YD>
int launch_wide(const StepArgs<D, YD>& a, int N, int lanes, hipStream_t s)
{
    return dispatch_values<8, 16, 32, 64>(lanes, GLABC_ERR_ARG, [&](auto l) { return launch_wide_l<D, YD, decltype(l)::value>(a, N, s); });
}

template int launch_wide<1, 1>(const StepArgs<1, 1>&, int, int, hipStream_t);
template int launch_wide<2, 2>(const StepArgs<2, 2>&, int, int, hipStream_t);
template int launch_wide<3, 3>(const StepArgs<3, 3>&, int, int, hipStream_t);
template int launch_wide<4, 4>(const StepArgs<4, 4>&, int, int, hipStream_t);
template int launch_wide<4, 8>(const StepArgs<4, 8>&, int, int, hipStream_t);

}  // namespace glabc
