// glabc_wide_mix.hip -- the GaussianMixture variant of the lane-group GLMCMC kernel (glabc_wide.h, MX): its instantiations for
// the (theta_dim, y_dim) the library ships at L = 8 / 16 / 32 / 64 lanes per chain, and their host launcher.  Its own
// translation unit: the objects of the other variants do not change.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "glabc_dispatch.h"
#include "glabc_launch.h"
#include "glabc_lds_grant.h"
#include "glabc_mix.h"
#include "glabc_wide.h"

namespace glabc {

template <int D, int YD, int L>
static int launch_wide_mix_l(const MixStepArgs<D, YD>& a, int N, hipStream_t s)
{
    constexpr int GROUPS = WIDE_BLOCK / L;
    const size_t lds = (size_t)wide_lds_bytes(L, N);
    static LdsGrant grant;                               // per instantiation, per device
    if (!grant_dynamic_lds(grant, (const void*)wide_kernel<D, YD, L, false, true>, lds)) return GLABC_ERR_LAUNCH;
    const unsigned grid = grid_for(a.n_chains, GROUPS);
    hipLaunchKernelGGL((wide_kernel<D, YD, L, false, true>), dim3(grid), dim3(WIDE_BLOCK), lds, s, a, N);     // the block first: mix_of
    return launch_status();
}

template <int D, int YD>
int launch_wide_mix(const MixStepArgs<D, YD>& a, int N, int lanes, hipStream_t s)
{
    return dispatch_values<8, 16, 32, 64>(lanes, GLABC_ERR_ARG, [&](auto l) { return launch_wide_mix_l<D, YD, decltype(l)::value>(a, N, s); });
}

template int launch_wide_mix<1, 1>(const MixStepArgs<1, 1>&, int, int, hipStream_t);
template int launch_wide_mix<2, 2>(const MixStepArgs<2, 2>&, int, int, hipStream_t);
template int launch_wide_mix<3, 3>(const MixStepArgs<3, 3>&, int, int, hipStream_t);
template int launch_wide_mix<4, 4>(const MixStepArgs<4, 4>&, int, int, hipStream_t);
template int launch_wide_mix<4, 8>(const MixStepArgs<4, 8>&, int, int, hipStream_t);

}  // namespace glabc
