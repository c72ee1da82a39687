// glabc_geometry.h -- the integer rules of the fused samplers' launch geometry: how a team splits an iteration's candidates
// and what LDS it takes, the lane-group kernel's block, lanes and LDS, the lanes per chain of a small launch.  constexpr and
// free of HIP: the kernels (glabc_team.h, glabc_wide.h -- hiprtc sees this text too), their host launchers and the launch
// plan (glabc_plan.h) all read the one definition.
#pragma once

#include "../../include/glabc.h"

namespace glabc {

// ---- team of NW wavefronts per 64 chains (glabc_team.h) --------------------------------------------------------------------

// Split of an iteration's N candidates over the NW wavefronts of a team.  The main wavefront (candidate 0 included) also draws
// the step head and takes the decision, which cost it about 1.1 candidates (85 + 165 of 227 vector instructions); the helpers
// share the rest evenly.  N = 5: two wavefronts 2 | 3, three wavefronts 1 | 2 2, four 1 | 2 1 1.
constexpr int team_main_candidates(int n, int nw)
{
    const int t10 = (10 * n + 11) / nw - 11;               // ten times ((n + 1.1) / nw - 1.1)
    const int na = (t10 + 5) / 10;                         // rounded
    return na < 1 ? 1 : (na > n - (nw - 1) ? n - (nw - 1) : na);
}
// first candidate of helper h (h = 0 .. nw-2; h = nw-1 gives n)
constexpr int team_helper_first(int n, int nw, int h)
{
    const int na = team_main_candidates(n, nw), nh = n - na, per = nh / (nw - 1), extra = nh % (nw - 1);
    return na + h * per + (h < extra ? h : extra);
}
constexpr bool team_split_ok(int n, int nw) { return n >= nw && team_main_candidates(n, nw) >= 1; }

// LDS of one workgroup (two iterations of the helpers' candidates); a CU hosts 1024 / 256 = 4 workgroups of a 65 536-chain launch
constexpr int team_lds_bytes(int d, int yd, int n, int nw) { return 2 * (n - team_main_candidates(n, nw)) * (4 + d + yd) * 64 * 4; }
constexpr int TEAM_MAX_LDS = 40 * 1024;
constexpr bool team_config_ok(int d, int yd, int n, int nw)
{
    return n >= 2 && n <= GLABC_MAX_BATCH && team_split_ok(n, nw) && team_lds_bytes(d, yd, n, nw) <= TEAM_MAX_LDS;
}

// GlobalMCMC team (global_team_kernel): iterations per barrier, and the LDS of a workgroup -- two chunks of that many
// iterations' draws
constexpr int GLOBAL_TEAM_CHUNK = 8;
constexpr int global_team_lds_bytes(int d, int nd) { return 2 * GLOBAL_TEAM_CHUNK * (2 + d + 2 * ((nd + 1) / 2)) * 64 * 4; }

// ---- lane groups (glabc_wide.h, batch sizes beyond GLABC_MAX_BATCH) ---------------------------------------------------------

constexpr int WIDE_BLOCK = 256;
constexpr int WIDE_LANES[4] = {8, 16, 32, 64};             // the instantiated lanes per chain
// lanes per chain when the caller leaves them to the library: the smallest group that keeps a lane at no more than 8 candidates
// (the per-step head, total and index search are executed by every lane of the group, so small groups amortise them best)
constexpr int wide_default_lanes(int n) { return n <= 64 ? 8 : n <= 128 ? 16 : n <= 256 ? 32 : 64; }
// a group's LDS row, in floats: the weights w[0..N] and the 32 accumulator-lane sums of torch.sum
constexpr int wide_row_floats(int n) { return n + 1 + 32; }
// dynamic LDS of a wide_kernel<L> workgroup at batch size N: one row per group of L lanes
constexpr int64_t wide_lds_bytes(int l, int n) { return (int64_t)4 * (WIDE_BLOCK / l) * wide_row_floats(n); }

// ---- lanes per chain of sampler_kernel ---------------------------------------------------------------------------------------

// lanes per chain: a launch-geometry choice (results do not depend on it).  Measured on MI355X
// (profiles/): with the branch-free candidate code one wave per SIMD already interleaves its N
// independent candidates, and one work-item per chain is fastest at 65 536 chains for N = 5
// (6.3 ms / 2000 iterations vs 6.8 ms with 2 lanes, 9.2 ms with 4); the split only pays when a
// launch would otherwise leave SIMDs empty (fewer chains than lanes on the chip).
constexpr int pick_lanes(int requested, int n_batch, int64_t n_chains)
{
    int lanes = requested;
    if (lanes <= 0) {
        const int64_t chip_lanes = 64 * 1024;                // one wave on each of the 1024 SIMDs
        lanes = 1;
        while (lanes < 4 && n_chains * lanes < chip_lanes) lanes *= 2;
    }
    if (lanes >= 4 && n_batch >= 3) return 4;
    if (lanes >= 2 && n_batch >= 2) return 2;
    return 1;
}

}  // namespace glabc
