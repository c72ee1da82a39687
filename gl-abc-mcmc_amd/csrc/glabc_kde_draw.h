// glabc_kde_draw.h -- one row of KernelDensity.sample drawn on the device (kernel_density.py:130-150), shared by glabc_kde_sample
// (glabc_kde.hip) and glabc_smc_draws (glabc_smc.hip), so that an ABC-SMC proposal is row `id` of glabc_kde_sample by construction;
// and the same row under a full-covariance kernel (FULL: glabc_kde_sample_full, glabc_smc_draws_full), which departs in the
// perturbation alone.
#pragma once

#include "glabc_device.h"

namespace glabc {

// kde_draw_row's last argument where there is no Cholesky factor to fetch
struct NoChol {};

// z[d], d < D: the Philox blocks (key; id_lo, id_hi, 0, b), b < ceil((D + 2) / 4).  Words 0-1 of block 0 give the float64 uniform u,
// the centre is the first j with cum_q[j] > (int64)(u * cum_q[S - 1]) (clamped to S - 1), the normals come from words 2-3 of block 0
// and then from blocks 1 onwards; z_d = x[d * S + j] + nrm_d * bw_d, two rounded operations.  `bw` may be a by-value argument array:
// it is indexed by unrolled counters only.  The search is log2(S) dependent loads of cum_q.
// FULL: z_d = x[d * S + j] + acc_d, acc_d = nrm_0 L[d][0], then acc_d = acc_d + nrm_e L[d][e] for e = 1 .. d ascending, every product
// and every sum a rounded float32 operation.  `chol()` is asked for L AFTER the search -- the lower factor packed row-major,
// L[d][e] = chol()[d (d + 1) / 2 + e], wave-uniform and indexed by unrolled counters only (glabc_smc.h says why after) --; `bw` is
// not read
template <int D, bool FULL = false, class Chol = NoChol>
GLABC_DEV void kde_draw_row(const float* x, const int64_t* cum_q, int64_t S, const float (&bw)[D], uint64_t id, uint32_t key_lo,
                            uint32_t key_hi, float (&z)[D], Chol chol = Chol())
{
    constexpr int NB = (D + 2 + 3) / 4;
    float nrm[4 * NB];
    double u = 0.0;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        glabc_u32x4 w = glabc_philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), 0u, (uint32_t)b, key_lo, key_hi);
        if (b == 0) {
            u = glabc_uniform_f64(w.v[0], w.v[1]);
            glabc_normal_pair(w.v[2], w.v[3], &nrm[0], &nrm[1]);
        } else {
            glabc_normal_pair(w.v[0], w.v[1], &nrm[4 * b - 2], &nrm[4 * b - 1]);
            glabc_normal_pair(w.v[2], w.v[3], &nrm[4 * b], &nrm[4 * b + 1]);
        }
    }
    const int64_t target = (int64_t)(u * (double)cum_q[S - 1]);
    int64_t lo = 0, hi = S - 1;                            // first j with cum_q[j] > target (clamped to S-1)
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cum_q[mid] > target) hi = mid; else lo = mid + 1;
    }
    if constexpr (FULL) {
        const float* l = chol();
#pragma unroll
        for (int d = 0; d < D; ++d) {
            float acc = nrm[0] * l[d * (d + 1) / 2];
#pragma unroll
            for (int e = 1; e <= d; ++e) acc = acc + nrm[e] * l[d * (d + 1) / 2 + e];
            z[d] = x[d * S + lo] + acc;
        }
    } else {
#pragma unroll
        for (int d = 0; d < D; ++d) z[d] = x[d * S + lo] + nrm[d] * bw[d];   // kernel_density.py:147-148
    }
}

}  // namespace glabc
