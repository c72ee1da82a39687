// glabc_coverage.h -- coverage_kernel<D, YD>: the kernel of the coverage check of an ABC posterior on pseudo-observed data, as
// glabc_coverage.hip instantiates it for the built-in simulators (glabc_coverage_counts).  include/glabc.h holds the specification of
// a pair (test r, table draw i) and of the three integer sums.  No host includes: the header can be handed to hiprtc as text.
//
// Tests live in lanes, draws are broadcast.  A workgroup of COV_WAVES wavefronts walks chunks of COV_BLOCK table draws.  Per chunk every
// lane makes one draw exactly as abc_draws_kernel makes it -- dist_forward_variates under the seed, draw_simulate of glabc_draw.h under
// the noise key -- and parks (y, theta) in LDS, one record of REC floats per draw, 16-byte aligned.  After the barrier a lane, which owns
// ONE test with theta*, y* and its width in at most 17 vector registers, walks the records: every lane of a wavefront reads the same
// record (ds_read_b128 of one address: a broadcast, no bank conflict), forms model_discrepancy_rows<YD>(y_i, y*_r) -- the function
// glabc_model_discrepancy inlines, which is what makes the bits agree with it --, the multiplicity and the sums in private registers.
// No ballot, no LDS atomic and no load from memory in the pair loop; one 64-bit global atomic per non-zero sum and lane at the end.
//
// Geometry (coverage_geometry): the grid is draw chunks (x, a workgroup strides over them) by tiles of tests (y).  A tile is 64 * tw
// tests, tw = 1, 2 or 4 wavefronts wide; the COV_WAVES / tw wavefronts that share a test split the chunk's draws between them, so a
// call with few tests still fills the workgroup.  Every sum is an integer: the result is the same bits for every geometry.
// Which sums are wanted and which kernel weighs a pair is wave-uniform: cov_pairs is instantiated per case and chosen on scalar
// branches.  The hard kernel counts in 32 bits (a workgroup meets fewer than 2^31 draws) and widens at the end; the Model's kernel
// adds multiplicities up to 2^16 and their squares up to 2^32 in 64 bits (v_mad_u64_u32).
// The hard kernel without the square root.  d = sqrtf(ss) with ss the row sum of squares, and the correctly rounded square root is
// monotone, so d <= width holds exactly for ss <= T, T the largest float whose square root is <= width.  A lane finds T once, from
// width * width by steps of one float up and down through the very sqrtf a pair would take, and checks it (cov_squared_threshold);
// the pair loop then compares sums of squares: about 20 vector instructions per pair fewer.  A wavefront in which any lane's check
// fails -- none can, by the argument -- and a build with a user's distance take the loop that forms d.
// The by-value argument arrays are indexed by unrolled loop counters only, so the block stays in scalar registers;
// profiles/coverage_kernel_resources.txt holds the compiler's resource report.
#pragma once

#include "glabc_device.h"
#include "glabc_draw.h"
#include "glabc_forward.h"

namespace glabc {

constexpr int COV_LANES = 64;
constexpr int COV_WAVES = 4;
constexpr int COV_BLOCK = COV_LANES * COV_WAVES;              // table draws per chunk, one per lane
constexpr int64_t COV_MAX_DRAWS = (int64_t)1 << 30;           // per call: the worst sum, 2^32 x 2^30, fits 64 bits
constexpr int64_t COV_MAX_TESTS = (int64_t)1 << 20;           // per call: the grid's y stays inside 16 bits
constexpr int COV_TARGET_BLOCKS = 2048;                       // workgroups of a full launch: 8 per CU

// floats of a draw's record in LDS: y, then theta, padded to whole 16-byte reads
constexpr int cov_record(int D, int YD) { return 4 * ((D + YD + 3) / 4); }

struct CovGeometry {
    unsigned chunks_x, tiles_y;   // the grid
    int tw;                       // wavefronts of a workgroup side by side over the tests: 1, 2 or 4
};

// n >= 1 draws, n_tests >= 1 tests
constexpr CovGeometry coverage_geometry(int64_t n, int64_t n_tests)
{
    const int tw = n_tests <= COV_LANES ? 1 : n_tests <= 2 * COV_LANES ? 2 : COV_WAVES;
    const int64_t tiles = (n_tests + COV_LANES * tw - 1) / (COV_LANES * tw);
    const int64_t chunks = (n + COV_BLOCK - 1) / COV_BLOCK;
    const int64_t want = tiles >= COV_TARGET_BLOCKS ? 1 : COV_TARGET_BLOCKS / tiles;
    return CovGeometry{(unsigned)(chunks < want ? chunks : want), (unsigned)tiles, tw};
}

template <int D, int YD>
struct CovArgs {
    StepArgs<D, YD> s;            // the Model as the samplers' kernels see it: prior, simulator (y_obs is not read)
    DrawArgs d;                   // the keys and the range of glabc_abc_draws; every output NULL, ids NULL
    const float* theta_star;      // [D][test_stride]
    const float* y_star;          // [YD][test_stride]
    const float* width;           // [n_tests]
    int64_t n_tests, test_stride;
    int32_t kernel;               // 0 hard, 1 the Model's
    int32_t tw;                   // coverage_geometry's
    unsigned long long* mass;
    unsigned long long* mass2;    // may be NULL
    unsigned long long* below;    // may be NULL: [n_tests][D]
};

// The multiplicity of a pair under the Model's kernel: draw_accept_probability's ratio K(d) / K(0) at the test's width, quantised to
// 2^-16.  Every operator one rounded float32 operation; a NaN anywhere gives 0
GLABC_DEV uint32_t cov_model_multiplicity(float d, float width)
{
    const float e = (d - 0.0f) / width;
    const float p = glabc_expf(-(0.5f * (e * e)));
    return p == p ? (uint32_t)__builtin_rintf(p * 65536.0f) : 0u;
}

// model_discrepancy_rows (glabc_device.h) before its square root: the same differences, squares and aten_rowsum, so that
// __builtin_sqrtf of this IS that function's value
template <int YD>
GLABC_DEV float cov_sum_squares(const float (&y)[YD], const float (&ys)[YD])
{
    float t[YD];
#pragma unroll
    for (int j = 0; j < YD; ++j) {
        float d = y[j] - ys[j];
        t[j] = d * d;
    }
    return aten_rowsum<YD>(t);
}

GLABC_DEV float cov_float_up(float t) { return __uint_as_float(__float_as_uint(t) + 1u); }          // t >= 0, not +inf
GLABC_DEV float cov_float_down(float t) { return __uint_as_float(__float_as_uint(t) - 1u); }        // t > 0

// The largest T with sqrtf(T) <= width, so that for every sum of squares ss >= 0 (ss <= T) == (sqrtf(ss) <= width); a NaN where no
// ss qualifies (a negative or NaN width: the comparison is then always false, as d <= width is).  *ok: T was verified -- sqrtf(T) <=
// width and not sqrtf(next float) <= width.  T lies within two floats of width * width ((width + ulp / 2)^2 is width^2 (1 + 2^-23) at
// most), so eight steps either way are ample; where width * width overflows the walk starts at +inf and steps down to FLT_MAX
GLABC_DEV float cov_squared_threshold(float width, bool* ok)
{
    *ok = true;
    if (!(width >= 0.0f)) return __builtin_nanf("");
    if (width == __builtin_inff()) return width;                      // every ss but a NaN, +inf included
    float t = width * width;
#pragma unroll 1
    for (int k = 0; k < 8 && !(__builtin_sqrtf(t) <= width); ++k) t = cov_float_down(t);          // sqrtf(0) = 0 <= width: t > 0 here
#pragma unroll 1
    for (int k = 0; k < 8 && t != __builtin_inff() && __builtin_sqrtf(cov_float_up(t)) <= width; ++k) t = cov_float_up(t);
    *ok = __builtin_sqrtf(t) <= width && t != __builtin_inff() && !(__builtin_sqrtf(cov_float_up(t)) <= width);
    return t;
}

// The sums of one lane's test over draws first, first + step, .. < n_live of the chunk in `rec`.  HARD: m is 0 or 1 and the sums are
// 32-bit counts (acc: mass, below_0 ..; mass2 is mass); else 64-bit sums (acc: mass, mass2, below_0 ..).  SQUARED (hard only):
// `width` is cov_squared_threshold's T and is compared with the sum of squares
template <int D, int YD, bool HARD, bool BELOW, bool MASS2, bool SQUARED = false>
GLABC_DEV void cov_pairs(const float* rec, int first, int step, int n_live, const float (&ys)[YD], const float (&ths)[D], float width,
                         uint32_t (&cnt)[D + 1], unsigned long long (&sum)[D + 2])
{
    constexpr int REC = cov_record(D, YD);
#pragma unroll 2
    for (int i = first; i < n_live; i += step) {
        const float4* p = reinterpret_cast<const float4*>(rec + i * REC);
        float v[REC];
#pragma unroll
        for (int q = 0; q < REC / 4; ++q) {
            if (BELOW || 4 * q < YD) {                                // a counting-only walk reads y alone
                const float4 t = p[q];
                v[4 * q] = t.x, v[4 * q + 1] = t.y, v[4 * q + 2] = t.z, v[4 * q + 3] = t.w;
            }
        }
        float y[YD];
#pragma unroll
        for (int j = 0; j < YD; ++j) y[j] = v[j];
        const float dis = SQUARED ? cov_sum_squares<YD>(y, ys) : model_discrepancy_rows<YD>(y, ys);
        if (HARD) {
            const bool in = dis <= width;                            // a NaN on either side: false
            cnt[0] += in ? 1u : 0u;
            if (BELOW) {
#pragma unroll
                for (int j = 0; j < D; ++j) cnt[1 + j] += (in && v[YD + j] < ths[j]) ? 1u : 0u;
            }
        } else {
            const uint32_t m = cov_model_multiplicity(dis, width);
            sum[0] += m;
            if (MASS2) sum[1] += (unsigned long long)m * m;
            if (BELOW) {
#pragma unroll
                for (int j = 0; j < D; ++j) sum[2 + j] += v[YD + j] < ths[j] ? m : 0u;
            }
        }
    }
}

template <int D, int YD>
__global__ void __launch_bounds__(COV_BLOCK) coverage_kernel(const CovArgs<D, YD> a)
{
    constexpr int REC = cov_record(D, YD);
    __shared__ __attribute__((aligned(16))) float rec[COV_BLOCK * REC];

    const int tid = threadIdx.x, lane = tid & (COV_LANES - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / COV_LANES);          // wave-uniform: the pair loop's bounds stay scalar
    const int tw = a.tw, part = wave / tw, parts = COV_WAVES / tw;
    const int64_t test = ((int64_t)blockIdx.y * tw + wave % tw) * COV_LANES + lane;
    const bool live = test < a.n_tests;

    // this lane's test.  A lane past the last test weighs every pair 0: its width is a NaN
    float ths[D], ys[YD], width = __builtin_nanf("");
#pragma unroll
    for (int j = 0; j < D; ++j) ths[j] = 0.0f;
#pragma unroll
    for (int j = 0; j < YD; ++j) ys[j] = 0.0f;
    if (live) {
#pragma unroll
        for (int j = 0; j < D; ++j) ths[j] = a.theta_star[(int64_t)j * a.test_stride + test];
#pragma unroll
        for (int j = 0; j < YD; ++j) ys[j] = a.y_star[(int64_t)j * a.test_stride + test];
        width = a.width[test];
    }

    uint32_t cnt[D + 1];
    unsigned long long sum[D + 2];
#pragma unroll
    for (int j = 0; j < D + 1; ++j) cnt[j] = 0u;
#pragma unroll
    for (int j = 0; j < D + 2; ++j) sum[j] = 0ull;

    const bool hard = a.kernel == 0, want_below = a.below != nullptr, want_mass2 = a.mass2 != nullptr;
    // the hard kernel's threshold on the sum of squares, where every lane of the wavefront verified its own
    bool squared = false;
    float thr2 = width;
#ifndef GLABC_USER_DISCREPANCY
    if (hard) {
        bool ok;
        thr2 = cov_squared_threshold(width, &ok);
        squared = __all(ok);
    }
#endif
    const int64_t n_chunks = (a.d.n + COV_BLOCK - 1) / COV_BLOCK;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {          // the same trips for the whole workgroup
        const int64_t r = c * COV_BLOCK + tid;
        if (r < a.d.n) {
            // the draw of abc_draws_kernel (glabc_abc.h): theta is row id of glabc_dist_forward(prior), y the shared tail's
            const uint64_t id = draw_id(a.d, r);
            float e[4 * ((D + 3) / 4)], theta[D], y[YD];
            dist_forward_variates<D>(a.s.prior, id, a.d.theta_lo, a.d.theta_hi, e);
#pragma unroll
            for (int j = 0; j < D; ++j) theta[j] = a.s.prior.p0[j] + a.s.prior.p2[j] * e[j];
            draw_simulate<D, YD>(a.s, a.d, r, id, theta, y);
#pragma unroll
            for (int j = 0; j < YD; ++j) rec[tid * REC + j] = y[j];
#pragma unroll
            for (int j = 0; j < D; ++j) rec[tid * REC + YD + j] = theta[j];
        }
        __syncthreads();
        const int64_t left = a.d.n - c * COV_BLOCK;
        const int n_live = left < COV_BLOCK ? (int)left : COV_BLOCK;
        if (hard && squared) {
            if (want_below) cov_pairs<D, YD, true, true, false, true>(rec, part, parts, n_live, ys, ths, thr2, cnt, sum);
            else cov_pairs<D, YD, true, false, false, true>(rec, part, parts, n_live, ys, ths, thr2, cnt, sum);
        } else if (hard) {
            if (want_below) cov_pairs<D, YD, true, true, false>(rec, part, parts, n_live, ys, ths, width, cnt, sum);
            else cov_pairs<D, YD, true, false, false>(rec, part, parts, n_live, ys, ths, width, cnt, sum);
        } else if (want_below) {
            if (want_mass2) cov_pairs<D, YD, false, true, true>(rec, part, parts, n_live, ys, ths, width, cnt, sum);
            else cov_pairs<D, YD, false, true, false>(rec, part, parts, n_live, ys, ths, width, cnt, sum);
        } else {
            if (want_mass2) cov_pairs<D, YD, false, false, true>(rec, part, parts, n_live, ys, ths, width, cnt, sum);
            else cov_pairs<D, YD, false, false, false>(rec, part, parts, n_live, ys, ths, width, cnt, sum);
        }
        __syncthreads();                                               // the records are free for the next chunk
    }

    if (hard) {                                                       // a hard pair's m is its square
        sum[0] = cnt[0], sum[1] = cnt[0];
#pragma unroll
        for (int j = 0; j < D; ++j) sum[2 + j] = cnt[1 + j];
    }
    if (!live) return;
    if (sum[0]) atomicAdd(&a.mass[test], sum[0]);
    if (want_mass2 && sum[1]) atomicAdd(&a.mass2[test], sum[1]);
    if (want_below) {
#pragma unroll
        for (int j = 0; j < D; ++j)
            if (sum[2 + j]) atomicAdd(&a.below[test * D + j], sum[2 + j]);
    }
}

}  // namespace glabc
