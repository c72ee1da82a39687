// glabc_coverage.hip -- coverage checks of an ABC posterior on pseudo-observed data: glabc_coverage_counts of include/glabc.h, which
// holds the specification of a pair and of the three integer sums.
//
// The kernel, coverage_kernel<D, YD>, lives in glabc_coverage.h; this file holds its nine built-in instantiations -- |theta| + noise
// at theta_dim 1 .. 8 and g-and-k, as glabc_abc.hip's -- and the entry point.  The Model block and the keys come from the packer of
// the draw kernels (glabc_draws_pack.h), so a table draw cannot drift from glabc_abc_draws'.
// profiles/coverage_kernel_resources.txt holds the compiler's resource report.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "glabc_check.h"
#include "glabc_coverage.h"
#include "glabc_dispatch.h"
#include "glabc_draws_pack.h"
#include "glabc_launch.h"

namespace glabc {

static_assert(COV_MAX_DRAWS == GLABC_MAX_COVERAGE_DRAWS && COV_MAX_TESTS == GLABC_MAX_COVERAGE_TESTS, "the limits of include/glabc.h");
// the grid rule (glabc_coverage.h): one chunk and one tile; the three widths of a tile; the workgroups of a full launch; the largest call
static_assert(coverage_geometry(1, 1).chunks_x == 1 && coverage_geometry(1, 1).tiles_y == 1 && coverage_geometry(1, 1).tw == 1, "");
static_assert(coverage_geometry(257, 64).chunks_x == 2 && coverage_geometry(257, 64).tw == 1 && coverage_geometry(1, 65).tw == 2 &&
                  coverage_geometry(1, 65).tiles_y == 1 && coverage_geometry(1, 129).tw == 4 && coverage_geometry(1, 257).tiles_y == 2, "");
static_assert(coverage_geometry(1 << 20, 1024).chunks_x == 512 && coverage_geometry(1 << 20, 1024).tiles_y == 4 &&
                  coverage_geometry(COV_MAX_DRAWS, COV_MAX_TESTS).chunks_x == 1 && coverage_geometry(COV_MAX_DRAWS, COV_MAX_TESTS).tiles_y == 4096, "");

struct CovCall {
    const glabc_model* m;
    uint64_t seed;
    int64_t row0, n;
    const float* theta_star;
    const float* y_star;
    const float* width;
    int64_t n_tests, test_stride;
    int32_t kernel;
    unsigned long long* mass;
    unsigned long long* mass2;
    unsigned long long* below;
};

template <int D, int YD>
inline int launch_coverage(const CovCall& c, hipStream_t s)
{
    CovArgs<D, YD> a;
    std::memset(&a, 0, sizeof a);
    // glabc_abc_draws' block for draws row0 .. row0 + n - 1 with no output: the Model, theta's key and the noise key
    const DrawsCall draws{c.m, nullptr, c.seed, c.row0, nullptr, c.n, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    pack_draw_common<D, YD>(draws, &a.s, &a.d);
    const CovGeometry g = coverage_geometry(c.n, c.n_tests);
    a.theta_star = c.theta_star, a.y_star = c.y_star, a.width = c.width;
    a.n_tests = c.n_tests, a.test_stride = c.test_stride;
    a.kernel = c.kernel, a.tw = g.tw;
    a.mass = c.mass, a.mass2 = c.mass2, a.below = c.below;
    hipLaunchKernelGGL((coverage_kernel<D, YD>), dim3(g.chunks_x, g.tiles_y), dim3(COV_BLOCK), 0, s, a);
    return launch_status();
}

}  // namespace glabc

using namespace glabc;

extern "C" {

__attribute__((visibility("default"))) int glabc_coverage_counts(const glabc_model* model, uint64_t seed, int64_t row0, int64_t n,
                                                                 const float* theta_star, const float* y_star, const float* width,
                                                                 int64_t n_tests, int64_t test_stride, int32_t kernel,
                                                                 unsigned long long* mass, unsigned long long* mass2,
                                                                 unsigned long long* below, void* stream)
{
    if (int e = check_coverage_counts(model, row0, n, theta_star, y_star, width, n_tests, test_stride, kernel, mass)) return e;
    if (n == 0 || n_tests == 0) return GLABC_OK;
    const CovCall c{model, seed, row0, n, theta_star, y_star, width, n_tests, test_stride, kernel, mass, mass2, below};
    hipStream_t s = (hipStream_t)stream;
    if (model->sim_kind == GLABC_SIM_GK) return launch_coverage<4, 8>(c, s);
    return dispatch_range<1, 8>(model->theta_dim, GLABC_ERR_DIM, [&](auto d) {
        constexpr int D = decltype(d)::value;
        return launch_coverage<D, D>(c, s);
    });
}

}  // extern "C"
