// Candidates for a cheaper exactly rounded square root on the domain of glabc_sqrtf_normal (include/glabc_numerics.h):
// +-0 and every float in [2^-64, FLT_MAX].  For each form: the number of inputs on which it differs from the exactly rounded
// (float)sqrt((double)x) (the sweep of tests/test_hip_numerics.py), and its issue cost at 3 wavefronts per SIMD.
//   form 0  glabc_sqrtf_normal: v_sqrt_f32 + compare-both-neighbours correction                     (10 instructions)
//   form 1  s = v_sqrt_f32(x); r = fma(-s, s, x); s + r * v_rcp_f32(2 s + 2^-80)                     (5, 2 transcendental)
//   form 2  y = v_rsq_f32(max(x, 2^-100)); s = x y; r = fma(-s, s, x); s + r * (y / 2)               (6, 1 transcendental)
//   form 3  form 2 with x clamped by v_med3_f32 and r by v_min_f32, which keeps +inf at +inf as forms 0 and 1 do    (7)
// Whether the one-step forms round correctly everywhere depends on the bits of the hardware estimates: only the sweep tells.
// DESIGN.md 4.1-r3 "Round 5" has the outcome (forms 2 and 3 round correctly and are cheaper here, but did not make the
// sampler kernel faster, so glabc_sqrtf_normal stays form 0).
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off sqrt_forms.hip -o sqrt_forms ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../include/glabc_numerics.h"

template <int FORM>
__device__ __forceinline__ float sqrt_form(float x)
{
    if constexpr (FORM == 0) {
        return glabc_sqrtf_normal(x);
    } else if constexpr (FORM == 1) {
        const float s = __builtin_amdgcn_sqrtf(x);
        const float r = __builtin_fmaf(-s, s, x);
        const float h = __builtin_amdgcn_rcpf(__builtin_fmaf(2.0f, s, 0x1p-80f));      // 2 s exactly for s >= 2^-32; finite at +-0
        return __builtin_fmaf(r, h, s);
    } else if constexpr (FORM == 2) {
        const float y = __builtin_amdgcn_rsqf(__builtin_fmaxf(x, 0x1p-100f));          // finite at +-0: x * y is then x itself
        const float s = x * y;
        const float r = __builtin_fmaf(-s, s, x);
        return __builtin_fmaf(r, 0.5f * y, s);
    } else {
        const float y = __builtin_amdgcn_rsqf(__builtin_amdgcn_fmed3f(x, 0x1p-100f, 0x1.fffffep+127f));
        const float s = x * y;
        const float r = __builtin_fminf(__builtin_fmaf(-s, s, x), 0x1.fffffep+127f);   // +inf: the residual is nan, the result stays +inf
        return __builtin_fmaf(r, 0.5f * y, s);
    }
}

// out[0] = mismatches, out[1] = lowest mismatching bit pattern + 1 (0: none)
template <int FORM>
__global__ void __launch_bounds__(256) sweep(uint32_t first, uint32_t last, unsigned long long* __restrict__ out)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    unsigned long long local = 0, low = ~0ull;
    for (uint64_t b = (uint64_t)first + (uint64_t)blockIdx.x * 256 + threadIdx.x; b <= (uint64_t)last; b += stride) {
        const float x = glabc_u2f((uint32_t)b);
        const float want = (float)__builtin_sqrt((double)x);
        if (glabc_f2u(sqrt_form<FORM>(x)) != glabc_f2u(want)) {
            ++local;
            low = b + 1 < low ? b + 1 : low;
        }
    }
    if (local) {
        atomicAdd(&out[0], local);
        atomicMin(&out[1], low);
    }
}

template <int FORM>
__global__ void __launch_bounds__(64) cost(unsigned long long* __restrict__ out, int iters, float seed)
{
    float a0 = seed + threadIdx.x, a1 = a0 + 0.37f, a2 = a0 * 1.7f, a3 = a0 + 11.0f;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            a0 = sqrt_form<FORM>(a0) + 3.0f;
            a1 = sqrt_form<FORM>(a1) + 3.0f;
            a2 = sqrt_form<FORM>(a2) + 3.0f;
            a3 = sqrt_form<FORM>(a3) + 3.0f;
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0) out[blockIdx.x * 2] = t1 - t0;
    if (a0 + a1 + a2 + a3 == 0.123f) out[blockIdx.x * 2 + 1] = 1;
}

template <int FORM>
int run(unsigned long long* d)
{
    const uint32_t ranges[3][2] = {{0x1f800000u, 0x7f7fffffu}, {0u, 0u}, {0x80000000u, 0x80000000u}};
    unsigned long long h[2] = {0ull, ~0ull};
    if (hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice) != hipSuccess) return 1;
    for (auto& r : ranges) hipLaunchKernelGGL((sweep<FORM>), dim3(4096), dim3(256), 0, 0, r[0], r[1], d);
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    if (hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    printf("form %d: %llu mismatches", FORM, h[0]);
    if (h[0]) printf(" (lowest input bits 0x%08llx)", h[1] - 1);
    const int iters = 200, blocks = 3072;                      // 64-thread blocks: 3 wavefronts per SIMD on 256 CUs x 4 SIMDs
    hipLaunchKernelGGL((cost<FORM>), dim3(blocks), dim3(64), 0, 0, d, iters, 2.5f);
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    std::vector<unsigned long long> t(2 * blocks);
    if (hipMemcpy(t.data(), d, sizeof(unsigned long long) * 2 * blocks, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    double sum = 0;
    for (int i = 0; i < blocks; ++i) sum += (double)t[2 * i];
    printf("; %.1f s_memtime ticks per square root (+ one v_add_f32) per wavefront, 3 wavefronts per SIMD\n",
           sum / blocks / (32.0 * iters));
    return 0;
}

int main()
{
    unsigned long long* d;
    if (hipMalloc(&d, sizeof(unsigned long long) * 2 * 3072) != hipSuccess) return 1;
    int rc = run<0>(d) || run<1>(d) || run<2>(d) || run<3>(d);
    (void)hipFree(d);
    return rc;
}
