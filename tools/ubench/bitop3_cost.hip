// Microbenchmark: issue cost of v_bitop3_b32 (three-input bitwise op, here a ^ b ^ c) against v_xor_b32, four independent
// chains per wave, at 1 and 3 waves per SIMD -- the question behind the Philox rounds of include/glabc_numerics.h: is one
// v_bitop3_b32 cheaper than the two v_xor_b32 it replaces?
// Build: hipcc --offload-arch=gfx950 -O2 bitop3_cost.hip -o bitop3_cost ; run on the GPU box.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

#define REP4(x) x x x x
#define REP16(x) REP4(x) REP4(x) REP4(x) REP4(x)

template <int OP>
__global__ void k(unsigned long long* out, int iters, unsigned seed)
{
    unsigned a0 = threadIdx.x * 2654435761u + seed, a1 = a0 ^ 0x9e3779b9u, a2 = a0 + 77u, a3 = a0 * 3u;
    const unsigned b = a0 * 7u + 1u;
    unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int it = 0; it < iters; ++it) {
        if constexpr (OP == 0) {   // v_xor_b32 with one SGPR operand, as in the Philox rounds (the key word)
            REP16(asm volatile("v_xor_b32 %0, %5, %0\n v_xor_b32 %1, %5, %1\n v_xor_b32 %2, %5, %2\n v_xor_b32 %3, %5, %3"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b), "s"(seed));)
        } else {                   // v_bitop3_b32 a ^ b ^ s (0x96), one SGPR operand
            REP16(asm volatile("v_bitop3_b32 %0, %0, %4, %5 bitop3:0x96\n v_bitop3_b32 %1, %1, %4, %5 bitop3:0x96\n"
                               " v_bitop3_b32 %2, %2, %4, %5 bitop3:0x96\n v_bitop3_b32 %3, %3, %4, %5 bitop3:0x96"
                               : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3) : "v"(b), "s"(seed));)
        }
    }
    unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (threadIdx.x == 0) out[blockIdx.x * 2] = t1 - t0;
    if ((a0 ^ a1 ^ a2 ^ a3) == 0x12345678u) out[blockIdx.x * 2 + 1] = a0;
}

template <int OP>
void run(const char* name, unsigned long long* d_out)
{
    const int iters = 400;
    const double n_inst = 64.0 * iters;
    printf("%-14s:", name);
    for (int wps : {1, 3}) {
        const int blocks = 1024 * wps;         // 64-thread blocks: wps waves per SIMD on 256 CUs x 4 SIMDs
        hipLaunchKernelGGL((k<OP>), dim3(blocks), dim3(64), 0, 0, d_out, iters, 12345u);
        (void)hipDeviceSynchronize();
        std::vector<unsigned long long> h(blocks * 2);
        (void)hipMemcpy(h.data(), d_out, sizeof(unsigned long long) * blocks * 2, hipMemcpyDeviceToHost);
        double sum = 0;
        for (int i = 0; i < blocks; ++i) sum += (double)h[2 * i];
        const double cyc = sum / blocks / n_inst;
        printf("  %d wave(s)/SIMD: %6.2f ticks per wave-instruction, %6.2f per SIMD-instruction", wps, cyc, cyc / wps);
    }
    printf("\n");
}

int main()
{
    unsigned long long* d_out;
    if (hipMalloc(&d_out, sizeof(unsigned long long) * 2 * 1024 * 3) != hipSuccess) return 1;
    printf("s_memtime ticks per wave-instruction (four independent chains per wave)\n");
    run<0>("v_xor_b32", d_out);
    run<1>("v_bitop3_b32", d_out);
    (void)hipFree(d_out);
    return 0;
}
