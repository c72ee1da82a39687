// quant_modes.hip -- the counting kernel of csrc/glabc_quant.hip under each of its contention modes (COUNT_DIRECT, COUNT_RUNS),
// whatever mode the library launches: tools/quantile_bench.py --modes-lib times them per level on the same history
// and requires equal counts.  A shared library of its own around the library's source file:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-slp-vectorize -fPIC -shared tools/ubench/quant_modes.hip \
//         -o tools/ubench/libquant_modes.so
#include "../../gl-abc-mcmc_amd/csrc/glabc_quant.hip"

namespace glabc {
thread_local int g_last_hip_error = 0;          // glabc_launch.h: the library defines it in glabc_hip.hip
}

extern "C" __attribute__((visibility("default"))) int quant_modes_key_counts(int mode, const float* history, int64_t n_rows,
                                                                             int32_t theta_dim, int64_t n_chains, int64_t stride,
                                                                             int32_t level, int32_t n_prefixes, const uint32_t* prefixes,
                                                                             uint64_t* counts, void* stream)
{
    if (int e = check_key_counts(history, n_rows, theta_dim, n_chains, stride, level, n_prefixes, prefixes, counts)) return e;
    if (n_chains == 0) return GLABC_OK;
    hipStream_t s = (hipStream_t)stream;
    switch (mode) {
    case COUNT_DIRECT: return key_counts_as<COUNT_DIRECT>(history, n_rows, theta_dim, n_chains, stride, level, n_prefixes, prefixes, counts, s);
    case COUNT_RUNS: return key_counts_as<COUNT_RUNS>(history, n_rows, theta_dim, n_chains, stride, level, n_prefixes, prefixes, counts, s);
    }
    return GLABC_ERR_ARG;
}
