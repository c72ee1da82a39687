// glabc_slots.h -- the slot functions of the counting kernels: which counter of a table a value (KeySlots, HistSlots) or a pair of
// values (JointSlots) adds to, or none.  glabc_quant.hip and glabc_joint.hip count one per draw of a chain-major history with them,
// glabc_weighted.hip a draw's quantised weight: one text, so the key, the levels, the prefix rules, the bin arithmetic
// (glabc_history.h) and the slot layouts of the weighted entry points are those of their unweighted twins.  The slot structures
// travel as kernel arguments; the functions that fill them run on the host.  The quantised weight of include/glabc.h comes with
// glabc_weighted_walk.h, host and device, which a run-time compiled program is given too.
#pragma once

#include <cstdint>

#include "glabc_check.h"
#include "glabc_history.h"
#include "glabc_weighted_walk.h"

namespace glabc {

// ---- glabc_key_counts: value -> index of its counter in the coordinate's table, or -1 ------------------------------------------
// NP: 0 at level 0, where every value belongs and nothing is compared; otherwise the prefixes compared per value -- n_prefixes
// rounded up to 1, 2, 4 or 8, the slots past n_prefixes unused.  Two vector instructions per prefix and value: the kernel is bound
// by its vector instructions before it is bound by HBM, so a launch pays for the prefixes it has
template <int NP>
struct KeySlots {
    uint32_t prefix[GLABC_MAX_DIM][NP ? NP : 1];
    int32_t n_prefixes, prefix_shift, digit_shift, digit_bits;   // prefix_shift: 32 - prefix_bits

    __device__ int n_slots() const { return n_prefixes << digit_bits; }
    // the coordinate's prefixes, from the kernel arguments into scalar registers
    struct Local {
        uint32_t p[NP ? NP : 1];
        int32_t prefix_shift, digit_shift, digit_bits;
        __device__ int operator()(float x) const
        {
            const uint32_t k = float_key(x);
            const int digit = (int)((k >> digit_shift) & ((1u << digit_bits) - 1u));
            if (NP == 0) return digit;
            const uint32_t mine = k >> prefix_shift;
            int slot = -1;
#pragma unroll
            for (int s = 0; s < NP; ++s) slot = mine == p[s] ? s : slot;          // an unused slot matches no prefix
            return slot < 0 ? -1 : (slot << digit_bits) | digit;
        }
    };
    __device__ Local local(int j) const
    {
        Local l;
#pragma unroll
        for (int s = 0; s < (NP ? NP : 1); ++s) l.p[s] = prefix[j][s];
        l.prefix_shift = prefix_shift, l.digit_shift = digit_shift, l.digit_bits = digit_bits;
        return l;
    }
};

template <int NP>
inline KeySlots<NP> key_slots(int32_t theta_dim, int32_t level, int32_t n_prefixes, const uint32_t* prefixes)
{
    KeySlots<NP> k;
    for (int j = 0; j < GLABC_MAX_DIM; ++j)
        for (int s = 0; s < (NP ? NP : 1); ++s)
            k.prefix[j][s] = NP && j < theta_dim && s < n_prefixes ? prefixes[j * n_prefixes + s] : KEY_UNUSED_SLOT;
    k.n_prefixes = n_prefixes;
    k.prefix_shift = 32 - key_prefix_bits(level);               // level 0 (NP == 0) never shifts by it
    k.digit_bits = key_digit_bits(level);
    k.digit_shift = 32 - key_prefix_bits(level) - k.digit_bits;
    return k;
}

// ---- glabc_histogram: the n_bins + 3 slots of hist_slot ---------------------------------------------------------------------------
struct HistSlots {
    double lo[GLABC_MAX_DIM], hi[GLABC_MAX_DIM], scale[GLABC_MAX_DIM];
    int32_t n_bins;

    __device__ int n_slots() const { return n_bins + 3; }
    struct Local {
        BinAxis axis;
        int32_t n_bins;
        __device__ int operator()(float x) const { return hist_slot(x, axis, n_bins); }
    };
    __device__ Local local(int j) const { return Local{{lo[j], hi[j], scale[j]}, n_bins}; }
};

inline HistSlots hist_slots(int32_t theta_dim, int32_t n_bins, const double* lo, const double* hi)
{
    HistSlots h;
    for (int j = 0; j < GLABC_MAX_DIM; ++j) {
        const BinAxis a = j < theta_dim ? bin_axis(lo[j], hi[j], n_bins) : bin_axis(0.0, 1.0, n_bins);
        h.lo[j] = a.lo, h.hi[j] = a.hi, h.scale[j] = a.scale;
    }
    h.n_bins = n_bins;
    return h;
}

// ---- glabc_histogram2d: the n_bins^2 + 2 slots of a pair --------------------------------------------------------------------------
constexpr int AXIS_OUTSIDE = -1, AXIS_NAN = -2;

struct JointSlots {
    double lo[GLABC_MAX_DIM], hi[GLABC_MAX_DIM], scale[GLABC_MAX_DIM];
    int32_t n_bins;
    uint8_t a[GLABC_MAX_PAIRS], b[GLABC_MAX_PAIRS];
};

// the bin of a value on an axis, glabc_histogram's rule; AXIS_OUTSIDE below lo or above hi, AXIS_NAN
__device__ __forceinline__ int axis_bin(float xf, const BinAxis& a, int n_bins)
{
    const double x = (double)xf;
    if (x != x) return AXIS_NAN;
    if (x < a.lo || x > a.hi) return AXIS_OUTSIDE;
    return bin_inside(x, a, n_bins);
}

// a NaN on either axis before a value outside on either axis before the cell
__device__ __forceinline__ int joint_slot(int bin_a, int bin_b, int n_bins)
{
    const int least = bin_a < bin_b ? bin_a : bin_b;
    const int cells = n_bins * n_bins;
    return least >= 0 ? bin_a * n_bins + bin_b : least == AXIS_NAN ? cells + 1 : cells;
}

inline JointSlots joint_slots(int32_t n_pairs, const int32_t* pairs, int32_t n_bins, const double* lo, const double* hi)
{
    JointSlots j;
    for (int q = 0; q < GLABC_MAX_DIM; ++q) j.lo[q] = 0.0, j.hi[q] = 1.0, j.scale[q] = 1.0;          // a coordinate no pair uses
    for (int p = 0; p < GLABC_MAX_PAIRS; ++p) {
        j.a[p] = (uint8_t)(p < n_pairs ? pairs[2 * p] : 0);
        j.b[p] = (uint8_t)(p < n_pairs ? pairs[2 * p + 1] : 0);
    }
    for (int q = 0; q < 2 * n_pairs; ++q) {
        const int c = pairs[q];
        const BinAxis a = bin_axis(lo[c], hi[c], n_bins);
        j.lo[c] = a.lo, j.hi[c] = a.hi, j.scale[c] = a.scale;
    }
    j.n_bins = n_bins;
    return j;
}

}  // namespace glabc
