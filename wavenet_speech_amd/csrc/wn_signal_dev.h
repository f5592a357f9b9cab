// What the event tables (wn_events.hip) and the signal alignment (wn_sigalign.hip, section 7k) share: the
// quantisation of a sample, the index of a k-mer window and their limits.  ONE definition each: the alignment makes the
// segmentation that the event tables consume, so both must quantise a sample to the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace wn {

constexpr int kSigMaxK = 6;                   // k-mer length
constexpr int kSigMaxFirst = 8;               // |first|: the offset of a window against its event or state
constexpr int kSigMaxFrac = 20;               // frac_bits
constexpr int kSigQLimit = 1 << 23;           // |q| (and a model's |level|) stay below

// q = llrint(v 2^F), v = x scale + shift in double with one rounding; false for a non-finite v or |q| >= 2^23
template <typename T>
__device__ __forceinline__ bool quantise(T x, bool scaled, double scale, double shift, double two_f, int* q) {
    double v = (double)x;
    if (scaled) v = __fma_rn(v, scale, shift);
    const double r = rint(v * two_f);                                // ties to even; a power-of-two product is exact
    if (!(fabs(r) < (double)kSigQLimit)) return false;               // NaN and inf fail the comparison
    *q = (int)r;
    return true;
}

// the k-mer index of the window lab[0 .. k), first base most significant; a label outside 1..4 clears *ok and counts as 1
__device__ __forceinline__ int kmer_code(const int* lab, int k, bool* ok) {
    int idx = 0;
    for (int i = 0; i < k; ++i) {
        const int v = lab[i];
        if (v < 1 || v > 4) *ok = false;
        idx = idx * 4 + ((v - 1) & 3);
    }
    return idx;
}

// host: a signal pointer is aligned to its element (signal_kind 0: float, 1: short)
inline bool signal_aligned(const void* signal, int signal_kind) { return ((size_t)signal & (signal_kind ? 1 : 3)) == 0; }

}  // namespace wn
