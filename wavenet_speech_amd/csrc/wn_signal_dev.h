// What the event tables (wn_events.hip), the signal alignment (wn_sigalign.hip, section 7k) and the signal
// mapping (wn_sigmap.hip, section 7l) share: the quantisation of a sample, the index of a k-mer window, the cost of a sample in a
// state with the check of a model row, a read's scale pair, the sentinels of a path's cost, and their limits.  ONE definition each: the alignment makes the segmentation that the event
// tables consume, so both must quantise a sample to the same bits, and a mapping must cost what the alignment of its span costs.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace wn {

constexpr int kSigMaxK = 6;                   // k-mer length
constexpr int kSigMaxFirst = 8;               // |first|: the offset of a window against its event or state
constexpr int kSigMaxFrac = 20;               // frac_bits
constexpr int kSigQLimit = 1 << 23;           // |q| (and a model's |level|) stay below
constexpr int kSaOffsetLimit = 1 << 30;       // a model's |offset| stays below

// the sentinels of a path's cost; every user proves beside its own limits that its finite costs stay below kPathInf
constexpr long long kPathInf = 1ll << 62;     // no path reaches this state
constexpr long long kPathNone = 0x7fffffffffffffffll;                // a read's score: no alignment / no mapping (LLONG_MAX)
constexpr long long kPathBadRead = -0x7fffffffffffffffll - 1;        // a read's score: a bad read (LLONG_MIN)

// read b's (scale, shift) of scale_shift [B][2]; nullptr: samples are taken as they are
struct ReadScale {
    bool scaled;
    double scale, shift;
};
__device__ __forceinline__ ReadScale read_scale(const float* scale_shift, int b) {
    const bool scaled = scale_shift != nullptr;
    return {scaled, scaled ? (double)scale_shift[2 * b] : 1.0, scaled ? (double)scale_shift[2 * b + 1] : 0.0};
}

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

// min((d d weight) >> S, max_cost) + offset with d = |q - level| < 2^24: the 79-bit product in two 64-bit halves
__device__ __forceinline__ long long sa_sample_cost(int q, int level, int weight, int offset, int S, int max_cost) {
    const int df = q - level;
    const unsigned d = (unsigned)(df < 0 ? -df : df);
    const unsigned long long dd = (unsigned long long)d * d;         // < 2^48
    const unsigned long long w = (unsigned)weight;
    const unsigned long long p0 = (dd & 0xffffffffull) * w, p1 = (dd >> 32) * w;     // p1 < 2^47
    const unsigned long long lo = p0 + (p1 << 32);
    const unsigned long long hi = (p1 >> 32) + (lo < p0 ? 1ull : 0ull);              // < 2^15
    const unsigned long long sh = (lo >> S) | (hi << (64 - S));      // S in 16..63: the quotient is below 2^63
    const long long c = sh < (unsigned long long)max_cost ? (long long)sh : (long long)max_cost;
    return c + offset;
}

// the model row of a k-mer that the path can use; a row out of range clears *ok and is replaced by (0, 1, 0)
__device__ __forceinline__ void sa_model_row(const int* model, int code, int* level, int* weight, int* offset, bool* ok) {
    const int l = model[3 * code], w = model[3 * code + 1], o = model[3 * code + 2];
    const bool good = w >= 1 && l > -kSigQLimit && l < kSigQLimit && o > -kSaOffsetLimit && o < kSaOffsetLimit;
    if (!good) *ok = false;
    *level = good ? l : 0;
    *weight = good ? w : 1;
    *offset = good ? o : 0;
}

// host: a signal pointer is aligned to its element (signal_kind 0: float, 1: short)
inline bool signal_aligned(const void* signal, int signal_kind) { return ((size_t)signal & (signal_kind ? 1 : 3)) == 0; }

}  // namespace wn
