// Exact per-read order statistics of ragged reads (wavenet_speech_amd/normalise.py): the median, the MAD and quantiles that
// turn raw DAC counts into the (scale, shift) of wn_chunk_gather.  For every read b and every k < K the value of the
// ranks[b][k]-th smallest (0-based) of the read's first signal_lengths[b] samples -- a selection, not a sort: a most-significant-
// digit radix select over an order-preserving unsigned key, 8 bits per pass, integer histograms only (exact, and bitwise
// reproducible: integer sums do not depend on the order of the atomics).
//
//   key      int16            (uint16)x ^ 0x8000                                       16 bits, 2 passes
//            fp32             u = bits(x); u ^ (u >> 31 ? 0xFFFFFFFF : 0x80000000)     32 bits, 4 passes: -0.0 directly below +0.0,
//                             a positive-sign NaN above +inf and a negative-sign NaN below -inf, as their bit patterns order them
//            with center      d = fabsf(__fsub_rn((float)x, center[b])), bits(d)       32 bits, 4 passes, either dtype
//   select_pass_kernel   one launch per digit, grid (ceil(ld / kSelTile), B), 256 threads.  Prologue: every workgroup recomputes
//                        from the global histograms of the earlier passes the prefix (the digits chosen so far) and the remaining
//                        rank of each of the K ranks (wave w owns ranks w and w + 4; a 256-bin scan is one 16-byte load per lane
//                        and a wave prefix sum), so no workgroup waits for another and nothing but the histograms is shared.
//                        Ranks whose prefixes are equal share one histogram (all K do in the first pass; the two middle ranks of
//                        a median nearly always do).  Body: the workgroup streams its tile [x kSelTile, (x + 1) kSelTile) of the
//                        read once (16-byte loads from the first 16-byte boundary on, the misaligned head and the tail per
//                        element; nothing at or past the length is read) and counts in LDS the digit of every element whose
//                        higher digits equal a live prefix.  Lanes of a wave that hit the same bin are added as one atomic of
//                        their number (sel_wave_add).  Epilogue: non-zero LDS bins go to the read's global histogram with
//                        vector integer atomics.
//   select_final_kernel  grid (B), 256 threads: the same chain over all passes gives the whole key; the inverse of the key
//                        transform is the element itself (x or d) as fp32.  A read with len < 0 or len > ld and a rank outside
//                        [0, len) write 0.0f and count in *bad, once per (b, k): only this kernel counts.
//
// workspace: per read 1 + (passes - 1) K histograms of 256 uint32 (pass 0 has one, every later pass one per rank), zeroed on
// the stream by wn_read_select itself.  The number of launches depends on the dtype and on center only; nothing is read back.
// No length or rank is used before it is checked.  No scratch, no loop with a data-dependent trip count beyond the tile.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"
#include "wn_wave_dev.h"

namespace wn {

constexpr int kSelThreads = 256;
constexpr int kSelWaves = kSelThreads / 64;
constexpr int kSelTile = 8192;                   // samples of one workgroup; a multiple of 8: tiles keep the row's 16-byte phase
constexpr int kSelBins = 256;                    // 8 bits per pass
constexpr int kSelMaxK = 8;
constexpr int kSelMaxDim = 2147482624;           // 2^31 - 1024, as wn_chunk
constexpr long long kSelMaxGridThreads = 4294967296ll;
constexpr int kSelAggRounds = 4;                 // sel_wave_add: groups of equal bins served before the rest adds lane by lane
constexpr int kSelAggMin = 8;                    // ... and the group size below which grouping stops paying

__host__ __device__ constexpr int sel_passes(bool is_int16, bool has_center) { return (is_int16 && !has_center) ? 2 : 4; }
__host__ __device__ constexpr long long sel_hists_per_read(int passes, int K) { return 1 + (long long)(passes - 1) * K; }
// first bin of the histogram of pass q, rank slot `slot`, inside a read's block of histograms
__device__ inline int sel_hist_offset(int q, int slot, int K) { return q == 0 ? 0 : (1 + (q - 1) * K + slot) * kSelBins; }

template <typename T, bool DEV>
__device__ inline unsigned sel_key(T x, float c) {
    if constexpr (DEV) {
        return __float_as_uint(fabsf(__fsub_rn((float)x, c)));
    } else if constexpr (sizeof(T) == 2) {
        return (unsigned)(unsigned short)x ^ 0x8000u;
    } else {
        const unsigned u = __float_as_uint(x);
        return u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    }
}

template <typename T, bool DEV>
__device__ inline float sel_value(unsigned key) {
    if constexpr (DEV) {
        return __uint_as_float(key);
    } else if constexpr (sizeof(T) == 2) {
        return (float)(short)(unsigned short)(key ^ 0x8000u);
    } else {
        return __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu));
    }
}

// One wave, one histogram of 256 bins, `rem` < its total: the bin that holds the rem-th smallest and the rank inside that bin.
__device__ inline void sel_scan(const unsigned* __restrict__ hist, unsigned rem, int lane, unsigned& digit, unsigned& rest) {
    const uint4 h = reinterpret_cast<const uint4*>(hist)[lane];
    const unsigned s1 = h.x, s2 = s1 + h.y, s3 = s2 + h.z, s4 = s3 + h.w;
    const unsigned incl = wave_scan(s4, lane, OpAdd());
    const unsigned excl = incl - s4;
    const unsigned long long mine = __ballot(rem >= excl && rem < incl);
    const int src = mine ? __ffsll((long long)mine) - 1 : 0;         // exactly one lane whenever rem < total
    const unsigned r = rem - excl;
    unsigned j = 3, below = s3;
    if (r < s1) { j = 0; below = 0; }
    else if (r < s2) { j = 1; below = s1; }
    else if (r < s3) { j = 2; below = s2; }
    digit = __shfl((unsigned)lane * 4 + j, src);
    rest = __shfl(r - below, src);
}

struct SelShared {
    unsigned prefix[kSelMaxK];
    int leader[kSelMaxK];        // the lowest live rank with the same prefix: its slot holds the histogram of the next pass
    int live[kSelMaxK];
};

// All 256 threads of a workgroup, len already checked.  After it, for every live rank k: sh.prefix[k] = the `upto` digits
// chosen so far (most significant first) and sh.leader[k] as above; the rank among the elements that share the prefix stays
// in the registers of the wave that owns k.  upto = 0 leaves prefix 0 and one leader for all live ranks.
__device__ inline void sel_chain(const unsigned* __restrict__ hist_b, const int* __restrict__ ranks_b, int K, int len, int upto,
                                 SelShared& sh) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    unsigned prefix[2] = {0u, 0u}, rem[2] = {0u, 0u};
    bool live[2] = {false, false};
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int k = wave + kSelWaves * i;
        if (k < K) {
            const int r = ranks_b[k];
            live[i] = r >= 0 && r < len;
            rem[i] = live[i] ? (unsigned)r : 0u;
        }
    }
    if (tid < kSelMaxK) {
        int first = -1;
        bool me = false;
        for (int j = 0; j < K; ++j) {
            const int r = ranks_b[j];
            const bool ok = r >= 0 && r < len;
            if (ok && first < 0) first = j;
            if (j == tid) me = ok;
        }
        sh.live[tid] = me ? 1 : 0;
        sh.leader[tid] = me ? first : -1;
        sh.prefix[tid] = 0u;
    }
    __syncthreads();
    for (int q = 0; q < upto; ++q) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int k = wave + kSelWaves * i;
            if (k < K && live[i]) {                                  // wave-uniform
                unsigned digit, rest;
                sel_scan(hist_b + sel_hist_offset(q, sh.leader[k], K), rem[i], lane, digit, rest);
                prefix[i] = (prefix[i] << 8) | digit;
                rem[i] = rest;
                if (lane == 0) sh.prefix[k] = prefix[i];
            }
        }
        __syncthreads();
        int lead = -1;
        if (tid < K && sh.live[tid]) {
            for (int j = tid; j >= 0; --j)
                if (sh.live[j] && sh.prefix[j] == sh.prefix[tid]) lead = j;
        }
        if (tid < K) sh.leader[tid] = lead;                          // read before the barrier above, next after the one below
        __syncthreads();
    }
}

// Every lane of a converged wave: lanes with `on` add 1 to h[idx].  Lanes that hit the same bin are served together, one atomic
// of their number by the first of them; after kSelAggRounds groups, or a group below kSelAggMin lanes (the values are spread:
// grouping costs more than it saves), the remaining lanes add one by one.  Concentrated signal puts nearly a whole wave into
// two or three bins, which plain same-address LDS atomics would serialise.
__device__ inline void sel_wave_add(unsigned* h, unsigned idx, bool on, int lane) {
    unsigned long long todo = __ballot(on);
#pragma unroll 1
    for (int round = 0; round < kSelAggRounds && todo; ++round) {
        const int first = __ffsll((long long)todo) - 1;
        const unsigned v = __shfl(idx, first);
        const unsigned long long same = __ballot(on && idx == v) & todo;
        const int n = __popcll(same);
        if (lane == first) atomicAdd(&h[v], (unsigned)n);
        todo &= ~same;
        if (n < kSelAggMin) break;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&h[idx], 1u);
}

template <typename T, bool DEV>
__global__ __launch_bounds__(kSelThreads) void select_pass_kernel(const T* __restrict__ signal, int ld,
                                                                  const int* __restrict__ signal_lengths,
                                                                  const int* __restrict__ ranks, int K,
                                                                  const float* __restrict__ center, int pass,
                                                                  unsigned* __restrict__ hist) {
    constexpr int kPasses = sel_passes(sizeof(T) == 2, DEV);
    constexpr int kVec = 16 / (int)sizeof(T);
    __shared__ unsigned lh[kSelMaxK * kSelBins];
    __shared__ SelShared sh;
    __shared__ unsigned u_prefix[kSelMaxK];
    __shared__ int u_slot[kSelMaxK];
    __shared__ int n_unique;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int len = signal_lengths[b];
    if (len < 0 || len > ld) return;                                 // refused: select_final_kernel reports it
    const long long t0 = (long long)blockIdx.x * kSelTile;
    if (t0 >= (long long)len) return;
    const int t1 = (int)(t0 + kSelTile < (long long)len ? t0 + kSelTile : (long long)len);
    unsigned* hist_b = hist + (long long)b * sel_hists_per_read(kPasses, K) * kSelBins;
    sel_chain(hist_b, ranks + (long long)b * K, K, len, pass, sh);
    for (int i = tid; i < kSelMaxK * kSelBins; i += kSelThreads) lh[i] = 0u;
    if (tid == 0) {
        int n = 0;
        for (int k = 0; k < K; ++k)
            if (sh.live[k] && sh.leader[k] == k) {
                u_prefix[n] = sh.prefix[k];
                u_slot[n] = k;
                ++n;
            }
        n_unique = n;
    }
    __syncthreads();
    const int nu = n_unique;
    if (nu == 0) return;                                             // no valid rank in this read
    unsigned up[kSelMaxK];
#pragma unroll
    for (int j = 0; j < kSelMaxK; ++j) up[j] = j < nu ? u_prefix[j] : 0xFFFFFFFFu;       // a prefix has at most 24 bits
    const int shift = (kPasses - 1 - pass) * 8;
    const float c = DEV ? center[b] : 0.0f;

    auto take = [&](T x, bool on) {
        const unsigned key = sel_key<T, DEV>(x, c);
        const unsigned hi = pass == 0 ? 0u : key >> (shift + 8);
        int u = -1;
#pragma unroll
        for (int j = 0; j < kSelMaxK; ++j)
            if (hi == up[j]) u = j;
        sel_wave_add(lh, (unsigned)(u < 0 ? 0 : u) * kSelBins + ((key >> shift) & 255u), on && u >= 0, lane);
    };

    const T* row = signal + (long long)b * ld;
    const int count = t1 - (int)t0;                                  // 1 .. kSelTile
    int head = (int)(((0 - reinterpret_cast<uintptr_t>(row + t0)) & 15) / sizeof(T));    // elements before a 16-byte boundary
    if (head > count) head = count;
    const int nvec = (count - head) / kVec;
    const int tail = count - head - nvec * kVec;
    {   // the misaligned head and the tail, one element per thread: head + tail < 2 kVec <= 16
        const bool on = tid < head + tail;
        const long long i = tid < head ? t0 + tid : t0 + head + (long long)nvec * kVec + (tid - head);
        T x = T(0);
        if (on) x = row[i];
        take(x, on);
    }
    const uint4* body = reinterpret_cast<const uint4*>(row + t0 + head);
    for (int v0 = 0; v0 < nvec; v0 += kSelThreads) {                 // uniform trip count: the waves stay converged for the ballots
        const bool on = v0 + tid < nvec;
        uint4 raw = make_uint4(0u, 0u, 0u, 0u);
        if (on) raw = body[v0 + tid];
        T x[kVec];
        __builtin_memcpy(x, &raw, 16);
#pragma unroll
        for (int e = 0; e < kVec; ++e) take(x[e], on);
    }
    __syncthreads();
    for (int u = 0; u < nu; ++u) {
        unsigned* dst = hist_b + sel_hist_offset(pass, pass == 0 ? 0 : u_slot[u], K);
        const unsigned n = lh[u * kSelBins + tid];                   // kSelThreads == kSelBins
        if (n) atomicAdd(dst + tid, n);
    }
}

template <typename T, bool DEV>
__global__ __launch_bounds__(kSelThreads) void select_final_kernel(int ld, const int* __restrict__ signal_lengths,
                                                                   const int* __restrict__ ranks, int K,
                                                                   const unsigned* __restrict__ hist, float* __restrict__ out,
                                                                   int* __restrict__ bad) {
    constexpr int kPasses = sel_passes(sizeof(T) == 2, DEV);
    __shared__ SelShared sh;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int len = signal_lengths[b];
    if (len < 0 || len > ld) {
        if (tid < K) {
            out[(long long)b * K + tid] = 0.0f;
            if (bad) atomicAdd(bad, 1);
        }
        return;
    }
    sel_chain(hist + (long long)b * sel_hists_per_read(kPasses, K) * kSelBins, ranks + (long long)b * K, K, len, kPasses, sh);
    if (tid < K) {
        float v = 0.0f;
        if (sh.live[tid]) v = sel_value<T, DEV>(sh.prefix[tid]);
        else if (bad) atomicAdd(bad, 1);
        out[(long long)b * K + tid] = v;
    }
}

template <typename T, bool DEV>
static int select_launch(const void* signal, int batch, int ld, const int* signal_lengths, const int* ranks, int K,
                         const float* center, float* out, unsigned* hist, int* bad, hipStream_t stream) {
    constexpr int kPasses = sel_passes(sizeof(T) == 2, DEV);
    const dim3 grid((unsigned)((ld + kSelTile - 1) / kSelTile), (unsigned)batch);
    for (int pass = 0; pass < kPasses; ++pass) {
        hipLaunchKernelGGL((select_pass_kernel<T, DEV>), grid, dim3(kSelThreads), 0, stream, reinterpret_cast<const T*>(signal), ld,
                           signal_lengths, ranks, K, center, pass, hist);
        WN_HIP(hipGetLastError(), "read_select pass");
    }
    hipLaunchKernelGGL((select_final_kernel<T, DEV>), dim3((unsigned)batch), dim3(kSelThreads), 0, stream, ld, signal_lengths, ranks,
                       K, hist, out, bad);
    WN_HIP(hipGetLastError(), "read_select final");
    return WN_OK;
}

}  // namespace wn
using namespace wn;

size_t wn_read_select_workspace_bytes(int batch, int K, int signal_is_int16, int has_center) {
    if (batch < 1 || batch > 65535 || K < 1 || K > kSelMaxK) return 0;
    return (size_t)batch * (size_t)sel_hists_per_read(sel_passes(signal_is_int16 != 0, has_center != 0), K) * kSelBins * sizeof(unsigned);
}

int wn_read_select(const void* signal, int signal_is_int16, int batch, int ld, const int* signal_lengths, const int* ranks, int K,
                   const float* center, float* out, void* workspace, size_t workspace_bytes, int* bad, wn_stream_t stream) {
    if (batch <= 0 || ld <= 0 || K <= 0) return WN_ERR_BAD_SHAPE;
    if (K > kSelMaxK || batch > 65535 || ld >= kSelMaxDim) return WN_ERR_UNSUPPORTED;
    if (((long long)ld + kSelTile - 1) / kSelTile * batch * kSelThreads >= kSelMaxGridThreads) return WN_ERR_UNSUPPORTED;
    if (!signal || !signal_lengths || !ranks || !out || !workspace) return WN_ERR_NULL;
    const size_t need = wn_read_select_workspace_bytes(batch, K, signal_is_int16, center != nullptr);
    if ((reinterpret_cast<uintptr_t>(workspace) & 15) || workspace_bytes < need) return WN_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(signal) & (signal_is_int16 ? 1 : 3)) return WN_ERR_WORKSPACE;       // not aligned to its element
    hipStream_t s = (hipStream_t)stream;
    WN_HIP(hipMemsetAsync(workspace, 0, need, s), "read_select memset");
    unsigned* hist = reinterpret_cast<unsigned*>(workspace);
    if (signal_is_int16)
        return center ? select_launch<short, true>(signal, batch, ld, signal_lengths, ranks, K, center, out, hist, bad, s)
                      : select_launch<short, false>(signal, batch, ld, signal_lengths, ranks, K, center, out, hist, bad, s);
    return center ? select_launch<float, true>(signal, batch, ld, signal_lengths, ranks, K, center, out, hist, bad, s)
                  : select_launch<float, false>(signal, batch, ld, signal_lengths, ranks, K, center, out, hist, bad, s);
}
