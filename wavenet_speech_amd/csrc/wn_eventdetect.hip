// Event detection: a raw read in, the table of its events out -- where the level changes -- with no bases
// and no network.  Samples are quantised exactly as the event tables do (wn_signal_dev.h); everything after that is an integer.
//
// The definition.  q_t = llrint(v_t 2^F), |q| < 2^23, T = signal_lengths[b].  Two detectors, d = 0 (short) and d = 1 (long), each
// with a window w (1..16; w_1 = 0 switches the long one off), a radius r (1..64), a threshold theta (int32 >= 1, on t^2 in units
// of 2^-8) and a variance floor vmin (int64, 1..2^55).  For a position i with w <= i <= T - w:
//     S1 = sum q[i-w .. i),  S2 = sum q[i .. i+w),  Q = sum of q^2 over both windows,
//     A_i = w (S2 - S1)^2  (< 2^60),   V_i = max(w Q - S1^2 - S2^2, vmin)  (<= 2^55),   score(i) = A_i / V_i
// which is Welch's t^2 between two equal windows; every other position has score 0 (A = 0, V = 1).  Scores are compared as
// rationals, A_i V_j against A_j V_i in 128-bit products, and i passes the threshold iff 256 A_i >= theta V_i: no division, no
// square root, no float.  i is a PEAK of detector d iff it passes the threshold, its score is strictly greater than that of every
// j in [i - r, i) and greater than or equal to that of every j in (i, i + r]: the arg-max of its neighbourhood, ties to the
// smaller index.  The boundaries of a read with T >= 1: position 0, every short peak, and every long peak with no short peak
// within +-w_1.  A gap between consecutive boundaries (T counts as the last one) longer than max_event_len (1..65536) also gets a
// forced boundary every max_event_len samples after its left end.  Event e is [b_e, b_(e+1)).
//
//   event_peaks_kernel<T>   grid (ceil(max_signal / chunk), batch), 256 threads; a workgroup walks its chunk in tiles of 768
//                           positions.  Per tile: quantise and validate the tile and a halo of max(w_0 + r_0 + w_1, r_1 + w_1)
//                           <= 96 samples a side into LDS; per detector form (A, V) of every position the tile's peaks can see,
//                           then the arg-max of every power-of-two run by log-step doubling (floor(log2(2 r + 1)) steps of one
//                           exact comparison per position: a neighbourhood is two overlapping runs), then one comparison and the
//                           threshold per position; peaks leave as ballot words.  The merge rule reads the short peaks' words
//                           through a (2 w_1 + 1)-bit mask.  Out: two bit planes in the workspace (boundary; boundary of the long
//                           detector), one 64-bit word per 64 positions, and the per-read bad flag.  Tiles past the read's end
//                           are skipped, and so are the words past it: nothing reads them.
//   event_ranks_kernel      one workgroup (1024 threads) per read, a word per thread and 1024 words per step: a max-scan carries
//                           the last boundary across words and steps, each boundary counts itself and the forced splits before
//                           it (with max_event_len >= 64 only a word's first boundary can have any), a sum-scan ranks them;
//                           every thread then writes starts / ev_kind of its boundaries and of the forced splits before them
//                           (a gap inside a word is below 64 samples: at most 62 splits).  Only the gap before a word's first
//                           boundary, or before the read's end, is unbounded: above 16 splits it goes to a shared list (one
//                           entry per thread at the most) and is written by the whole workgroup.  n_events is the true count,
//                           whatever max_events.
//   event_sums_kernel<T>    grid (ceil((max_events + 1) / 256), batch): a wave takes 64 consecutive events, one lane each, as
//                           kmer_events_kernel does: an event of up to 32 samples is summed by its lane, a longer one by the
//                           whole wave (lanes striding its samples, integer butterfly), so an event of 65536 samples is 1024
//                           steps of a wave.  The rows past the last event, and every row of a bad read, are filled here.
//
// The chunk tunes the grid and nothing else: every position is decided from its own neighbourhood, wherever the seams fall.  No
// value of a length or a sample is used as an index before it is checked; every LDS index is bounded by the tile's geometry.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"
#include "wn_signal_dev.h"
#include "wn_wave_dev.h"

namespace wn {

typedef unsigned long long u64;
typedef unsigned __int128 u128;

constexpr int kEdThreads = 256;
constexpr int kEdTile = 768;                  // positions per tile: a multiple of 256
constexpr int kEdMaxWindow = 16;
constexpr int kEdMaxRadius = 64;
constexpr int kEdMaxScoreHalo = kEdMaxWindow + kEdMaxRadius;         // scores a side: max(w_1 + r_0, r_1)
constexpr int kEdMaxHalo = kEdMaxScoreHalo + kEdMaxWindow;           // samples a side
constexpr int kEdSamples = kEdTile + 2 * kEdMaxHalo;
constexpr int kEdScores = kEdTile + 2 * kEdMaxScoreHalo;
constexpr int kEdPerThread = (kEdScores + kEdThreads - 1) / kEdThreads;
constexpr int kEdFlagWords = kEdTile / 64 + 2;                       // the tile and 64 positions a side
constexpr long long kEdMaxVmin = 1ll << 55;
constexpr int kEdMaxEventLen = 65536;         // sum of q^2 < 2^16 * 2^46 = 2^62
constexpr int kEdMaxSignal = 1 << 24;
constexpr int kEdMaxEvents = 1 << 24;
constexpr int kEdMinChunk = 256, kEdMaxChunk = 16384;
constexpr int kEdRankThreads = 1024;
constexpr int kEdInlineSplits = 16;           // up to here a thread writes the forced splits before its word's first boundary itself
constexpr int kEdShort = 32;                  // up to here one lane sums the event; above, the whole wave

struct DetectArgs {
    const void* signal;
    const int* signal_lengths;
    const float* scale_shift;           // [B][2] or nullptr
    long long signal_stride;
    int B, max_signal, max_events, max_event_len, chunk, words;      // words: 64-bit words per read in a bit plane
    double two_f;                       // 2^frac_bits
    int w[2], r[2], theta[2];
    long long vmin[2];
    int* n_events;
    int* starts;
    long long* ev_sum;
    long long* ev_sumsq;
    int* ev_kind;                       // or nullptr
    int* flag;                          // workspace: [B]
    u64* bits_any;                      // workspace: [B][words]
    u64* bits_long;                     // workspace: [B][words]
    int* bad;
};

struct DetectTile {
    int q[kEdSamples];
    u64 A[kEdScores], V[kEdScores];
    int idx[kEdScores];
    u64 peaks[2][kEdFlagWords];
};

// the arg-max of two positions of the tile: the greater score A / V, the smaller index on a tie
__device__ __forceinline__ int ed_pick(const DetectTile& s, int x, int y) {
    const u128 px = (u128)s.A[x] * s.V[y], py = (u128)s.A[y] * s.V[x];
    return (px > py || (px == py && x <= y)) ? x : y;
}

// One detector over one tile.  Scores of the positions [p0 - hs, p0 + pt + hs), run arg-maxima, then the peaks among the
// positions [p0 - need, p0 + pt + need) as bit words over [p0 - 64, p0 + pt + 64); need + r <= hs and hs + w <= hq.
__device__ __forceinline__ void ed_detector(DetectTile& s, u64* out, int p0, int pt, int hq, int hs, int need, int w, int r, int theta,
                                            long long vmin, int Tn, int tid) {
    const int N = pt + 2 * hs;
    for (int x = tid; x < N; x += kEdThreads) {
        const int n = p0 - hs + x;
        u64 A = 0, V = 1;
        if (n >= w && n <= Tn - w) {
            const int* qq = s.q + (x + hq - hs - w);                 // sample n - w
            int s1 = 0, s2 = 0;                                      // |s| <= 16 * 2^23
            u64 Q = 0;
            for (int k = 0; k < w; ++k) {
                const int u = qq[k], v = qq[w + k];
                s1 += u;
                s2 += v;
                Q += (u64)((long long)u * u) + (u64)((long long)v * v);
            }
            const int d = s2 - s1;                                   // |d| < 2^28
            A = (u64)w * (u64)((long long)d * d);
            const long long var = (long long)((u64)w * Q) - (long long)s1 * s1 - (long long)s2 * s2; // >= 0 (Cauchy-Schwarz), <= 2^55
            V = (u64)(var > vmin ? var : vmin);
        }
        s.A[x] = A;
        s.V[x] = V;
        s.idx[x] = x;
    }
    __syncthreads();
    const int L = 31 - __clz(2 * r + 1);                             // 2^L <= 2 r + 1 < 2^(L + 1)
    for (int k = 0; k < L; ++k) {                                    // idx[x]: the arg-max of [x, x + 2^(k + 1)), cut at N
        const int step = 1 << k;
        int nv[kEdPerThread];
#pragma unroll
        for (int it = 0; it < kEdPerThread; ++it) {
            const int x = tid + it * kEdThreads;
            if (x < N) {
                const int y = x + step < N ? x + step : N - 1;
                nv[it] = ed_pick(s, s.idx[x], s.idx[y]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < kEdPerThread; ++it) {
            const int x = tid + it * kEdThreads;
            if (x < N) s.idx[x] = nv[it];
        }
        __syncthreads();
    }
    const int lane = tid & 63;
    for (int wd = tid >> 6; wd < pt / 64 + 2; wd += kEdThreads / 64) {
        const int i = p0 - 64 + 64 * wd + lane;
        bool peak = false;
        if (i >= p0 - need && i < p0 + pt + need) {
            const int x = i - (p0 - hs);                             // r <= x and x + r < N
            if ((u128)s.A[x] * 256u >= (u128)s.V[x] * (u64)theta)
                peak = ed_pick(s, s.idx[x - r], s.idx[x + r + 1 - (1 << L)]) == x;
        }
        const u64 word = __ballot(peak);
        if (lane == 0) out[wd] = word;
    }
    __syncthreads();
}

template <typename T>
__global__ __launch_bounds__(kEdThreads) void event_peaks_kernel(const DetectArgs a) {
    __shared__ DetectTile s;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int Tn = a.signal_lengths[b];
    if (Tn < 0 || Tn > a.max_signal) {                               // nothing of such a read is looked at
        if (blockIdx.x == 0 && tid == 0) atomicOr(a.flag + b, 1);
        return;
    }
    const long long c0 = (long long)blockIdx.x * a.chunk;
    if (c0 >= Tn) return;                                            // workgroup-uniform
    const int w1 = a.w[1];
    const int hs0 = w1 + a.r[0], hs1 = a.r[1];
    const int hq0 = hs0 + a.w[0], hq1 = w1 > 0 ? hs1 + w1 : 0;
    const int hq = hq0 > hq1 ? hq0 : hq1;                            // <= 96
    const T* sig = (const T*)a.signal + (long long)b * a.signal_stride;
    const auto [scaled, scale, shift] = read_scale(a.scale_shift, b);
    const int cend = (int)(c0 + a.chunk);
    for (int p0 = (int)c0; p0 < cend && p0 < Tn; p0 += kEdTile) {
        const int pt = cend - p0 < kEdTile ? cend - p0 : kEdTile;    // a multiple of 256
        bool bad = false;
        for (int x = tid; x < pt + 2 * hq; x += kEdThreads) {
            const int n = p0 - hq + x;
            int q = 0;
            if (n >= 0 && n < Tn && !quantise(sig[n], scaled, scale, shift, a.two_f, &q)) { bad = true; q = 0; }
            s.q[x] = q;
        }
        if (bad) atomicOr(a.flag + b, 1);
        __syncthreads();
        ed_detector(s, s.peaks[0], p0, pt, hq, hs0, w1, a.w[0], a.r[0], a.theta[0], a.vmin[0], Tn, tid);
        if (w1 > 0) ed_detector(s, s.peaks[1], p0, pt, hq, hs1, 0, w1, a.r[1], a.theta[1], a.vmin[1], Tn, tid);
        const u64 mask = (1ull << (2 * w1 + 1)) - 1ull;              // the short peaks within +-w_1
        for (int wd = tid >> 6; wd < pt / 64; wd += kEdThreads / 64) {
            const int lo = 64 + 64 * wd + lane - w1;                 // bit of position i - w_1 in the short peaks' words; >= 48
            const int sh = lo & 63;
            u64 win = s.peaks[0][lo >> 6] >> sh;
            if (sh) win |= s.peaks[0][(lo >> 6) + 1] << (64 - sh);   // word pt / 64 + 1 at most
            const bool short_here = (win >> w1) & 1ull;
            const bool long_here = w1 > 0 && ((s.peaks[1][wd + 1] >> lane) & 1ull) && (win & mask) == 0ull;
            const u64 any = __ballot(short_here || long_here), lng = __ballot(long_here);
            const int i0 = p0 + 64 * wd;
            if (lane == 0 && i0 < Tn) {                              // i0 / 64 < words: the word holds a position of the read
                a.bits_any[(long long)b * a.words + (i0 >> 6)] = any;
                a.bits_long[(long long)b * a.words + (i0 >> 6)] = lng;
            }
        }
        __syncthreads();                                             // the next tile overwrites s
    }
}

// the forced splits between a boundary and its predecessor; no division for the common gap within max_event_len
__device__ __forceinline__ int ed_splits(int p, int prev, int M) { return p - prev > M ? (p - prev - 1) / M : 0; }

__device__ __forceinline__ void ed_write(const DetectArgs& a, int b, int rank, int pos, int kind) {
    if (rank <= a.max_events) a.starts[(long long)b * (a.max_events + 1) + rank] = pos;
    if (rank < a.max_events && a.ev_kind) a.ev_kind[(long long)b * a.max_events + rank] = kind;
}

__global__ __launch_bounds__(kEdRankThreads) void event_ranks_kernel(const DetectArgs a) {
    __shared__ int s_wave[kEdRankThreads / 64];
    __shared__ int s_big[kEdRankThreads][3];                         // (left end, forced splits, rank of the first): one per thread at most
    __shared__ int s_nbig;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Tn = a.signal_lengths[b];
    if (Tn < 0 || Tn > a.max_signal || a.flag[b] != 0) {             // workgroup-uniform: the first launch is complete
        if (tid == 0) {
            a.n_events[b] = -1;
            if (a.bad) atomicAdd(a.bad, 1);
        }
        return;
    }
    if (Tn == 0) {
        if (tid == 0) a.n_events[b] = 0;
        return;
    }
    const int M = a.max_event_len;
    const int nwords = (Tn + 63) >> 6;
    const u64* any_row = a.bits_any + (long long)b * a.words;
    const u64* long_row = a.bits_long + (long long)b * a.words;
    int last = -1, count = 0;                                        // the last boundary so far and the events before it
    for (int base = 0; base < nwords; base += kEdRankThreads) {
        const int wd = base + tid;
        u64 word = 0, lng = 0;
        if (wd < nwords) {
            word = any_row[wd];
            lng = long_row[wd];
            if (wd == nwords - 1 && (Tn & 63)) word &= (1ull << (Tn & 63)) - 1ull;   // no boundary at or past T (none is ever set)
            if (wd == 0) word |= 1ull;                               // position 0
        }
        if (tid == 0) s_nbig = 0;
        int before, total_last;
        before = block_scan<kEdRankThreads / 64>(word ? wd * 64 + 63 - __clzll((long long)word) : -1, tid, s_wave, &total_last, OpMax(), -1);
        __syncthreads();                                             // s_wave is free again
        if (before < last) before = last;
        int mine = 0, prev = before;
        if (M >= 64) {                                               // a gap inside a word is below 64 <= M: only the first boundary has splits
            if (word) mine = __popcll(word) + ed_splits(wd * 64 + __ffsll((long long)word) - 1, before, M);
        } else {
            for (u64 rest = word; rest; rest &= rest - 1) {
                const int p = wd * 64 + __ffsll((long long)rest) - 1;
                mine += 1 + ed_splits(p, prev, M);                   // prev = -1 before position 0: no split
                prev = p;
            }
        }
        int total;
        const int ex = block_scan<kEdRankThreads / 64>(mine, tid, s_wave, &total);
        __syncthreads();                                             // s_wave is free again
        int rank = count + ex;
        prev = before;
        for (u64 rest = word; rest; rest &= rest - 1) {
            const int bit = __ffsll((long long)rest) - 1;
            const int p = wd * 64 + bit;
            const int splits = ed_splits(p, prev, M);
            // Only the gap that reaches back before the word is unbounded, so only a word's first boundary may go to the shared list:
            // at most one entry per thread.  A gap inside the word is below 64 samples, at most 62 splits, and is written here
            if (rest == word && splits > kEdInlineSplits) {
                const int at = atomicAdd(&s_nbig, 1);
                s_big[at][0] = prev;
                s_big[at][1] = splits;
                s_big[at][2] = rank;
            } else {
                for (int k = 0; k < splits; ++k) ed_write(a, b, rank + k, prev + (k + 1) * M, 3);
            }
            rank += splits;
            ed_write(a, b, rank, p, p == 0 ? 0 : ((lng >> bit) & 1ull) ? 2 : 1);
            ++rank;
            prev = p;
        }
        __syncthreads();
        const int nbig = s_nbig;
        for (int g = 0; g < nbig; ++g) {                             // the order of the list changes no output
            const int left = s_big[g][0], splits = s_big[g][1], first = s_big[g][2];
            for (int k = tid; k < splits; k += kEdRankThreads) ed_write(a, b, first + k, left + (k + 1) * M, 3);
        }
        __syncthreads();                                             // s_nbig and s_big are free again
        if (total_last > last) last = total_last;
        count += total;
    }
    const int splits = ed_splits(Tn, last, M);                          // the last event against the read's end
    for (int k = tid; k < splits; k += kEdRankThreads) ed_write(a, b, count + k, last + (k + 1) * M, 3);
    if (tid == 0) a.n_events[b] = count + splits;
}

template <typename T>
__global__ __launch_bounds__(kEdThreads) void event_sums_kernel(const DetectArgs a) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const long long e64 = (long long)blockIdx.x * kEdThreads + tid;
    const int N = a.max_events;
    const int n = a.n_events[b];                                     // -1: a bad read
    const int Tn = a.signal_lengths[b];
    const bool row = e64 < N;
    const int e = (int)e64;
    int* starts = a.starts + (long long)b * (N + 1);
    if (e64 <= N && (n < 0 || e >= n)) starts[e] = n < 0 ? -1 : Tn;
    const bool used = row && e < n;
    int start = 0, len = 0;
    if (used) {
        start = starts[e];                                           // written by the second launch: 0 <= start < end <= T
        len = (e + 1 < n ? starts[e + 1] : Tn) - start;
    }
    const T* sig = (const T*)a.signal + (long long)b * a.signal_stride;
    const auto [scaled, scale, shift] = read_scale(a.scale_shift, b);
    long long sum = 0, sumsq = 0;
    if (used && len <= kEdShort) {
        for (int t = 0; t < len; ++t) {
            int q = 0;
            quantise(sig[start + t], scaled, scale, shift, a.two_f, &q);             // validated by the first launch
            sum += q;
            sumsq += (long long)q * q;
        }
    }
    u64 wide = __ballot(used && len > kEdShort);
    while (wide) {                                                   // wave-uniform
        const int src = __ffsll((long long)wide) - 1;
        wide &= wide - 1;
        const int st = __shfl(start, src), ln = __shfl(len, src);
        long long s1 = 0, s2 = 0;
        for (int t = lane; t < ln; t += 64) {
            int q = 0;
            quantise(sig[st + t], scaled, scale, shift, a.two_f, &q);
            s1 += q;
            s2 += (long long)q * q;
        }
        wave_reduce_each(OpAdd(), s1, s2);
        if (lane == src) { sum = s1; sumsq = s2; }
    }
    if (!row) return;
    const long long o = (long long)b * N + e;
    a.ev_sum[o] = sum;
    a.ev_sumsq[o] = sumsq;
    if (!used && a.ev_kind) a.ev_kind[o] = -1;
}

static bool ed_chunk_ok(int chunk) { return chunk == 0 || (chunk >= kEdMinChunk && chunk <= kEdMaxChunk && chunk % 256 == 0); }

// the automatic chunk: four tiles, halved while the grid is short of four workgroups per CU
static int ed_auto_chunk(int batch, int max_signal) {
    int chunk = 4 * kEdTile;
    while (chunk > kEdTile && (long long)batch * cdiv(max_signal, chunk) < 1024) chunk /= 2;
    return chunk;
}

static size_t ed_flag_bytes(int batch) { return align256((size_t)batch * sizeof(int)); }
static size_t ed_plane_bytes(int batch, int max_signal) { return align256((size_t)batch * (size_t)cdiv(max_signal, 64) * sizeof(u64)); }

}  // namespace wn
using namespace wn;

size_t wn_event_detect_workspace_bytes(int batch, int max_signal) {
    if (batch < 1 || batch > 65535 || max_signal < 1 || max_signal > kEdMaxSignal) return 0;
    return ed_flag_bytes(batch) + 2 * ed_plane_bytes(batch, max_signal);
}

int wn_event_detect(const void* signal, int signal_kind, long long signal_stride, const int* signal_lengths, const float* scale_shift,
                    int batch, int max_signal, int frac_bits, int window_short, int window_long, int radius_short, int radius_long,
                    int threshold_short, int threshold_long, long long min_var_short, long long min_var_long, int max_event_len,
                    int max_events, int chunk_samples, int* n_events, int* starts, long long* ev_sum, long long* ev_sumsq, int* ev_kind,
                    void* workspace, size_t workspace_bytes, int* bad, wn_stream_t stream) {
    if (batch < 1 || max_signal < 1 || max_events < 1) return WN_ERR_BAD_SHAPE;
    if (signal_stride < 0 || signal_kind < 0 || signal_kind > 1) return WN_ERR_BAD_SHAPE;
    if (frac_bits < 0 || frac_bits > kSigMaxFrac || batch > 65535 || max_signal > kEdMaxSignal || max_events > kEdMaxEvents)
        return WN_ERR_UNSUPPORTED;
    if (window_short < 1 || window_short > kEdMaxWindow || radius_short < 1 || radius_short > kEdMaxRadius || threshold_short < 1 ||
        min_var_short < 1 || min_var_short > kEdMaxVmin)
        return WN_ERR_UNSUPPORTED;
    if (window_long < 0 || window_long > kEdMaxWindow) return WN_ERR_UNSUPPORTED;
    if (window_long > 0 && (radius_long < 1 || radius_long > kEdMaxRadius || threshold_long < 1 || min_var_long < 1 ||
                            min_var_long > kEdMaxVmin))
        return WN_ERR_UNSUPPORTED;
    if (max_event_len < 1 || max_event_len > kEdMaxEventLen || !ed_chunk_ok(chunk_samples)) return WN_ERR_UNSUPPORTED;
    if (!signal || !signal_lengths || !n_events || !starts || !ev_sum || !ev_sumsq || !workspace) return WN_ERR_NULL;
    if (workspace_bytes < wn_event_detect_workspace_bytes(batch, max_signal) || ((size_t)workspace & 15)) return WN_ERR_WORKSPACE;
    if (!signal_aligned(signal, signal_kind)) return WN_ERR_WORKSPACE;

    DetectArgs a = {};
    a.signal = signal; a.signal_lengths = signal_lengths; a.scale_shift = scale_shift; a.signal_stride = signal_stride;
    a.B = batch; a.max_signal = max_signal; a.max_events = max_events; a.max_event_len = max_event_len;
    a.chunk = chunk_samples ? chunk_samples : ed_auto_chunk(batch, max_signal);
    a.words = cdiv(max_signal, 64);
    a.two_f = (double)(1 << frac_bits);
    a.w[0] = window_short; a.r[0] = radius_short; a.theta[0] = threshold_short; a.vmin[0] = min_var_short;
    a.w[1] = window_long; a.r[1] = window_long ? radius_long : 1; a.theta[1] = threshold_long; a.vmin[1] = min_var_long;
    a.n_events = n_events; a.starts = starts; a.ev_sum = ev_sum; a.ev_sumsq = ev_sumsq; a.ev_kind = ev_kind;
    char* ws = (char*)workspace;
    a.flag = (int*)ws;
    a.bits_any = (u64*)(ws + ed_flag_bytes(batch));
    a.bits_long = (u64*)(ws + ed_flag_bytes(batch) + ed_plane_bytes(batch, max_signal));
    a.bad = bad;

    hipStream_t st = (hipStream_t)stream;
    WN_HIP(hipMemsetAsync(a.flag, 0, (size_t)batch * sizeof(int), st), "event_detect flags");
    const dim3 grid1((unsigned)cdiv(max_signal, a.chunk), (unsigned)batch);
    const dim3 grid3((unsigned)cdiv(max_events + 1, kEdThreads), (unsigned)batch);
    if (signal_kind)
        hipLaunchKernelGGL(event_peaks_kernel<short>, grid1, dim3(kEdThreads), 0, st, a);
    else
        hipLaunchKernelGGL(event_peaks_kernel<float>, grid1, dim3(kEdThreads), 0, st, a);
    WN_HIP(hipGetLastError(), "event_peaks");
    hipLaunchKernelGGL(event_ranks_kernel, dim3((unsigned)batch), dim3(kEdRankThreads), 0, st, a);
    WN_HIP(hipGetLastError(), "event_ranks");
    if (signal_kind)
        hipLaunchKernelGGL(event_sums_kernel<short>, grid3, dim3(kEdThreads), 0, st, a);
    else
        hipLaunchKernelGGL(event_sums_kernel<float>, grid3, dim3(kEdThreads), 0, st, a);
    WN_HIP(hipGetLastError(), "event_sums");
    return WN_OK;
}
