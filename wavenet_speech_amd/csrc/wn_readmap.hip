// Read mapping in base space on the device: which stretch of a reference, on which strand, a decoded read
// came from -- the step minimap2 runs after basecalling: sketch the read into minimizers, look them up in an index of the
// reference's minimizers, chain colinear hits.  Everything written is an integer and every rule is a lexicographic maximum (or
// minimum) over a set, so no order of evaluation changes a result; tests/readmap_ref.py states the same definition as plain loops.
//
// Labels: int32, 1..4 are bases with complement 5 - v (" AGCT"); anything else, 0 included, is a break.
//
//   K-MERS       the k-mer at p in [0, n - k] has the forward code f = sum_i (label[p+i] - 1) 4^(k-1-i) and the reverse-complement
//                code r = sum_i (4 - label[p+i]) 4^i, both uint32 (k <= 16).  It is INVALID if a label is outside 1..4 or f == r (a
//                palindrome); otherwise canon = min(f, r), strand = (r < f), hash = fmix32(canon) (murmur3's finaliser, a bijection
//                on 32 bits) and its key is the pair (hash, p).
//   MINIMIZERS   with n_k = n - k + 1 >= 1 the windows are [s, s + w) for s in [0, n_k - w]; if n_k < w there is the single window
//                [0, n_k).  p is a minimizer iff it holds a valid k-mer whose key is the lexicographic minimum over the valid k-mers
//                of at least one window (equal hashes: the smallest position).  A per-position predicate over a neighbourhood of
//                2 w - 1 positions: how the row is cut into chunks changes nothing.
//   INDEX        the reference's minimizers as one sorted int64 word each: canon << 28 | pos << 1 | strand, i.e. sorted by (canon, pos).
//   ANCHORS      of a read of length n: its minimizers in ascending position q, for each the index entries of equal canon in
//                ascending pos; a canon with more than max_occ entries is dropped whole.  An anchor is (s, r, q'): s = strand_read ^
//                strand_ref, r = pos, q' = q if s == 0 else n - k - q (the k-mer's start in the reverse-complemented read).  The first
//                anchors_per_read anchors of this enumeration are kept (truncated[b] = 1 if there were more), each as one sortable
//                int64 word s << 43 | r << 16 | q'; every row is then sorted ascending (keys are distinct: one result); pads are
//                INT64_MAX and stay last.
//   CHAINING     each strand on its own over its anchors sorted by (r, q').  f(i) = max over candidates of (score, j), lexicographic:
//                the fresh start (16 k, i), and every j in [max(0, i - h), i) with dr = r_i - r_j, dq = q'_i - q'_j, 0 < dr <= max_dist,
//                0 < dq <= max_dist, dd = |dr - dq| <= bandwidth as (f(j) + 16 min(dr, dq, k) - gap(dd), j); gap(0) = 0, else gap(dd) =
//                gap_base dd + gap_log floor(log2 dd).  So a fresh start beats an extension of equal score, and of equal extensions
//                the nearest predecessor wins (minimap2's rules).  Beside the score: root(i) = i or root(pred), count(i) = 1 or
//                count(pred) + 1.  16 k <= f <= 16 * 16 * 32768 = 2^23.
//   RESULT       the best anchor is the maximum of f over both strands, ties to the forward strand, then to the smallest i.  ref_start =
//                r_root, ref_end = r_best + k; the query span in read orientation: forward [q'_root, q'_best + k), reverse
//                [n - k - q'_best, n - q'_root); n_anchors = count; runner_up = the greatest f over all anchors whose (strand, root)
//                differs from the best one's, INT_MIN if there is none (predecessor links form a forest: chains with different roots
//                share no anchor, so no traceback is needed).  No anchors: score INT_MIN, strand and positions -1, n_anchors 0.
//
//   minimizer_kernel    grid (chunk, read), 256 threads.  A block stages the labels of its chunk with a halo of w - 1 + k - 1 on
//                       either side, writes the key of every k-mer start of the extended range to LDS (hash << 32 | p, all ones for
//                       an invalid one: above every valid key) and decides each position of the chunk from the runs of greater keys
//                       to its left and right (at most w - 1 steps each): p is the minimum of window s iff p - L <= s and s + w - 1 <= p + R.
//   read_seeds_kernel   one workgroup per read, tiles of 256 positions in order: a binary search of the index per minimizer, one
//                       workgroup prefix scan of (minimizer, hits) packed into one int, anchors written at their scanned offsets;
//                       then the workgroup sorts its kept anchors in place by a bitonic network over the next power of two.
//   chain_kernel        one workgroup per read, ONE WAVE PER STRAND.  The recurrence is serial over i; the 64 lanes take the
//                       predecessors j = i - 1 - lane in rounds of 64, nearest first.  A round's candidates are reduced by a DPP wave
//                       maximum of the scores (no LDS, no barrier); the first lane of the ballot that holds the maximum is the nearest
//                       predecessor, and a later round replaces an earlier one only with a strictly greater score, as an extension
//                       replaces the fresh start: the lexicographic maximum without packing.  f, count, r, q' and the root's (r, q') of
//                       the last h anchors live in an LDS ring of the next power of two; nothing but the wave itself touches it.  The
//                       best chain and the runner-up are carried as a running top two over DISTINCT roots.
//
// Nothing is read back, nothing is allocated, every result leaves through ordinary vector stores; all three run on the passed
// stream and can be captured into a graph.
#include <climits>

#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"
#include "wn_wave_dev.h"

namespace wn {

constexpr int kRmMaxK = 16;
constexpr int kRmMaxW = 64;
constexpr int kRmMaxOcc = 64;
constexpr int kRmMaxH = 1024;
constexpr int kRmMaxAnchors = 32768;
constexpr int kRmMaxRead = 65535;
constexpr int kRmMaxRef = 1 << 26;
constexpr int kRmMaxDist = 1 << 26;
constexpr int kRmMaxGap = 1024;
constexpr int kRmMaxChunk = 2048;
constexpr int kRmAutoChunk = 1024;
constexpr int kRmExt = kRmMaxChunk + 2 * (kRmMaxW - 1);          // k-mer starts a block looks at
constexpr int kRmStrandShift = 43, kRmRefShift = 16;             // anchor word: s << 43 | r << 16 | q'
constexpr int kRmIndexShift = 28;                                // index word: canon << 28 | pos << 1 | strand
constexpr long long kRmPosMask = (1LL << 27) - 1;
constexpr long long kRmRootMask = (1LL << kRmStrandShift) - 1;   // (r, q') of an anchor word

__device__ __forceinline__ unsigned rm_fmix32(unsigned x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}

struct MinimizerArgs {
    const int* labels;                   // [B] rows of labels_stride elements
    long long labels_stride;
    const int* lengths;                  // [B]
    unsigned* code;                      // [B][max_len]
    unsigned char* flag;                 // [B][max_len]
    int* bad;
    int B, max_len, k, w, chunk;
};

__global__ __launch_bounds__(256) void minimizer_kernel(const MinimizerArgs a) {
    __shared__ int lab[kRmExt + kRmMaxK - 1];
    __shared__ unsigned long long key[kRmExt];
    __shared__ unsigned canon[kRmExt];
    __shared__ unsigned char strand[kRmExt];                             // the flag a minimizer gets: 1 forward, 2 reverse complement
    const int b = blockIdx.y, tid = threadIdx.x;
    const int k = a.k, w = a.w;
    int n = a.lengths[b];
    const bool bad_read = n < 0 || n > a.max_len;
    if (bad_read) n = 0;                                                 // the length is never used as an index
    const int n_k = n - k + 1;
    const int c0 = blockIdx.x * a.chunk, e0 = c0 - (w - 1);              // first position of the chunk / of the extended range
    const int ext = a.chunk + 2 * (w - 1);
    const int* row = a.labels + (long long)b * a.labels_stride;
    for (int t = tid; t < ext + k - 1; t += 256) {
        const int p = e0 + t;
        lab[t] = p >= 0 && p < n ? row[p] : 0;
    }
    __syncthreads();
    for (int t = tid; t < ext; t += 256) {
        const int p = e0 + t;
        unsigned long long kk = ~0ull;                                   // invalid: above every valid key
        unsigned c = 0;
        bool rev = false;
        if (p >= 0 && p < n_k) {
            unsigned f = 0, r = 0;
            bool ok = true;
            for (int i = 0; i < k; ++i) {
                const int v = lab[t + i];
                ok = ok && v >= 1 && v <= 4;
                f = (f << 2) | (unsigned)((v - 1) & 3);
                r |= (unsigned)((4 - v) & 3) << (2 * i);
            }
            if (ok && f != r) {
                rev = r < f;
                c = rev ? r : f;
                kk = ((unsigned long long)rm_fmix32(c) << 32) | (unsigned long long)(unsigned)p;
            }
        }
        key[t] = kk;
        canon[t] = c;
        strand[t] = rev ? 2 : 1;
    }
    __syncthreads();
    for (int u = tid; u < a.chunk; u += 256) {
        const int p = c0 + u, t = u + (w - 1);
        if (p >= a.max_len) break;
        const unsigned long long mine = key[t];
        int fl = 0;
        if (mine != ~0ull) {
            int L = 0, R = 0;                                            // runs of greater keys (an invalid key is greater)
            while (L < w - 1 && key[t - 1 - L] > mine) ++L;
            while (R < w - 1 && key[t + 1 + R] > mine) ++R;
            bool is_min;
            if (n_k >= w) {
                const int lo = max(max(0, p - w + 1), p - L), hi = min(min(p, n_k - w), p + R - w + 1);
                is_min = lo <= hi;
            } else {
                is_min = p - L <= 0 && p + R >= n_k - 1;
            }
            if (is_min) fl = strand[t];
        }
        const long long o = (long long)b * a.max_len + p;
        a.code[o] = fl ? canon[t] : 0u;
        a.flag[o] = (unsigned char)fl;
    }
    if (bad_read && blockIdx.x == 0 && tid == 0 && a.bad) atomicAdd(a.bad, 1);
}

// ---- seeds ------------------------------------------------------------------------------------------------------------------

struct SeedArgs {
    const unsigned* code;                // [B][max_len]
    const unsigned char* flag;
    const int* lengths;                  // [B]
    const long long* index;              // [n_index] sorted
    long long* keys;                     // [B][cap]
    int* n_minimizers;                   // [B]
    int* n_anchors;
    int* truncated;
    int* bad;
    int n_index, B, max_len, k, max_occ, cap;
};

__device__ __forceinline__ int rm_lower_bound(const long long* v, int n, long long x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void read_seeds_kernel(const SeedArgs a) {
    __shared__ int wave_sum[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int n = a.lengths[b];
    const bool bad_read = n < 0 || n > a.max_len;
    if (bad_read) n = 0;
    long long* out = a.keys + (long long)b * a.cap;
    int total_min = 0, total_anchors = 0;                                // at most 65535 and 65535 * 64
    for (int base = 0; base < n; base += 256) {
        const int q = base + tid;
        const int fl = q < n ? a.flag[(long long)b * a.max_len + q] : 0;
        int lo = 0, cnt = 0;
        if (fl) {
            const long long c = (long long)a.code[(long long)b * a.max_len + q];
            lo = rm_lower_bound(a.index, a.n_index, c << kRmIndexShift);
            cnt = rm_lower_bound(a.index, a.n_index, (c + 1) << kRmIndexShift) - lo;
            if (cnt > a.max_occ) cnt = 0;                                // a repeat: dropped whole
        }
        // one scan for both counts: minimizers (<= 256) from bit 16 up, hits (<= 256 * 64 = 2^14) below
        const int v = (fl ? 1 << 16 : 0) + cnt;
        int inc = v;                                                     // by hand: with wave_scan / block_scan this stage measured 0.3 % slower
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(inc, d);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        int before, all;
        wave_offsets<4>(wave_sum, wave, &before, &all);
        __syncthreads();                                                 // wave_sum is written again in the next tile
        const int off = total_anchors + ((before + inc - v) & 0xFFFF);
        const int s_read = fl == 2;
        for (int j = 0; j < cnt; ++j) {
            if (off + j >= a.cap) break;
            const long long e = a.index[lo + j];
            const long long s = (long long)(s_read ^ (int)(e & 1));
            const long long pos = (e >> 1) & kRmPosMask;
            const long long qq = s ? n - a.k - q : q;
            out[off + j] = (s << kRmStrandShift) | (pos << kRmRefShift) | qq;
        }
        total_min += all >> 16;
        total_anchors += all & 0xFFFF;
    }
    const int kept = min(total_anchors, a.cap);
    for (int i = kept + tid; i < a.cap; i += 256) out[i] = LLONG_MAX;
    // sort the kept anchors where they lie (the row is this workgroup's own): a bitonic network over the next power of two in its
    // all-ascending form -- the first step of a merge mirrors, i with i ^ (k2 - 1), the others pair i with i | j, and every exchange
    // puts the smaller word at the lower index -- so that the slots from `kept` up count as +infinity and are never touched
    int pow2 = 1;
    while (pow2 < kept) pow2 <<= 1;
    for (int k2 = 2; k2 <= pow2; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            __syncthreads();                                             // the anchors, and the exchanges of the step before
            for (int t = tid; t < (pow2 >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = j == (k2 >> 1) ? i ^ (k2 - 1) : i | j;
                if (l < kept) {
                    const long long lo_word = out[i], hi_word = out[l];
                    if (lo_word > hi_word) { out[i] = hi_word; out[l] = lo_word; }
                }
            }
        }
    }
    if (tid == 0) {
        a.n_minimizers[b] = total_min;
        a.n_anchors[b] = kept;
        a.truncated[b] = total_anchors > a.cap ? 1 : 0;
        if (bad_read && a.bad) atomicAdd(a.bad, 1);
    }
}

// ---- chaining ---------------------------------------------------------------------------------------------------------------

struct ChainArgs {
    const long long* keys;               // [B][cap] sorted rows
    const int* n_anchors;                // [B]
    const int* lengths;                  // [B]
    int* result;                         // [B][8]
    int* f;                              // [B][cap] or NULL
    int* pred;
    int* bad;
    int B, max_len, cap, k, h, ring, max_dist, bandwidth, gap_base, gap_log;
};

constexpr int kRmFloor = -(1 << 30);     // a candidate this low has lost to the fresh start (16 k > 0) long ago

__global__ __launch_bounds__(128) void chain_kernel(const ChainArgs a) {
    extern __shared__ long long ring_mem[];                             // per wave: root [ring] int64, then f, count, r, q' [ring] int32
    __shared__ int res[2][8];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ring = a.ring, mask = ring - 1;
    long long* r_root = ring_mem + (long long)wave * 3 * ring;          // 8 + 4 * 4 = 24 bytes a slot
    int* r_f = (int*)(r_root + ring);
    int* r_cnt = r_f + ring;
    int* r_r = r_cnt + ring;
    int* r_q = r_r + ring;

    int n = a.n_anchors[b];
    const int len = a.lengths[b];
    const bool bad_read = len < 0 || len > a.max_len || n < 0 || n > a.cap;
    if (bad_read) n = 0;                                                 // neither is ever used as an index
    const long long* row = a.keys + (long long)b * a.cap;
    int nf = 0;                                                          // the forward strand's anchors come first
    {
        int hi = n;
        while (nf < hi) {
            const int mid = (nf + hi) >> 1;
            if (row[mid] < (1LL << kRmStrandShift)) nf = mid + 1; else hi = mid;
        }
    }
    const int begin = wave ? nf : 0, m = (wave ? n : nf) - begin;
    const int k = a.k, fresh = 16 * k;

    int b_f = INT_MIN, b_f2 = INT_MIN, b_r = -1, b_q = -1, b_cnt = 0;
    long long b_root = -1;
    long long mine = 0;
    for (int i = 0; i < m; ++i) {
        if ((i & 63) == 0) mine = i + lane < m ? row[begin + i + lane] : 0;
        const int src = i & 63;                                          // wave-uniform
        const unsigned k_lo = __builtin_amdgcn_readlane((int)(unsigned)(mine & 0xFFFFFFFFll), src);
        const unsigned k_hi = __builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)mine >> 32), src);
        const long long ki = (long long)(((unsigned long long)k_hi << 32) | k_lo) & kRmRootMask;
        const int ri = (int)(ki >> kRmRefShift), qi = (int)(ki & 0xFFFF);
        const int npred = min(i, a.h);
        int best = fresh, best_d = -1;
        for (int t0 = 0; t0 < npred; t0 += 64) {
            const int d = t0 + lane;
            int sc = INT_MIN;
            if (d < npred) {
                const int slot = (i - 1 - d) & mask;
                const int dr = ri - r_r[slot], dq = qi - r_q[slot];
                if (dr > 0 && dr <= a.max_dist && dq > 0 && dq <= a.max_dist) {
                    const int dd = abs(dr - dq);
                    if (dd <= a.bandwidth) {
                        const long long gap = dd ? (long long)a.gap_base * dd + (long long)a.gap_log * (31 - __clz(dd)) : 0;
                        const long long c = (long long)r_f[slot] + 16 * min(min(dr, dq), k) - gap;
                        sc = c < kRmFloor ? kRmFloor : (int)c;
                    }
                }
            }
            const int top = wave_max_dpp(sc);
            if (top > best) {                                            // strictly: the earlier (nearer) round and the fresh start win ties
                best = top;
                best_d = t0 + __ffsll((unsigned long long)__ballot(sc == top)) - 1;
            }
        }
        int cnt_i = 1, pr = -1;
        long long root_i = ki;
        if (best_d >= 0) {
            const int slot = (i - 1 - best_d) & mask;
            root_i = r_root[slot]; cnt_i = r_cnt[slot] + 1; pr = begin + i - 1 - best_d;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            const int slot = i & mask;
            r_root[slot] = root_i; r_f[slot] = best; r_cnt[slot] = cnt_i; r_r[slot] = ri; r_q[slot] = qi;
            if (a.f) { a.f[(long long)b * a.cap + begin + i] = best; a.pred[(long long)b * a.cap + begin + i] = pr; }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");           // the ring is the wave's own: its LDS accesses stay in order
        // the running top two over distinct roots; i ascends, so "strictly greater" keeps the smallest i
        if (root_i == b_root) {
            if (best > b_f) { b_f = best; b_r = ri; b_q = qi; b_cnt = cnt_i; }
        } else if (best > b_f) {
            b_f2 = b_f; b_f = best; b_root = root_i; b_r = ri; b_q = qi; b_cnt = cnt_i;
        } else {
            b_f2 = max(b_f2, best);
        }
    }
    if (lane == 0) {
        int* o = res[wave];
        o[0] = b_f; o[1] = b_f2; o[2] = (int)(b_root >> kRmRefShift); o[3] = (int)(b_root & 0xFFFF); o[4] = b_r; o[5] = b_q; o[6] = b_cnt;
    }
    if (a.f)
        for (int i = n + tid; i < a.cap; i += 128) { a.f[(long long)b * a.cap + i] = INT_MIN; a.pred[(long long)b * a.cap + i] = -1; }
    __syncthreads();
    if (tid == 0) {
        int* o = a.result + (long long)b * 8;
        const int s = res[1][0] > res[0][0] ? 1 : 0;                     // ties to the forward strand
        const int* w = res[s];
        if (w[0] == INT_MIN) {
            o[0] = INT_MIN; o[1] = -1; o[2] = -1; o[3] = -1; o[4] = -1; o[5] = -1; o[6] = 0; o[7] = INT_MIN;
        } else {
            o[0] = w[0]; o[1] = s; o[2] = w[2]; o[3] = w[4] + k;
            o[4] = s ? len - k - w[5] : w[3];
            o[5] = s ? len - w[3] : w[5] + k;
            o[6] = w[6];
            o[7] = max(w[1], res[1 - s][0]);
        }
        if (bad_read && a.bad) atomicAdd(a.bad, 1);
    }
}

}  // namespace wn

using namespace wn;

int wn_minimizers(const int* labels, long long labels_stride, const int* lengths, int batch, int max_len, int k, int w, int chunk,
                  unsigned* code, unsigned char* flag, int* bad, wn_stream_t stream) {
    if (batch <= 0 || max_len <= 0 || labels_stride < 0 || chunk < 0) return WN_ERR_BAD_SHAPE;
    if (batch > 65535 || max_len > kRmMaxRef || k < 1 || k > kRmMaxK || w < 1 || w > kRmMaxW || chunk > kRmMaxChunk) return WN_ERR_UNSUPPORTED;
    if (!labels || !lengths || !code || !flag) return WN_ERR_NULL;
    MinimizerArgs a = {};
    a.labels = labels; a.labels_stride = labels_stride; a.lengths = lengths; a.code = code; a.flag = flag; a.bad = bad;
    a.B = batch; a.max_len = max_len; a.k = k; a.w = w;
    a.chunk = chunk ? chunk : kRmAutoChunk;
    hipLaunchKernelGGL(minimizer_kernel, dim3(cdiv(max_len, a.chunk), batch), dim3(256), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "minimizers");
    return WN_OK;
}

int wn_read_seeds(const unsigned* code, const unsigned char* flag, const int* lengths, const long long* index, int n_index, int batch,
                  int max_len, int k, int max_occ, int anchors_per_read, long long* keys, int* n_minimizers, int* n_anchors,
                  int* truncated, int* bad, wn_stream_t stream) {
    if (batch <= 0 || max_len <= 0 || n_index < 0) return WN_ERR_BAD_SHAPE;
    if (batch > 65535 || max_len > kRmMaxRead || n_index > kRmMaxRef || k < 1 || k > kRmMaxK || max_occ < 1 || max_occ > kRmMaxOcc ||
        anchors_per_read < 1 || anchors_per_read > kRmMaxAnchors)
        return WN_ERR_UNSUPPORTED;
    if (!code || !flag || !lengths || !index || !keys || !n_minimizers || !n_anchors || !truncated) return WN_ERR_NULL;
    SeedArgs a = {};
    a.code = code; a.flag = flag; a.lengths = lengths; a.index = index; a.keys = keys; a.n_minimizers = n_minimizers;
    a.n_anchors = n_anchors; a.truncated = truncated; a.bad = bad;
    a.n_index = n_index; a.B = batch; a.max_len = max_len; a.k = k; a.max_occ = max_occ; a.cap = anchors_per_read;
    hipLaunchKernelGGL(read_seeds_kernel, dim3(batch), dim3(256), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "read_seeds");
    return WN_OK;
}

int wn_chain(const long long* keys, const int* n_anchors, const int* lengths, int batch, int max_len, int anchors_per_read, int k, int h,
             int max_dist, int bandwidth, int gap_base, int gap_log, int* result, int* f, int* pred, int* bad, wn_stream_t stream) {
    if (batch <= 0 || max_len <= 0) return WN_ERR_BAD_SHAPE;
    if (batch > 65535 || max_len > kRmMaxRead || anchors_per_read < 1 || anchors_per_read > kRmMaxAnchors || k < 1 || k > kRmMaxK ||
        h < 1 || h > kRmMaxH || max_dist < 1 || max_dist > kRmMaxDist || bandwidth < 1 || bandwidth > kRmMaxDist || gap_base < 0 ||
        gap_base > kRmMaxGap || gap_log < 0 || gap_log > kRmMaxGap)
        return WN_ERR_UNSUPPORTED;
    if (!keys || !n_anchors || !lengths || !result || (f == nullptr) != (pred == nullptr)) return WN_ERR_NULL;
    ChainArgs a = {};
    a.keys = keys; a.n_anchors = n_anchors; a.lengths = lengths; a.result = result; a.f = f; a.pred = pred; a.bad = bad;
    a.B = batch; a.max_len = max_len; a.cap = anchors_per_read; a.k = k; a.h = h;
    a.ring = 64;
    while (a.ring < h) a.ring <<= 1;
    a.max_dist = max_dist; a.bandwidth = bandwidth; a.gap_base = gap_base; a.gap_log = gap_log;
    const size_t lds = (size_t)2 * 24 * a.ring;                          // two waves, 24 bytes a slot: at most 48 KiB
    hipLaunchKernelGGL(chain_kernel, dim3(batch), dim3(128), lds, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "chain");
    return WN_OK;
}
