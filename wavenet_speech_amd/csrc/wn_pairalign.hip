// Global pairwise alignment of two label sequences with affine gaps on the device (Needleman-Wunsch / Gotoh): how good is a
// decoded read?  The step the reference's evaluation notebook hands to EMBOSS needle after decoding: score, identity /
// mismatch / gap counts and the alignment itself.  With unit costs the same kernel gives the Levenshtein edit distance.
// The inputs are the decoders' label rows (wn_decode.hip) and the targets as wn_ctc_align takes them, read in place.
//
//   pair_align_kernel<multi>   one workgroup per pair, three phases in one launch.  `a` is the reference (rows i = 1..N), `b`
//                              the query (columns j = 1..M); a gap of length n costs gap_open + (n - 1) gap_extend.
//
//     fill      E[i][j] = max(H[i][j-1] - go, E[i][j-1] - ge)      a column of b against a gap
//               F[i][j] = max(H[i-1][j] - go, F[i-1][j] - ge)      a row of a against a gap
//               H[i][j] = best of  H[i-1][j-1] + (a[i-1] == b[j-1] ? match : mismatch),  E[i][j],  F[i][j]
//               in int32: every sum is exact.  A systolic wavefront as in ctc_align_kernel: every thread owns 8 CONSECUTIVE
//               columns (j = 8 tid + 1 .. 8 tid + 8) and keeps their H and F of the previous row in registers; at step k thread
//               t does row k - t + 1.  E runs along the row, so exactly one (H, E) pair -- the thread's last column -- crosses
//               to the right neighbour per step, and the pair received one step earlier holds the diagonal H.  Inside a wave
//               that is a DPP wavefront shift; across waves a double-buffered LDS slot and one workgroup barrier per step.  Up
//               to 512 columns run in ONE wave: that instantiation has no barrier in its step.  The reference rows are staged
//               1024 at a time in a 2048-entry LDS ring (thread t reads row k - t, at most 1023 behind the newest).  The eight
//               4-bit backpointers of a thread and step (2 bits H's choice, 1 bit E, 1 bit F) are ONE dword, stored in the
//               skewed order bp[step][thread]: a wave's store is contiguous.
//     end cell  (N, M); with free end gaps the best of (N, M), then the last row from j = M down, then the last column from
//               i = N down, a later cell replacing an earlier one only if strictly greater.  The last row is in the threads'
//               registers after the last step (one 64-bit LDS atomic max over score and column); the owner of column M tracks
//               the last column while the rows go by.
//     trace     the H / E / F state machine back from the end cell until i == 0 or j == 0, in chunks of 64 lookups: a lookup
//               moves at most one row and one column, so all threads load the 72 steps x 9 threads of backpointer words a chunk
//               can touch into LDS and one lane walks them there (no chain of dependent global loads), as ctc_align_kernel
//               does.  The ops go back to front into the workspace; then all threads write the row front to back: head end
//               gaps, the path, tail end gaps, zero padding.
//
// Ties (part of the contract, tests/pairwise_align_ref.py holds the same rule): opening a gap wins over extending one on
// equality (bit 0 = opened, 1 = extended); H tries diagonal, E, F in that order and a later one replaces an earlier one only
// if strictly greater.  -infinity is -2^30 and every "- ge" on a value that may be the sentinel is clamped back to it, so it can
// neither wrap nor come near a real score (|scores| <= (65535 + 8192) * 1024 < 2^27).  All results leave through ordinary
// vector stores.  The score-only form (no ops, no stats) stores no backpointers and needs no workspace.
#include <climits>

#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"
#include "wn_wave_dev.h"

namespace wn {

constexpr int kPaPer = 8;                // consecutive query columns per thread
constexpr int kPaMaxThreads = 1024;      // 8192 columns
static_assert(kPaMaxQuery == kPaPer * kPaMaxThreads);            // the limits themselves: wn_host.h
constexpr int kPaRing = 2048;            // reference rows in LDS: two halves of 1024, loaded alternately
constexpr int kPaChunk = 64;             // backpointer lookups of the trace per LDS window
constexpr int kPaWinThreads = kPaChunk / kPaPer + 1;             // threads' words a chunk can touch: 9
constexpr int kPaWinSteps = kPaChunk + kPaWinThreads - 1;        // steps (skewed rows) it can touch: 72
constexpr int kPaNeg = -(1 << 30);       // -infinity
constexpr int kPaBias = 1 << 30;         // makes a score a non-negative sort key

struct PairAlignArgs {
    const int* ref;                      // [B] rows of ref_stride elements
    const int* query;
    long long ref_stride, query_stride;
    const int* ref_len;                  // [B]
    const int* query_len;                // [B]
    int* score;                          // [B]
    int* stats;                          // [B][4] or nullptr
    unsigned char* ops;                  // [B][N + M] or nullptr
    int* ops_len;                        // [B] or nullptr
    unsigned* bp;                        // [B][N + W - 1][W] or nullptr (score only)
    unsigned char* rev;                  // [B][rev_stride]: the path's ops, back to front
    long long rev_stride;
    int* bad;
    int B, N, M, W;                      // W = threads that own a column of the widest query
    int match, mismatch, go, ge, free_ends;
};

template <bool kMulti>
__global__ __launch_bounds__(kMulti ? kPaMaxThreads : 64) void pair_align_kernel(const PairAlignArgs a) {
    __shared__ int ring[kPaRing];
    __shared__ int2 edge[2][kPaMaxThreads / 64];                         // (H, E) of every wave's last column, by step parity
    __shared__ unsigned long long row_key;                               // best of the last row: (score + bias) << 16 | column
    __shared__ int col_best[2];                                          // best of the last column and its row
    __shared__ unsigned win[kPaWinSteps * kPaWinThreads];                // the trace's backpointer window
    __shared__ int wa[kPaChunk], wb[kPaChunk];                           // and the labels under it, back to front
    __shared__ unsigned char wops[kPaChunk];
    __shared__ int cur[3], fin[2];                                       // the walker's cell and op count; matches, mismatches
    const int p = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int go = a.go, ge = a.ge;
    const bool free_ends = a.free_ends != 0;
    int Nb = a.ref_len[p], Mb = a.query_len[p];
    const bool poisoned = Nb < 0 || Nb > a.N || Mb < 0 || Mb > a.M;
    if (poisoned) { Nb = 0; Mb = 0; }                                    // the lengths are never used as an index
    const int* ar = a.ref + (long long)p * a.ref_stride;
    const int* bq = a.query + (long long)p * a.query_stride;
    const int nact = (Mb + kPaPer - 1) / kPaPer;                         // threads that own a column of this query
    const int nsteps = (Nb > 0 && nact > 0) ? Nb + nact - 1 : 0;
    const int tM = Mb > 0 ? (Mb - 1) / kPaPer : -1, cM = Mb > 0 ? (Mb - 1) % kPaPer : 0;   // the owner of column M
    if (tid == 0) { row_key = 0ull; col_best[0] = 0; col_best[1] = 0; }

    // border(k): H[k][0] = H[0][k]
    auto border = [&](int k) { return (free_ends || k == 0) ? 0 : -(go + ge * (k - 1)); };
    int qb[kPaPer], H[kPaPer], F[kPaPer];
#pragma unroll
    for (int c = 0; c < kPaPer; ++c) {
        const int j = kPaPer * tid + c + 1;
        qb[c] = j <= Mb ? bq[j - 1] : 0;                                 // columns past M compute values nobody reads
        H[c] = border(min(j, Mb + 1));
        F[c] = kPaNeg;
    }
    int diag = border(min(kPaPer * tid, Mb + 1));                        // H[i-1][8 tid]
    int send_h = 0, send_e = kPaNeg;
    int cbest = 0, cbest_i = 0;                                          // free end gaps: H[0][M] = 0
    unsigned* bprow = a.bp ? a.bp + (long long)p * (a.N + a.W - 1) * a.W : nullptr;

    for (int k = 0; k < nsteps; ++k) {
        if ((k & (kPaRing / 2 - 1)) == 0) {                              // rows [k, k + 1024): the half nobody reads any more
            for (int i = tid; i < kPaRing / 2; i += nthr) ring[(k + i) & (kPaRing - 1)] = k + i < Nb ? ar[k + i] : 0;
            __syncthreads();
        }
        int hl = wave_shr1(send_h, 0), el = wave_shr1(send_e, kPaNeg);
        if (kMulti && lane == 0 && wave > 0) { const int2 v = edge_left(edge, k, wave); hl = v.x; el = v.y; }
        if (tid == 0) { hl = border(k + 1); el = kPaNeg; }
        const int row = k - tid;                                         // this step's row is i = row + 1
        if (row >= 0 && row < Nb && tid < nact) {
            const int ai = ring[row & (kPaRing - 1)];
            int hd = diag, hleft = hl, eleft = el;
            unsigned bpw = 0;
#pragma unroll
            for (int c = 0; c < kPaPer; ++c) {
                const int eo = hleft - go, ee = max(eleft - ge, kPaNeg);
                const int fo = H[c] - go, fe = max(F[c] - ge, kPaNeg);
                const int e = max(eo, ee), f = max(fo, fe);
                unsigned bits = (ee > eo ? 4u : 0u) | (fe > fo ? 8u : 0u);
                int h = hd + (ai == qb[c] ? a.match : a.mismatch);
                if (e > h) { h = e; bits |= 1u; }
                if (f > h) { h = f; bits = (bits & ~3u) | 2u; }
                bpw |= bits << (4 * c);
                hd = H[c];
                H[c] = h; F[c] = f;
                hleft = h; eleft = e;
            }
            diag = hl;
            send_h = hleft; send_e = eleft;
            if (bprow) bprow[(long long)k * a.W + tid] = bpw;
            if (free_ends && tid == tM) {
                int hm = H[0];
#pragma unroll
                for (int c = 1; c < kPaPer; ++c) hm = c == cM ? H[c] : hm;
                if (hm >= cbest) { cbest = hm; cbest_i = row + 1; }      // the largest row among equals
            }
        }
        if (kMulti) {
            edge_publish(edge, k, lane, wave, make_int2(send_h, send_e));
            __syncthreads();                                             // one barrier per step: the slot of step k-1 is free again
        }
    }
    __syncthreads();                                                     // row_key / col_best initialised, backpointers visible

    // the end cell: the last row sits in the registers (row 0, the border, when there are no rows or no columns)
    {
        unsigned long long key = 0ull;
#pragma unroll
        for (int c = 0; c < kPaPer; ++c) {
            const int j = kPaPer * tid + c + 1;
            if (j <= Mb && (free_ends || j == Mb)) key = max(key, ((unsigned long long)(unsigned)(H[c] + kPaBias) << 16) | (unsigned)j);
        }
        if (tid == 0 && (free_ends || Mb == 0)) key = max(key, (unsigned long long)(unsigned)(border(Nb) + kPaBias) << 16);
        if (key) atomicMax(&row_key, key);                               // the largest column among equals
        if (free_ends && tid == tM) { col_best[0] = cbest; col_best[1] = cbest_i; }
    }
    __syncthreads();
    int score = (int)(unsigned)(row_key >> 16) - kPaBias, ie = Nb, je = (int)(row_key & 0xffffull);
    if (free_ends && Mb > 0 && col_best[0] > score) { score = col_best[0]; ie = col_best[1]; je = Mb; }
    if (tid == 0) {
        a.score[p] = poisoned ? INT_MIN : score;
        if (poisoned && a.bad) atomicAdd(a.bad, 1);
    }
    if (!a.bp) return;                                                   // score only

    const int P = a.N + a.M;
    unsigned char* ops = a.ops ? a.ops + (long long)p * P : nullptr;
    if (poisoned) {
        for (int q = tid; ops && q < P; q += nthr) ops[q] = 0;
        if (tid == 0 && a.ops_len) a.ops_len[p] = 0;
        if (tid < 4 && a.stats) a.stats[(long long)p * 4 + tid] = -1;
        return;
    }
    unsigned char* rev = a.rev + (long long)p * a.rev_stride;
    // chunks of 64 backpointer lookups.  A lookup moves at most one row and one column, so a chunk that starts in cell (i0, j0)
    // stays in rows (i0 - 64, i0] and columns (j0 - 64, j0]: 9 threads' words of 72 steps in the skewed order, loaded into LDS by
    // all threads with the 64 reference and query labels it can meet; one lane walks them in LDS (no chain of dependent
    // global loads) and the threads write the chunk's ops out
    int i0 = ie, j0 = je, np = 0;
    int st = 0, nmatch = 0, nmis = 0;                                    // thread 0's
    while (i0 > 0 && j0 > 0) {
        const int tj = (j0 - 1) / kPaPer, kbase = (i0 - 1) + tj - (kPaWinSteps - 1), tbase = tj - (kPaWinThreads - 1);
        for (int x = tid; x < kPaWinSteps * kPaWinThreads; x += nthr) {
            const int k = kbase + x / kPaWinThreads, t = tbase + x % kPaWinThreads;
            win[x] = (k >= 0 && t >= 0) ? bprow[(long long)k * a.W + t] : 0u;
        }
        for (int x = tid; x < kPaChunk; x += nthr) {
            wa[x] = i0 - 1 - x >= 0 ? ar[i0 - 1 - x] : 0;
            wb[x] = j0 - 1 - x >= 0 ? bq[j0 - 1 - x] : 0;
        }
        __syncthreads();                                                 // window loaded; the previous chunk's ops were read
        if (tid == 0) {
            int i = i0, j = j0, n = 0;
            for (int look = 0; look < kPaChunk && i > 0 && j > 0; ++look) {
                const int t = (j - 1) / kPaPer, c = (j - 1) % kPaPer;
                const unsigned nib = (win[(i - 1 + t - kbase) * kPaWinThreads + (t - tbase)] >> (4 * c)) & 15u;
                int op;
                if (st == 0) {
                    st = (int)(nib & 3u);
                    if (st != 0) continue;                               // into E or F at the same cell
                    const bool same = wa[i0 - i] == wb[j0 - j];
                    op = same ? 1 : 2;
                    nmatch += same; nmis += !same;
                    --i; --j;
                } else if (st == 1) {
                    op = 4; --j;
                    if (!(nib & 4u)) st = 0;
                } else {
                    op = 3; --i;
                    if (!(nib & 8u)) st = 0;
                }
                wops[n++] = (unsigned char)op;
            }
            cur[0] = i; cur[1] = j; cur[2] = n;
        }
        __syncthreads();
        const int n = cur[2];
        if (ops && tid < n) rev[np + tid] = wops[tid];                   // back to front
        np += n;
        i0 = cur[0]; j0 = cur[1];
    }
    if (tid == 0) { fin[0] = nmatch; fin[1] = nmis; }
    __syncthreads();                                                     // fin, and rev through global memory
    const int head = i0 + j0, tail = (Nb - ie) + (Mb - je), len = head + np + tail;
    const int head_op = i0 > 0 ? 3 : 4, tail_op = Nb - ie > 0 ? 3 : 4;       // at most one of each pair is not zero
    for (int q = tid; ops && q < P; q += nthr) {
        int op = 0;
        if (q < head) op = head_op;
        else if (q < head + np) op = rev[np - 1 - (q - head)];
        else if (q < len) op = tail_op;
        ops[q] = (unsigned char)op;
    }
    if (tid == 0) {
        if (a.ops_len) a.ops_len[p] = len;
        if (a.stats) {
            int* s = a.stats + (long long)p * 4;
            s[0] = fin[0]; s[1] = fin[1]; s[2] = len - fin[0] - fin[1]; s[3] = len;
        }
    }
}

}  // namespace wn

using namespace wn;

static int check_pair_align(int batch, int max_ref_len, int max_query_len) {
    if (batch <= 0 || max_ref_len <= 0 || max_query_len <= 0) return WN_ERR_BAD_SHAPE;
    if (batch > 65535 || max_ref_len > kPaMaxRef || max_query_len > kPaMaxQuery) return WN_ERR_UNSUPPORTED;
    return WN_OK;
}
static size_t pa_threads(int max_query_len) { return (size_t)(max_query_len + kPaPer - 1) / kPaPer; }
static size_t pa_rev_stride(int max_ref_len, int max_query_len) { return ((size_t)max_ref_len + max_query_len + 15) / 16 * 16; }
static size_t pa_bp_bytes(int batch, int max_ref_len, int max_query_len) {
    const size_t w = pa_threads(max_query_len);
    return (size_t)batch * ((size_t)max_ref_len + w - 1) * w * sizeof(unsigned);
}

// workspace: one dword of backpointers per thread and step, [B][N + W - 1][W] with W = ceil(M / 8), rounded up to 16 bytes, then
// the path's ops back to front, [B][round_up(N + M, 16)] bytes
size_t wn_pair_align_workspace_bytes(int batch, int max_ref_len, int max_query_len) {
    if (check_pair_align(batch, max_ref_len, max_query_len) != WN_OK) return 0;
    return (pa_bp_bytes(batch, max_ref_len, max_query_len) + 15) / 16 * 16 + (size_t)batch * pa_rev_stride(max_ref_len, max_query_len);
}

int wn_pair_align(const int* ref, long long ref_stride, const int* ref_lengths, const int* query, long long query_stride,
                  const int* query_lengths, int batch, int max_ref_len, int max_query_len, int match, int mismatch, int gap_open,
                  int gap_extend, int end_gaps_free, int* score, int* stats, unsigned char* ops, int* ops_len, void* workspace,
                  size_t workspace_bytes, int* bad, wn_stream_t stream) {
    const int rc = check_pair_align(batch, max_ref_len, max_query_len);
    if (rc != WN_OK) return rc;
    if (const int s = check_affine_costs(match, mismatch, gap_open, gap_extend)) return s;
    if (!ref || !ref_lengths || !query || !query_lengths || !score || (ops != nullptr) != (ops_len != nullptr)) return WN_ERR_NULL;
    const bool trace = ops || stats;
    if (trace) {
        if (!workspace) return WN_ERR_NULL;
        if (workspace_bytes < wn_pair_align_workspace_bytes(batch, max_ref_len, max_query_len)) return WN_ERR_WORKSPACE;
        if (reinterpret_cast<uintptr_t>(workspace) & 15) return WN_ERR_WORKSPACE;
    }
    PairAlignArgs a = {};
    a.ref = ref; a.query = query; a.ref_stride = ref_stride; a.query_stride = query_stride;
    a.ref_len = ref_lengths; a.query_len = query_lengths;
    a.score = score; a.stats = stats; a.ops = ops; a.ops_len = ops_len; a.bad = bad;
    a.B = batch; a.N = max_ref_len; a.M = max_query_len; a.W = (int)pa_threads(max_query_len);
    a.match = match; a.mismatch = mismatch; a.go = gap_open; a.ge = gap_extend; a.free_ends = end_gaps_free ? 1 : 0;
    if (trace) {
        a.bp = reinterpret_cast<unsigned*>(workspace);
        a.rev = reinterpret_cast<unsigned char*>(workspace) + (pa_bp_bytes(batch, max_ref_len, max_query_len) + 15) / 16 * 16;
        a.rev_stride = (long long)pa_rev_stride(max_ref_len, max_query_len);
    }
    const int threads = (a.W + 63) / 64 * 64;                            // 64 (one wave, no barrier per step) up to 1024
    hipStream_t s = (hipStream_t)stream;
    if (threads == 64) hipLaunchKernelGGL(pair_align_kernel<false>, dim3(batch), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(pair_align_kernel<true>, dim3(batch), dim3(threads), 0, s, a);
    WN_HIP(hipGetLastError(), "pair_align");
    return WN_OK;
}
