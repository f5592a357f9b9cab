// Banded global pairwise alignment of two label sequences with affine gaps on the device: the recurrence,
// tie rules, end-cell rule and op rows of wn_pairalign.hip, restricted per pair to the stripe of diagonals
// diag_lo <= j - i <= diag_hi.  Work and workspace go with (N + M) * width instead of N * M.
//
//   band_align_kernel<multi>   one workgroup per pair, three phases in one launch.  `a` is the reference (rows i), `b` the query
//                              (columns j); a cell is IN BAND iff diag_lo <= j - i <= diag_hi, and H / E / F of a cell that is not
//                              are -infinity wherever they are read.
//
//     fill      in the coordinates s = i + j (the step), d = j - i (the diagonal): cell (s, d) takes E from (s - 1, d - 1), F from
//               (s - 1, d + 1) and the diagonal from (s - 2, d).  Every thread owns 8 CONSECUTIVE diagonals (d = lo + 8 tid + c)
//               and keeps their newest H, E and F in registers; at step s the cells whose d has the parity of s are active, they
//               read only inactive neighbours, so the update is in place and there is no chain along a row.  Of a thread's four
//               active cells one reads a neighbour thread: c = 0 its left neighbour's (H, E) on even steps of the stripe, c = 7
//               its right neighbour's (H, F) on odd ones -- inside a wave one DPP wavefront shift each way (wave_shr1 / wave_shl1),
//               across waves a double-buffered LDS slot and one workgroup barrier per step.  Widths <= 512 run in ONE wave: that
//               instantiation has no barrier in its step.  A diagonal starts at step |d| with the full matrix's border value (0 with free
//               end gaps, else -(go + ge (|d| - 1))), whether or not (0, 0) is in band.  Both label rows pass through LDS rings filled
//               in chunks (kRing / kFill below): the labels a step reads span at most width / 2 + 1 entries of either.  The four
//               4-bit backpointers of a thread and step (2 bits H's choice, 1 bit E, 1 bit F) are ONE 16-bit word, stored as
//               bp[step][thread]: a wave's store is contiguous.  Steps before the stripe's first cell and after its last are skipped.
//     end cell  every diagonal of the stripe ends on the last row or the last column, so after the last step the candidates sit
//               in the owners' registers.  (N, M); with free end gaps (N, M), then the last row from j = M - 1 down, then the last
//               column from i = N - 1 down, in-band cells only, a later one replacing an earlier one only if strictly greater: one
//               64-bit LDS atomic max over (score, -rank in that order).
//     trace     the H / E / F state machine back from the end cell until i == 0 or j == 0, in chunks of 64 lookups: a lookup moves
//               at most two steps and one diagonal, so all threads load the 128 steps x 18 threads of backpointer words a chunk can
//               touch into LDS and one lane walks them there; a lookup that enters E or F makes that state's move at once.  The
//               ops go back to front into the workspace; then all threads write the row front to back: head end gaps, the path,
//               tail end gaps, zero padding.  The same lane counts edge_hits.
//
// No alignment (status 0, not an error): with free end gaps the stripe misses the rectangle (diag_lo > M or diag_hi < -N), with
// penalised ones (N, M) is not in band.  Every other in-band cell is reachable through the border cell of its own diagonal.
// -infinity is -2^30 and every "- ge" on a value that may be the sentinel is clamped back to it; real scores stay within
// 131070 * 1024 < 2^27.  All results leave through ordinary vector stores.  The score-only form stores no backpointers.
#include <climits>

#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"
#include "wn_wave_dev.h"

namespace wn {

constexpr int kBaPer = 8;                // consecutive diagonals per thread
constexpr int kBaMaxBand = 2048;         // diagonals of a stripe: 256 threads
constexpr int kBaMaxLen = 65535;         // labels of either sequence
constexpr int kBaChunk = 64;             // backpointer lookups of the trace per LDS window
constexpr int kBaWinSteps = 2 * kBaChunk;                            // steps a chunk can touch: 128
constexpr int kBaWinWords = (2 * kBaChunk + 1 + kBaPer - 1) / kBaPer + 1;       // threads' words over 129 diagonals: 18
constexpr int kBaNeg = -(1 << 30);       // -infinity
constexpr int kBaBias = 1 << 30;         // makes a score a non-negative sort key
constexpr int kBaRankBits = 17;          // an end cell's place in the scan order: 0 .. N + M <= 131070
constexpr int kBaRankMask = (1 << kBaRankBits) - 1;

struct BandAlignArgs {
    const int* ref;                      // [B] rows of ref_stride elements
    const int* query;
    long long ref_stride, query_stride;
    const int *ref_len, *query_len;      // [B]
    const int *diag_lo, *diag_hi;        // [B]
    int* score;                          // [B]
    int* stats;                          // [B][4] or nullptr
    unsigned char* ops;                  // [B][N + M] or nullptr
    int* ops_len;                        // [B] or nullptr
    signed char* status;                 // [B]
    int* edge_hits;                      // [B] or nullptr
    unsigned short* bp;                  // [B][N + M + 1][T] or nullptr (score only)
    unsigned char* rev;                  // [B][round_up(N + M, 16)]: the path's ops, back to front
    int* bad;
    int N, M;
    int max_band, match, mismatch, go, ge, free_ends;
};

template <bool kMulti>
__global__ __launch_bounds__(kMulti ? kBaMaxBand / kBaPer : 64) void band_align_kernel(const BandAlignArgs a) {
    constexpr int kWaves = kMulti ? kBaMaxBand / kBaPer / 64 : 1;
    constexpr int kRing = kMulti ? 4096 : 1024;                          // labels of either row in LDS
    constexpr int kFill = kMulti ? 1024 : 512;                           // and the chunk they are refilled by
    static_assert(kBaPer * 64 * kWaves / 2 + 1 + kFill <= kRing, "a chunk must not overwrite labels a step still reads");
    __shared__ int ring_a[kRing], ring_b[kRing];
    __shared__ int2 edge_l[2][kWaves], edge_r[2][kWaves];                // (H, E) of a wave's last diagonal, (H, F) of its first
    __shared__ unsigned long long end_key;                               // (score + bias) << 17 | (2^17 - 1 - rank)
    __shared__ unsigned short win[kBaWinSteps * kBaWinWords];            // the trace's backpointer window
    __shared__ int wa[kBaChunk], wb[kBaChunk];                           // and the labels under it, back to front
    __shared__ unsigned char wops[kBaChunk];
    __shared__ int cur[3], fin[3];                                       // the walker's cell and op count; matches, mismatches, hits
    const int p = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int go = a.go, ge = a.ge;
    const bool free_ends = a.free_ends != 0;
    int Nb = a.ref_len[p], Mb = a.query_len[p];
    const int dlo = a.diag_lo[p], dhi = a.diag_hi[p];
    const bool poisoned = Nb < 0 || Nb > a.N || Mb < 0 || Mb > a.M || dlo > dhi || (long long)dhi - dlo + 1 > a.max_band;
    if (poisoned) { Nb = 0; Mb = 0; }                                    // no bad value is ever used as an index
    const int lo = poisoned ? 0 : max(dlo, -Nb), hi = poisoned ? 0 : min(dhi, Mb);       // the diagonals that meet the rectangle
    const int corner = Mb - Nb;
    const bool none = free_ends ? lo > hi : (dlo > corner || dhi < corner);
    const int P = a.N + a.M;
    unsigned char* ops = a.ops ? a.ops + (long long)p * P : nullptr;
    if (poisoned || none) {
        if (tid == 0) {
            a.score[p] = INT_MIN;
            a.status[p] = poisoned ? -1 : 0;
            if (a.edge_hits) a.edge_hits[p] = poisoned ? -1 : 0;
            if (a.ops_len) a.ops_len[p] = 0;
            if (poisoned && a.bad) atomicAdd(a.bad, 1);
        }
        if (tid < 4 && a.stats) a.stats[(long long)p * 4 + tid] = poisoned ? -1 : 0;
        for (int q = tid; ops && q < P; q += nthr) ops[q] = 0;
        return;
    }
    const int* ar = a.ref + (long long)p * a.ref_stride;
    const int* bq = a.query + (long long)p * a.query_stride;
    const int T = (a.max_band + kBaPer - 1) / kBaPer;                    // threads that own a diagonal of the widest stripe
    unsigned short* bprow = a.bp ? a.bp + (long long)p * (P + 1) * T : nullptr;

    // border(k): H[k][0] = H[0][k]
    auto border = [&](int k) { return (free_ends || k == 0) ? 0 : -(go + ge * (k - 1)); };
    const int d0 = lo + kBaPer * tid;                                    // this thread's first diagonal
    int H[kBaPer], E[kBaPer], F[kBaPer];
    int first[kBaPer];                                                   // diagonal d has its border cell at step |d| and inner cells at
    unsigned inner[kBaPer];                                              // the steps of its parity in (|d|, min(2 M - d, 2 N + d)]
#pragma unroll
    for (int c = 0; c < kBaPer; ++c) {
        H[c] = kBaNeg; E[c] = kBaNeg; F[c] = kBaNeg;
        const int d = d0 + c, ad = d < 0 ? -d : d;
        first[c] = d <= hi ? ad + 1 : INT_MAX;                           // a diagonal past the stripe never starts
        inner[c] = d <= hi ? (unsigned)(min(2 * Mb - d, 2 * Nb + d) - ad) : 0u;
    }
    if (tid == 0) { end_key = 0ull; a.status[p] = 1; }                  // every other pair has an alignment
    if (kMulti && lane == 0) {
        edge_l[0][wave] = edge_l[1][wave] = make_int2(kBaNeg, kBaNeg);
        edge_r[0][wave] = edge_r[1][wave] = make_int2(kBaNeg, kBaNeg);
    }
    // the first step with a cell of the stripe, and the last: the end of the diagonal nearest the corner
    const int s_first = lo > 0 ? lo : (hi < 0 ? -hi : 0);
    const int dc = min(max(corner, lo), hi);
    const int s_last = min(2 * Mb - dc, 2 * Nb + dc);
    // the label rings hold [end - kRing, end); a step reads reference labels up to ((s - lo) >> 1) - 1 and query labels up to
    // ((s + hi) >> 1) - 1, and none more than width / 2 + 1 below those
    int end_a = max(((s_first - hi) >> 1) - 1, 0) / kFill * kFill, end_b = max(((s_first + lo) >> 1) - 1, 0) / kFill * kFill;
    __syncthreads();

    for (int s = s_first; s <= s_last; ++s) {
        const int need_a = ((s - lo) >> 1) - 1, need_b = ((s + hi) >> 1) - 1;
        if (need_a >= end_a || need_b >= end_b) {                        // uniform: everybody has finished the step before
            while (need_a >= end_a) {
                for (int x = tid; x < kFill; x += nthr) ring_a[(end_a + x) & (kRing - 1)] = end_a + x < Nb ? ar[end_a + x] : 0;
                end_a += kFill;
            }
            while (need_b >= end_b) {
                for (int x = tid; x < kFill; x += nthr) ring_b[(end_b + x) & (kRing - 1)] = end_b + x < Mb ? bq[end_b + x] : 0;
                end_b += kFill;
            }
            __syncthreads();
        }
        unsigned nibs = 0;
        // the cells c = par, par + 2, par + 4, par + 6 of every thread: those whose diagonal has the parity of s
        auto step = [&](auto par_c) {
            constexpr int par = decltype(par_c)::value;
            int hn, xn;                                                  // the neighbour thread's (H, E) or (H, F)
            if constexpr (par == 0) {
                hn = wave_shr1(H[kBaPer - 1], kBaNeg), xn = wave_shr1(E[kBaPer - 1], kBaNeg);
                if (kMulti && lane == 0 && wave > 0) { const int2 v = edge_l[(s - 1) & 1][wave - 1]; hn = v.x; xn = v.y; }
            } else {
                hn = wave_shl1(H[0], kBaNeg), xn = wave_shl1(F[0], kBaNeg);
                if (kMulti && lane == 63 && wave < kWaves - 1) { const int2 v = edge_r[(s - 1) & 1][wave + 1]; hn = v.x; xn = v.y; }
            }
#pragma unroll
            for (int k = 0; k < kBaPer / 2; ++k) {
                const int c = par + 2 * k, d = d0 + c;
                const int i = (s - d) >> 1, j = (s + d) >> 1;
                const bool live = (unsigned)(s - first[c]) < inner[c];   // an inner cell: 1 <= i <= N, 1 <= j <= M
                // a cell that is not live reads whatever the masked index holds (LDS not yet filled, too): its result is dropped
                const int ai = ring_a[(i - 1) & (kRing - 1)], bj = ring_b[(j - 1) & (kRing - 1)];
                const int hl = c == 0 ? hn : H[c == 0 ? 0 : c - 1], el = c == 0 ? xn : E[c == 0 ? 0 : c - 1];
                const int hu = c == kBaPer - 1 ? hn : H[c == kBaPer - 1 ? c : c + 1], fu = c == kBaPer - 1 ? xn : F[c == kBaPer - 1 ? c : c + 1];
                const int eo = hl - go, ee = max(el - ge, kBaNeg);
                const int fo = hu - go, fe = max(fu - ge, kBaNeg);
                const int e = max(eo, ee), f = max(fo, fe);
                unsigned bits = (ee > eo ? 4u : 0u) | (fe > fo ? 8u : 0u);
                int h = H[c] + (ai == bj ? a.match : a.mismatch);
                if (e > h) { h = e; bits |= 1u; }
                if (f > h) { h = f; bits = (bits & ~3u) | 2u; }
                if (live) { H[c] = h; E[c] = e; F[c] = f; nibs |= bits << (4 * k); }
                if (s + 1 == first[c]) H[c] = border(s);                 // the diagonal's border cell; its E and F are -infinity still
            }
        };
        if (((s ^ lo) & 1) == 0) step(std::integral_constant<int, 0>());
        else step(std::integral_constant<int, 1>());
        if (bprow && tid < T) bprow[(long long)s * T + tid] = (unsigned short)nibs;
        if (kMulti) {
            if (lane == 63) edge_l[s & 1][wave] = make_int2(H[kBaPer - 1], E[kBaPer - 1]);
            if (lane == 0) edge_r[s & 1][wave] = make_int2(H[0], F[0]);
            __syncthreads();                                             // one barrier per step: the slots of step s - 1 are free again
        }
    }
    __syncthreads();                                                     // end_key initialised, backpointers visible

    // the end cell: every diagonal's last cell sits in its owner's registers
    {
        unsigned long long key = 0ull;
#pragma unroll
        for (int c = 0; c < kBaPer; ++c) {
            const int d = d0 + c;
            const int rank = d == corner ? 0 : (d < corner ? corner - d : Nb + d);
            if (d <= hi && (free_ends || d == corner))
                key = max(key, ((unsigned long long)(unsigned)(H[c] + kBaBias) << kBaRankBits) | (unsigned)(kBaRankMask - rank));
        }
        if (key) atomicMax(&end_key, key);                               // the first in the scan order among equals
    }
    __syncthreads();
    const int score = (int)(unsigned)(end_key >> kBaRankBits) - kBaBias, rank = kBaRankMask - (int)(end_key & kBaRankMask);
    const int ie = rank <= Mb ? Nb : Nb + Mb - rank, je = rank <= Mb ? Mb - rank : Mb;
    if (tid == 0) a.score[p] = score;
    if (!a.bp) return;                                                   // score only

    unsigned char* rev = a.rev + (long long)p * ((P + 15) / 16 * 16);
    // chunks of 64 backpointer lookups.  A lookup moves at most two steps and one diagonal, so a chunk that starts in cell (s0, e0)
    // stays in steps (s0 - 128, s0] and diagonals [e0 - 64, e0 + 64]: 18 threads' words of 128 steps, loaded into LDS by all
    // threads with the 64 reference and query labels it can meet; one lane walks them there
    int i0 = ie, j0 = je, np = 0;
    int st = 0, nmatch = 0, ndiag = 0;                                   // thread 0's: the state, matches, diagonal ops
    int hits = (je - ie == dlo || je - ie == dhi) ? 1 : 0;               // the end cell is the path's last
    while (i0 > 0 && j0 > 0) {
        const int sbase = i0 + j0 - (kBaWinSteps - 1), tlo = (j0 - i0 - kBaChunk - lo) >> 3;
        // rows of skipped steps are workspace nobody wrote: they are loaded like the rest, and the walker never looks at them
        for (int x = tid; x < kBaWinSteps * kBaWinWords; x += nthr) {
            const int s = sbase + x / kBaWinWords, t = tlo + x % kBaWinWords;
            win[x] = (s >= 0 && t >= 0 && t < T) ? bprow[(long long)s * T + t] : (unsigned short)0;       // s <= i0 + j0: a row of this pair
        }
        for (int x = tid; x < kBaChunk; x += nthr) {
            wa[x] = i0 - 1 - x >= 0 ? ar[i0 - 1 - x] : 0;
            wb[x] = j0 - 1 - x >= 0 ? bq[j0 - 1 - x] : 0;
        }
        __syncthreads();                                                 // window loaded; the previous chunk's ops were read
        if (tid == 0) {
            int i = i0, j = j0, n = 0;
            for (int look = 0; look < kBaChunk && i > 0 && j > 0; ++look) {
                const int x = j - i - lo, t = x >> 3, k = (x & (kBaPer - 1)) >> 1;
                const unsigned nib = ((unsigned)win[(i + j - sbase) * kBaWinWords + (t - tlo)] >> (4 * k)) & 15u;
                // selects, no branches: wn_pairalign.hip's state machine, but a lookup that enters E or F moves at once
                if (st == 0) st = (int)(nib & 3u);                       // into E or F at the same cell: its nibble says how it goes on
                const bool dg = st == 0, eg = st == 1;                   // every lookup moves: selects, no branches
                const bool same = wa[i0 - i] == wb[j0 - j];
                const int op = dg ? (same ? 1 : 2) : (eg ? 4 : 3);
                nmatch += (dg && same) ? 1 : 0;
                ndiag += dg ? 1 : 0;
                st = dg ? 0 : (eg ? ((nib & 4u) ? 1 : 0) : ((nib & 8u) ? 2 : 0));
                i -= (dg || !eg) ? 1 : 0;
                j -= (dg || eg) ? 1 : 0;
                hits += (j - i == dlo || j - i == dhi) ? 1 : 0;
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
    if (tid == 0) { fin[0] = nmatch; fin[1] = ndiag - nmatch; fin[2] = hits; }
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
        if (a.edge_hits) a.edge_hits[p] = fin[2];
        if (a.stats) {
            int* s = a.stats + (long long)p * 4;
            s[0] = fin[0]; s[1] = fin[1]; s[2] = len - fin[0] - fin[1]; s[3] = len;
        }
    }
}

}  // namespace wn

using namespace wn;

static int check_band_align(int batch, int max_ref_len, int max_query_len, int max_band) {
    if (batch <= 0 || max_ref_len <= 0 || max_query_len <= 0 || max_band <= 0) return WN_ERR_BAD_SHAPE;
    if (max_band > kBaMaxBand) return WN_ERR_UNSUPPORTED;
    if (max_ref_len > kBaMaxLen) return WN_ERR_UNSUPPORTED;
    if (max_query_len > kBaMaxLen) return WN_ERR_UNSUPPORTED;
    if (batch > 65535) return WN_ERR_UNSUPPORTED;
    return WN_OK;
}
static size_t ba_threads(int max_band) { return (size_t)(max_band + kBaPer - 1) / kBaPer; }
static size_t ba_rev_stride(int max_ref_len, int max_query_len) { return ((size_t)max_ref_len + max_query_len + 15) / 16 * 16; }
static size_t ba_bp_bytes(int batch, int max_ref_len, int max_query_len, int max_band) {
    return (size_t)batch * ((size_t)max_ref_len + max_query_len + 1) * ba_threads(max_band) * sizeof(unsigned short);
}

// workspace: one 16-bit word of backpointers per thread and step, [B][N + M + 1][T] with T = ceil(max_band / 8), rounded up to 16
// bytes, then the path's ops back to front, [B][round_up(N + M, 16)] bytes
size_t wn_banded_align_workspace_bytes(int batch, int max_ref_len, int max_query_len, int max_band) {
    if (check_band_align(batch, max_ref_len, max_query_len, max_band) != WN_OK) return 0;
    return (ba_bp_bytes(batch, max_ref_len, max_query_len, max_band) + 15) / 16 * 16 +
           (size_t)batch * ba_rev_stride(max_ref_len, max_query_len);
}

int wn_banded_align(const int* ref, long long ref_stride, const int* ref_lengths, const int* query, long long query_stride,
                    const int* query_lengths, const int* diag_lo, const int* diag_hi, int batch, int max_ref_len, int max_query_len,
                    int max_band, int match, int mismatch, int gap_open, int gap_extend, int end_gaps_free, int* score, int* stats,
                    unsigned char* ops, int* ops_len, signed char* status, int* edge_hits, void* workspace, size_t workspace_bytes,
                    int* bad, wn_stream_t stream) {
    const int rc = check_band_align(batch, max_ref_len, max_query_len, max_band);
    if (rc != WN_OK) return rc;
    if (const int s = check_affine_costs(match, mismatch, gap_open, gap_extend)) return s;
    const bool trace = ops || stats;
    if (!ref || !ref_lengths || !query || !query_lengths || !diag_lo || !diag_hi || !score || !status ||
        (ops != nullptr) != (ops_len != nullptr) || (!trace && edge_hits))
        return WN_ERR_NULL;
    if (trace) {
        if (!workspace) return WN_ERR_NULL;
        if (workspace_bytes < wn_banded_align_workspace_bytes(batch, max_ref_len, max_query_len, max_band)) return WN_ERR_WORKSPACE;
        if (reinterpret_cast<uintptr_t>(workspace) & 15) return WN_ERR_WORKSPACE;
    }
    BandAlignArgs a = {};
    a.ref = ref; a.query = query; a.ref_stride = ref_stride; a.query_stride = query_stride;
    a.ref_len = ref_lengths; a.query_len = query_lengths; a.diag_lo = diag_lo; a.diag_hi = diag_hi;
    a.score = score; a.stats = stats; a.ops = ops; a.ops_len = ops_len; a.status = status; a.edge_hits = edge_hits; a.bad = bad;
    a.N = max_ref_len; a.M = max_query_len; a.max_band = max_band;
    a.match = match; a.mismatch = mismatch; a.go = gap_open; a.ge = gap_extend; a.free_ends = end_gaps_free ? 1 : 0;
    if (trace) {
        a.bp = reinterpret_cast<unsigned short*>(workspace);
        a.rev = reinterpret_cast<unsigned char*>(workspace) + (ba_bp_bytes(batch, max_ref_len, max_query_len, max_band) + 15) / 16 * 16;
    }
    hipStream_t s = (hipStream_t)stream;
    if (ba_threads(max_band) <= 64) hipLaunchKernelGGL(band_align_kernel<false>, dim3(batch), dim3(64), 0, s, a);      // one wave, no barrier per step
    else hipLaunchKernelGGL(band_align_kernel<true>, dim3(batch), dim3(kBaMaxBand / kBaPer), 0, s, a);
    WN_HIP(hipGetLastError(), "banded_align");
    return WN_OK;
}
