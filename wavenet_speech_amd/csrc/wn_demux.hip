// Barcode demultiplexing and adapter trimming of decoded reads on the device: every read's two ends against
// a table of short patterns (barcodes with their flanks, adapters), then one decision per read.  What guppy, dorado, porechop and
// qcat do right after basecalling; here the label rows of the decoders (wn_decode.hip) never leave the device for it.
//
//   demux_score_kernel<R>        SEMI-GLOBAL alignment with affine gaps of every pattern against the read's front or rear window:
//                                the pattern (rows i = 1..P) is consumed whole, its start and end in the window (columns j = 1..W)
//                                are free.  Only the score, the start and the end of the best alignment are wanted: no traceback.
//
//     cells     (score, start) pairs; every maximum is lexicographic on (score, -start), so the result does not depend on the
//               order of the candidates: the greatest score over all semi-global alignments, among those the smallest start.
//               H[0][j] = (0, j);  H[i][0] = F[i][0] = (-(go + (i-1) ge), 0);  E[0][j] = F[0][j] = E[i][0] = -infinity
//               E[i][j] = max(H[i][j-1] - go, E[i][j-1] - ge);   F[i][j] = max(H[i-1][j] - go, F[i-1][j] - ge)
//               H[i][j] = max(H[i-1][j-1] + (equal ? match : mismatch), E[i][j], F[i][j])
//               result  = max over j in [0, W] of (H[P][j].score, -start, -j)
//     packing   ONE sortable int32 per pair: key = score * 1024 + (1023 - start).  The window is at most 512 columns, so
//               1023 - start lies in [511, 1023]: ten bits that a score difference (a multiple of 1024) never touches.  A cell
//               value is the score of a real path over at most 128 rows and 512 columns at costs of at most 1024 each:
//               -640 * 1024 <= score <= 128 * 1024, so |key| < 2^30, and the lexicographic maximum is a plain integer max.
//               -infinity is the key -1.5 * 2^30: below every real key minus any cost, and (clamped back after every
//               subtraction) 2^29 away from wrapping.  It stands for the contract's -2^30: a sentinel never reaches a result, since
//               H[i][j] >= F[i][j] > -infinity for every i >= 1, so any sentinel below all real values gives the same cells.
//     mapping   lanes are PATTERNS, not cells.  One wave serves one (read, end) and up to 64 of that end's patterns; the window
//               label of column j is wave-uniform (one LDS broadcast read); every lane runs an ordinary column-by-column Gotoh
//               recurrence of its own: no cross-lane dependency, no DPP shift, no barrier in the cell loop.  Per lane H[i] and
//               E[i] of the previous column persist; F and the diagonal are running scalars.  That column stays in REGISTERS,
//               the row loop fully unrolled in groups of 8 rows and left once past the longest pattern of the wave, in four
//               instantiations by the longest pattern of the call: R = 32, 64, 96 and 128 rows (R = 128 overflows the 256
//               vector registers into 21 accumulation registers; no scratch memory in any of them).  Registers and not LDS
//               also for long patterns: a column of 128 rows in LDS leaves room for one wave per CU.
//               Pattern labels are staged once per wave, transposed to [i][lane] (conflict-free).  A lane latches its result at
//               its own last row; lanes past the end's patterns and rows past P_k compute nothing that is read.
//
//   demux_pick_kernel            one wave per read over the [B][K] tables: per end the best hit (greatest score, ties to the lower
//                                pattern index) and the runner-up (greatest score among that end's patterns of ANOTHER group) by
//                                wave reduction, then thresholds, barcode and trim.  All integer.
//
// Nothing is read back, nothing is allocated, every result leaves through ordinary vector stores; both kernels run on the passed
// stream and can be captured into a graph.
#include <climits>

#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"
#include "wn_wave_dev.h"

namespace wn {

constexpr int kDxMaxWindow = 512;
constexpr int kDxMaxPatterns = 1024;
constexpr int kDxMaxPatLen = 128;
constexpr int kDxMaxLen = 1 << 24;
constexpr int kDxShift = 10;                     // key = score << 10 | (1023 - start)
constexpr int kDxStartMask = (1 << kDxShift) - 1;
constexpr int kDxNeg = -(3 << 29);               // -infinity as a key
constexpr int kDxRowGroup = 8;                   // rows between two looks at the wave's longest pattern
constexpr int kDxMaskRows = 16;                  // rows whose latch mask stays in scalar registers

struct DemuxScoreArgs {
    const int* labels;                   // [B] rows of labels_stride elements
    long long labels_stride;
    const int* lengths;                  // [B]
    const int* patterns;                 // [K] rows of pattern_stride elements
    long long pattern_stride;
    const int* pattern_len;              // [K]
    int* score;                          // [B][K]
    int* start;
    int* end;
    int* bad;
    int B, max_len, K, n_front, max_pat, window;
    int chunks_front, chunks_rear;       // waves per read and end
    int match, mismatch, go, ge;
};

__device__ __forceinline__ int dx_max3(int a, int b, int c) { return max(max(a, b), c); }

template <int R>
__global__ __launch_bounds__(64) void demux_score_kernel(const DemuxScoreArgs a) {
    __shared__ int win[kDxMaxWindow];
    __shared__ int pat[R][64];
    const int lane = threadIdx.x;
    const int per = a.chunks_front + a.chunks_rear;
    const int b = blockIdx.x / per, c = blockIdx.x % per;
    const bool rear = c >= a.chunks_front;
    const int k = rear ? a.n_front + (c - a.chunks_front) * 64 + lane : c * 64 + lane;
    const bool live = k < (rear ? a.K : a.n_front);
    int n = a.lengths[b];
    const bool bad_read = n < 0 || n > a.max_len;
    if (bad_read) n = 0;                                                 // the lengths are never used as an index
    const int Wb = min(n, a.window), off = rear ? n - Wb : 0;
    int P = live ? a.pattern_len[k] : 1;
    const bool bad_pat = P < 1 || P > a.max_pat;
    if (bad_pat) P = 1;

    const int* row = a.labels + (long long)b * a.labels_stride + off;
    for (int j = lane; j < Wb; j += 64) win[j] = row[j];
    if (live && !bad_pat) {
        const int* prow = a.patterns + (long long)k * a.pattern_stride;
        for (int i = 0; i < P; ++i) pat[i][lane] = prow[i];
    }
    const int pmax = __builtin_amdgcn_readfirstlane(wave_reduce(P, OpMax()));    // the longest pattern of the wave
    __syncthreads();

    const int go = a.go << kDxShift, ge = a.ge << kDxShift, ma = a.match << kDxShift, mi = a.mismatch << kDxShift;
    int best = -(go + (P - 1) * ge) + kDxStartMask, best_j = 0;          // H[P][0]
    int H[R], E[R];
    int border = kDxStartMask - go;                                      // H[i][0], stepped in a vector register: the R wave-uniform
    asm volatile("" : "+v"(border));                                     // values would otherwise wait in scalar registers and spill
#pragma unroll
    for (int i = 0; i < R; ++i) { H[i] = border; E[i] = kDxNeg; border -= ge; }
    for (int j = 1; j <= Wb; ++j) {
        const int w = win[j - 1];
        int diag = kDxStartMask - (j - 1), up = kDxStartMask - j, f = kDxNeg, last = kDxNeg;
#pragma unroll
        for (int i0 = 0; i0 < R; i0 += kDxRowGroup) {
            if (i0 < pmax) {                                             // wave-uniform
                // the latch "row i is this lane's last" does not depend on the column: the compiler keeps one lane mask per row
                // in a scalar register pair.  16 rows of masks fit; in the groups after them P is made opaque, so that their
                // compare is a vector instruction per cell, made where it is used, and holds no scalar register
                int p_late = P;
                if (i0 >= kDxMaskRows) asm volatile("" : "+v"(p_late));
#pragma unroll
                for (int i = i0; i < i0 + kDxRowGroup; ++i) {
                    const int e = dx_max3(H[i] - go, E[i] - ge, kDxNeg);
                    f = dx_max3(up - go, f - ge, kDxNeg);
                    const int h = dx_max3(diag + (pat[i][lane] == w ? ma : mi), e, f);
                    diag = H[i]; up = h;
                    H[i] = h; E[i] = e;
                    last = i + 1 == p_late ? h : last;
                }
            }
        }
        if (last > best) { best = last; best_j = j; }
    }

    const bool poisoned = bad_read || bad_pat;
    if (live) {
        const long long o = (long long)b * a.K + k;
        a.score[o] = poisoned ? INT_MIN : best >> kDxShift;              // arithmetic shift: the floor, the low field is >= 0
        a.start[o] = poisoned ? -1 : kDxStartMask - (best & kDxStartMask) + off;
        a.end[o] = poisoned ? -1 : best_j + off;
    }
    const int nbad = __popcll(__ballot(live && poisoned));
    if (lane == 0 && nbad > 0 && a.bad) atomicAdd(a.bad, nbad);
}

struct DemuxPickArgs {
    const int* score;                    // [B][K]
    const int* start;
    const int* end;
    const int* lengths;                  // [B]
    const int* group;                    // [K]
    const int* min_score;                // [K]
    int* barcode;                        // [B]
    int* trim;                           // [B][2]
    int* hits;                           // [B][2][4]
    int* runner_up;                      // [B][2]
    int B, K, n_front, min_margin, require_both;
};

__global__ __launch_bounds__(64) void demux_pick_kernel(const DemuxPickArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int* sc = a.score + (long long)b * a.K;
    int hit[2], hs[2], hb[2], he[2], ru[2];
    bool pass[2];
    for (int end = 0; end < 2; ++end) {
        const int k0 = end ? a.n_front : 0, k1 = end ? a.K : a.n_front;
        // the greatest score, the lowest index among equals: one sortable word (a poisoned entry, INT_MIN, is no candidate)
        long long key = LLONG_MIN;
        for (int k = k0 + lane; k < k1; k += 64) {
            const int s = sc[k];
            if (s != INT_MIN) key = max(key, (long long)s * 4096 + (4095 - k));
        }
        key = wave_reduce(key, OpMax());
        if (key == LLONG_MIN) { hit[end] = -1; hs[end] = -1; hb[end] = -1; he[end] = -1; ru[end] = INT_MIN; pass[end] = false; continue; }
        const int kb = 4095 - (int)(key & 4095), g = a.group[kb];
        int r = INT_MIN;
        for (int k = k0 + lane; k < k1; k += 64)
            if (a.group[k] != g) r = max(r, sc[k]);
        r = wave_reduce(r, OpMax());
        const int s = sc[kb];
        hit[end] = kb; hs[end] = s; ru[end] = r;
        hb[end] = a.start[(long long)b * a.K + kb]; he[end] = a.end[(long long)b * a.K + kb];
        pass[end] = s >= a.min_score[kb] && (r == INT_MIN || (long long)s - r >= a.min_margin);
    }
    if (lane != 0) return;
    int code = -1;
    if (a.require_both) {
        if (pass[0] && pass[1] && a.group[hit[0]] == a.group[hit[1]]) code = a.group[hit[0]];
    } else if (pass[0] && (!pass[1] || hs[0] >= hs[1])) {
        code = a.group[hit[0]];
    } else if (pass[1]) {
        code = a.group[hit[1]];
    }
    const int n = a.lengths[b];
    const int t0 = pass[0] ? he[0] : 0, t1 = pass[1] ? max(t0, hb[1]) : n;
    a.barcode[b] = code;
    a.trim[2 * b] = t0; a.trim[2 * b + 1] = t1;
    for (int end = 0; end < 2; ++end) {
        int* h = a.hits + (long long)b * 8 + 4 * end;
        h[0] = hit[end]; h[1] = hs[end]; h[2] = hb[end]; h[3] = he[end];
        a.runner_up[2 * b + end] = ru[end];
    }
}

}  // namespace wn

using namespace wn;

static int check_demux_shape(int batch, int n_patterns, int n_front) {
    if (batch <= 0 || n_patterns <= 0 || n_front < 0 || n_front > n_patterns) return WN_ERR_BAD_SHAPE;
    return WN_OK;
}

int wn_demux_scores(const int* labels, long long labels_stride, const int* lengths, const int* patterns, long long pattern_stride,
                    const int* pattern_lengths, int batch, int max_len, int n_patterns, int n_front, int max_pattern_len, int window,
                    int match, int mismatch, int gap_open, int gap_extend, int* score, int* start, int* end, int* bad,
                    wn_stream_t stream) {
    const int rc = check_demux_shape(batch, n_patterns, n_front);
    if (rc != WN_OK) return rc;
    if (max_len <= 0 || max_pattern_len <= 0 || window <= 0 || labels_stride < 0 || pattern_stride < 0) return WN_ERR_BAD_SHAPE;
    if (batch > 65535 || max_len > kDxMaxLen || n_patterns > kDxMaxPatterns || max_pattern_len > kDxMaxPatLen || window > kDxMaxWindow)
        return WN_ERR_UNSUPPORTED;
    if (const int s = check_affine_costs(match, mismatch, gap_open, gap_extend)) return s;
    if (!labels || !lengths || !patterns || !pattern_lengths || !score || !start || !end) return WN_ERR_NULL;
    DemuxScoreArgs a = {};
    a.labels = labels; a.labels_stride = labels_stride; a.lengths = lengths;
    a.patterns = patterns; a.pattern_stride = pattern_stride; a.pattern_len = pattern_lengths;
    a.score = score; a.start = start; a.end = end; a.bad = bad;
    a.B = batch; a.max_len = max_len; a.K = n_patterns; a.n_front = n_front; a.max_pat = max_pattern_len; a.window = window;
    a.chunks_front = cdiv(n_front, 64); a.chunks_rear = cdiv(n_patterns - n_front, 64);
    a.match = match; a.mismatch = mismatch; a.go = gap_open; a.ge = gap_extend;
    const dim3 grid((unsigned)batch * (unsigned)(a.chunks_front + a.chunks_rear));
    hipStream_t s = (hipStream_t)stream;
    if (max_pattern_len <= 32) hipLaunchKernelGGL((demux_score_kernel<32>), grid, dim3(64), 0, s, a);
    else if (max_pattern_len <= 64) hipLaunchKernelGGL((demux_score_kernel<64>), grid, dim3(64), 0, s, a);
    else if (max_pattern_len <= 96) hipLaunchKernelGGL((demux_score_kernel<96>), grid, dim3(64), 0, s, a);
    else hipLaunchKernelGGL((demux_score_kernel<kDxMaxPatLen>), grid, dim3(64), 0, s, a);
    WN_HIP(hipGetLastError(), "demux_scores");
    return WN_OK;
}

int wn_demux_pick(const int* score, const int* start, const int* end, const int* lengths, const int* pattern_group,
                  const int* min_score, int batch, int n_patterns, int n_front, int min_margin, int require_both, int* barcode,
                  int* trim, int* hits, int* runner_up, wn_stream_t stream) {
    const int rc = check_demux_shape(batch, n_patterns, n_front);
    if (rc != WN_OK) return rc;
    if (batch > 65535 || n_patterns > kDxMaxPatterns || min_margin < 0) return WN_ERR_UNSUPPORTED;
    if (!score || !start || !end || !lengths || !pattern_group || !min_score || !barcode || !trim || !hits || !runner_up) return WN_ERR_NULL;
    DemuxPickArgs a = {};
    a.score = score; a.start = start; a.end = end; a.lengths = lengths; a.group = pattern_group; a.min_score = min_score;
    a.barcode = barcode; a.trim = trim; a.hits = hits; a.runner_up = runner_up;
    a.B = batch; a.K = n_patterns; a.n_front = n_front; a.min_margin = min_margin; a.require_both = require_both ? 1 : 0;
    hipLaunchKernelGGL(demux_pick_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "demux_pick");
    return WN_OK;
}
