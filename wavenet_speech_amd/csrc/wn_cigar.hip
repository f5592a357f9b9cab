// CIGAR runs from op rows and op rows from CIGAR runs: the two directions between the op row of wn_pair_align
// and the run table SAM / BAM carry.  The definitions are in include/wavenet_amd.h; tests/cigar_ref.py states them as plain loops and
// both kernels equal it exactly.
//
//   cigar_encode_kernel  grid (batch), 256 threads, ONE WORKGROUP PER READ, the walk of wn_opscan.h.
//     pass 1   validate_ops with pileup's window in the header and nothing per column: the verdict, first and last.
//     pass 2   over the tiles up to `last`.  A column of the span has a class (=, X, D, I; = and X are one class without eqx) and is
//              a HEAD when it is `first` or its class differs from that of column w - 1, whose byte is LOADED AGAIN (the plain way:
//              it is right across lanes, waves and tiles without a carry; the listing shows one more byte load from the line the
//              column's own byte came from, and no LDS traffic).  A third ballot gives every head the number of heads before it
//              (wave_offsets over the waves' counts, a running base from tile to tile) and the last head before it (the highest
//              lane below, the waves' last heads through LDS, a running value from tile to tile), as pileup_kernel finds its
//              `prev`.  A head at w > first then CLOSES THE RUN BEFORE IT: entry r - 1 is (w - previous head, the class of w - 1).
//              The column `first` writes the front clip, the column `last` the last run and the back clip.  Every entry so has one
//              writer and is never read: there is no hazard between threads.  The tile of `first` has one barrier more, behind
//              which every thread knows whether there is a front clip.
//     end      writes are guarded by max_cigar; behind the barrier that ends pass 2 the row is zeroed from n_cigar on, or whole when
//              it needed more than max_cigar entries (used -2): a row is never truncated.
//   cigar_decode_kernel  grid (batch), 256 threads, ONE WORKGROUP PER READ.
//     pass 1   over the runs in tiles of 256: a run's columns, reference and query labels (its length, clamped to max_ops + 1: the
//              sums of a tile cannot wrap, and the running sums saturate at 2^27), three wave_scans and ONE barrier per tile, the
//              exclusive sums to the workspace [3][max_cigar]; then the checks on the totals.
//     pass 2   over the columns in tiles of 256: a binary search over the column offsets finds the run, the run's offsets give i
//              and j, the labels are loaded only where the op consumes both, and the column writes itself at w or n - 1 - w.
//              With `strict` a vote behind the pass turns the row bad and zeroes it.
// One launch each; no workgroup waits on another; nothing is read back.  No floating point, no scratch.  No value of an op, a run, a
// length, a position or a strand is used as an index before it is checked.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_opscan.h"

#include <cstdint>

namespace wn {

constexpr int kCgMaxCigar = 65535;            // BAM's n_cigar_op is 16 bits
constexpr int kCgSat = 1 << 27;               // where the running sums of the decoder stop growing: above every limit
constexpr int kCgM = 0, kCgI = 1, kCgD = 2, kCgN = 3, kCgS = 4, kCgEq = 7, kCgX = 8;      // BAM's codes; H 5 and P 6 emit nothing

struct CigarEncodeArgs {
    const unsigned char* ops;           // row b at ops + b * ops_stride
    const int *ops_len, *lo, *ref_len, *strand, *query_len;
    const unsigned char* keep;
    long long ops_stride, cigar_stride;
    unsigned* cigar;                    // row b at cigar + b * cigar_stride
    int* n_cigar;
    int* fields;                        // [B][5]
    signed char* used;
    int* bad;
    int B, M, max_ops, R, eqx, max_cigar;
};

// the class of an op: 1 '=' (and X without eqx), 2 X, 3 D, 4 I; and its BAM code
__device__ __forceinline__ int cigar_class(int op, int eqx) { return !eqx && op == 2 ? 1 : op; }
__device__ __forceinline__ unsigned cigar_code(int cls, int eqx) {
    return cls == 1 ? (eqx ? kCgEq : kCgM) : cls == 2 ? kCgX : cls == 3 ? kCgD : kCgI;
}

__global__ __launch_bounds__(kPThreads) void cigar_encode_kernel(const CigarEncodeArgs a) {
    __shared__ int s_slot[2][2][kPWaves];
    __shared__ int s_lo, s_hi, s_bad;
    __shared__ int s_heads[2][kPWaves], s_head_at[2][kPWaves];
    __shared__ int s_first_i, s_first_j, s_last_i, s_last_j, s_runs, s_nm;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned* out = a.cigar + (long long)b * a.cigar_stride;
    int* fields = a.fields + (long long)b * 5;

    // a skipped or a bad read, or one without an aligned column: an empty row
    const auto empty_row = [&](int verdict) {
        for (int r = tid; r < a.max_cigar; r += kPThreads) out[r] = 0u;
        if (tid == 0) {
            a.n_cigar[b] = 0;
            fields[0] = -1; fields[1] = 0; fields[2] = 0; fields[3] = 0; fields[4] = 0;
            a.used[b] = (signed char)verdict;
        }
    };

    const int strand = a.strand[b], n_ref = a.ref_len[b];
    if (read_skipped(strand, n_ref, a.keep, b)) {                    // nothing else of the read is looked at
        empty_row(0);
        return;
    }
    const int n_ops = a.ops_len[b], n_query = a.query_len[b], lo = a.lo[b];
    const bool header_ok = head_ok(strand, n_ref, lo >= 0 && (long long)lo + n_ref <= a.R, n_query, a.M, n_ops, a.max_ops);
    const OpRow row = op_row(a.ops + (long long)b * a.ops_stride, header_ok, n_ops, n_ref, n_query, strand == 1);

    validate_begin(tid, header_ok, &s_lo, &s_hi, &s_bad);
    if (tid == 0) s_nm = 0;
    __syncthreads();

    // ---- pass 1: validate, first / last aligned walk index
    OpWalk walk{s_slot};
    const OpSpan span = validate_ops(row, tid, &walk, &s_lo, &s_hi, &s_bad, [](const OpCol&, bool, bool) { return true; });
    if (span.bad) {
        empty_row(-1);
        report_bad(tid, a.bad);
        return;
    }
    const int first = span.first, last = span.last;
    if (last < 0) {                                                  // no aligned column: end columns only
        empty_row(0);
        return;
    }

    // ---- pass 2: the runs.  The ops are loaded again; first <= last < n were found in pass 1 on the same bytes
    const unsigned long long below = (1ull << lane) - 1ull;
    int head_before = -1;                                            // the last head of the tiles before this one
    int runs_before = 0;                                             // heads of the tiles before this one
    int front = 0;                                                   // 1 with a front clip: known from the tile of `first` on
    int nm = 0;                                                      // of this wave, the same in its lanes
    walk.base_ref = walk.base_query = 0;
    for (int t0 = 0; t0 <= last; t0 += kPThreads) {
        OpCol c = row.load(t0 + tid);
        const int w = c.w, slot = walk.tile & 1;
        const bool in_span = c.active && w >= first && w <= last;
        const int cls = cigar_class(c.op, a.eqx);
        const int cls_left = in_span && w > first ? cigar_class((int)row.ops[row.column(w - 1)], a.eqx) : 0;
        const bool head = in_span && cls != cls_left;                // `first` has no left class: a head
        const unsigned long long m_head = __ballot(head);
        nm += __popcll(__ballot(in_span && c.op >= 2));
        if (lane == 0) {
            s_heads[slot][wave] = __popcll(m_head);
            s_head_at[slot][wave] = m_head ? t0 + wave * 64 + 63 - __clzll((long long)m_head) : -1;
        }
        walk.scan(&c, tid);                                          // the barrier is in here
        int heads_left, heads_tile;
        wave_offsets<kPWaves>(s_heads[slot], wave, &heads_left, &heads_tile);
        int prev = head_before;                                      // the last head before w
#pragma unroll
        for (int v = 0; v < kPWaves; ++v) {
            const int l = s_head_at[slot][v];
            if (l >= 0) {
                head_before = l;
                if (v < wave) prev = l;
            }
        }
        if (m_head & below) prev = t0 + wave * 64 + 63 - __clzll((long long)(m_head & below));
        const int heads = runs_before + heads_left + __popcll(m_head & below);     // heads before w
        runs_before += heads_tile;
        if (t0 <= first && first < t0 + kPThreads) {                 // the same in every thread: the tile of `first`
            if (w == first) { s_first_i = c.i; s_first_j = c.j; }
            __syncthreads();
            front = s_first_j > 0 ? 1 : 0;
        }
        if (!in_span) continue;
        if (w == first) {
            if (c.j > 0 && a.max_cigar > 0) out[0] = (unsigned)c.j << 4 | kCgS;
        } else if (head) {                                           // closes the run before it: entry front + heads - 1
            const int r = front + heads - 1;
            if (r < a.max_cigar) out[r] = (unsigned)(w - prev) << 4 | cigar_code(cls_left, a.eqx);
        }
        if (w == last) {                                             // the last run and the back clip
            const int r = front + heads - (head ? 0 : 1), start = head ? w : prev;
            const int clip_back = n_query - c.j - 1;
            if (r < a.max_cigar) out[r] = (unsigned)(w + 1 - start) << 4 | cigar_code(cls, a.eqx);
            if (clip_back > 0 && r + 1 < a.max_cigar) out[r + 1] = (unsigned)clip_back << 4 | kCgS;
            s_last_i = c.i; s_last_j = c.j;
            s_runs = r + 1 + (clip_back > 0 ? 1 : 0);
        }
    }
    if (lane == 0) atomicAdd(&s_nm, nm);
    __syncthreads();                                                 // the runs are written; the zeroes below never meet them unordered

    const int n_runs = s_runs;
    const bool fits = n_runs <= a.max_cigar;
    for (int r = (fits ? n_runs : 0) + tid; r < a.max_cigar; r += kPThreads) out[r] = 0u;
    if (tid == 0) {
        a.n_cigar[b] = n_runs;
        fields[0] = lo + s_first_i;
        fields[1] = s_last_i - s_first_i + 1;
        fields[2] = s_first_j;
        fields[3] = n_query - s_last_j - 1;
        fields[4] = s_nm;
        a.used[b] = (signed char)(fits ? 1 : -2);
    }
    if (!fits) report_bad(tid, a.bad);
}

struct CigarDecodeArgs {
    const unsigned* cigar;              // row b at cigar + b * cigar_stride
    const int *n_cigar, *pos, *strand, *reference, *query, *query_len;
    long long cigar_stride, query_stride, ops_stride;
    unsigned char* ops;                 // row b at ops + b * ops_stride
    int *ops_len, *ref_len, *stats;
    signed char* used;
    int* offsets;                       // the workspace: [B][3][max_cigar]
    int* bad;
    int B, R, max_cigar, M, max_ops, strict;
};

__global__ __launch_bounds__(kPThreads) void cigar_decode_kernel(const CigarDecodeArgs a) {
    __shared__ int s_sum[2][3][kPWaves];
    __shared__ int s_match, s_mismatch;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned char* out = a.ops + (long long)b * a.ops_stride;

    // a skipped or a bad read: an empty row
    const auto empty_row = [&](int verdict) {
        for (int c = tid; c < a.max_ops; c += kPThreads) out[c] = 0;
        if (tid == 0) {
            const int v = verdict < 0 ? -1 : 0;
            a.ops_len[b] = 0;
            a.ref_len[b] = 0;
            a.stats[4 * b] = v; a.stats[4 * b + 1] = v; a.stats[4 * b + 2] = v; a.stats[4 * b + 3] = v;
            a.used[b] = (signed char)verdict;
        }
        if (verdict < 0) report_bad(tid, a.bad);
    };

    const int strand = a.strand[b], n_runs = a.n_cigar[b];
    if (strand < 0 || n_runs == 0) {                                 // nothing else of the read is looked at
        empty_row(0);
        return;
    }
    const int pos = a.pos[b], n_query = a.query_len[b];
    if (strand > 1 || n_runs < 0 || n_runs > a.max_cigar || pos < 0 || n_query < 0 || n_query > a.M) {
        empty_row(-1);
        return;
    }
    const bool rev = strand == 1;
    const unsigned* runs = a.cigar + (long long)b * a.cigar_stride;
    int* off_col = a.offsets + (long long)b * 3 * a.max_cigar;
    int* off_ref = off_col + a.max_cigar;
    int* off_query = off_ref + a.max_cigar;
    if (tid == 0) { s_match = 0; s_mismatch = 0; }

    // ---- pass 1: what every run consumes, scanned; the exclusive sums go to the workspace
    const int cap = a.max_ops + 1;                                   // a longer run is bad whatever its length
    int base_col = 0, base_ref = 0, base_query = 0;
    bool ok = true;
    for (int r0 = 0, tile = 0; r0 < n_runs; r0 += kPThreads, ++tile) {
        const int r = r0 + tid;
        int n_col = 0, n_r = 0, n_q = 0;
        if (r < n_runs) {
            const unsigned run = runs[r];
            const int code = (int)(run & 15u), len = (int)(run >> 4) < cap ? (int)(run >> 4) : cap;
            if (code > kCgX || code == kCgN) ok = false;
            const bool is_ref = code == kCgM || code == kCgD || code == kCgEq || code == kCgX;
            const bool is_query = code == kCgM || code == kCgI || code == kCgS || code == kCgEq || code == kCgX;
            n_col = is_ref || is_query ? len : 0;                    // H, P: nothing
            n_r = is_ref ? len : 0;
            n_q = is_query ? len : 0;
        }
        const int inc_col = wave_scan(n_col, lane, OpAdd()), inc_ref = wave_scan(n_r, lane, OpAdd()), inc_query = wave_scan(n_q, lane, OpAdd());
        int (*slot)[kPWaves] = s_sum[tile & 1];                      // written again two tiles on, a barrier between
        if (lane == 63) { slot[0][wave] = inc_col; slot[1][wave] = inc_ref; slot[2][wave] = inc_query; }
        __syncthreads();
        int left_col, left_ref, left_query, tot_col, tot_ref, tot_query;
        wave_offsets<kPWaves>(slot[0], wave, &left_col, &tot_col);
        wave_offsets<kPWaves>(slot[1], wave, &left_ref, &tot_ref);
        wave_offsets<kPWaves>(slot[2], wave, &left_query, &tot_query);
        if (r < n_runs) {
            off_col[r] = base_col + left_col + inc_col - n_col;
            off_ref[r] = base_ref + left_ref + inc_ref - n_r;
            off_query[r] = base_query + left_query + inc_query - n_q;
        }
        base_col = base_col + tot_col < kCgSat ? base_col + tot_col : kCgSat;      // a tile adds less than 2^25: no wrap
        base_ref = base_ref + tot_ref < kCgSat ? base_ref + tot_ref : kCgSat;
        base_query = base_query + tot_query < kCgSat ? base_query + tot_query : kCgSat;
    }
    const int n = base_col, n_ref = base_ref;                        // the same in every thread
    if (n > a.max_ops || n_ref < 1 || (long long)pos + n_ref > a.R || base_query != n_query) ok = false;
    if (__syncthreads_or(ok ? 0 : 1)) {                              // also: the offsets are in place for every wave
        empty_row(-1);
        return;
    }

    // ---- pass 2: every column finds its run.  n <= max_ops, pos + n_ref <= R and the query labels are exactly n_query
    int n_match = 0, n_mismatch = 0;
    bool strict_ok = true;
    for (int t0 = 0; t0 < n; t0 += kPThreads) {
        const int w = t0 + tid;
        int op = 0;
        if (w < n) {
            int lo_r = 0, hi_r = n_runs;                             // the first run that starts behind w; the one before holds w
            while (lo_r < hi_r) {
                const int mid = (lo_r + hi_r) >> 1;
                if (off_col[mid] <= w) lo_r = mid + 1;
                else hi_r = mid;
            }
            const int r = lo_r > 0 ? lo_r - 1 : 0;
            const int code = (int)(runs[r] & 15u), k = w - off_col[r];
            if (code == kCgD) op = 3;
            else if (code == kCgI || code == kCgS) op = 4;
            else {
                const int i = off_ref[r] + k, j = off_query[r] + k;
                int equal = 0;
                if (i >= 0 && i < n_ref && j >= 0 && j < n_query) {  // checked again before it is used
                    const int v = a.query[(long long)b * a.query_stride + (rev ? n_query - 1 - j : j)];
                    equal = a.reference[pos + i] == (rev && v >= 1 && v <= 4 ? 5 - v : v);
                }
                op = equal ? 1 : 2;
                if (a.strict && ((code == kCgEq && !equal) || (code == kCgX && equal))) strict_ok = false;
            }
            out[rev ? n - 1 - w : w] = (unsigned char)op;
        }
        n_match += __popcll(__ballot(op == 1));
        n_mismatch += __popcll(__ballot(op == 2));
    }
    if (lane == 0) { atomicAdd(&s_match, n_match); atomicAdd(&s_mismatch, n_mismatch); }
    if (__syncthreads_or(strict_ok ? 0 : 1)) {                       // the columns are written: the zeroes come behind them
        empty_row(-1);
        return;
    }
    for (int c = n + tid; c < a.max_ops; c += kPThreads) out[c] = 0;
    if (tid == 0) {
        a.ops_len[b] = n;
        a.ref_len[b] = n_ref;
        a.stats[4 * b] = s_match; a.stats[4 * b + 1] = s_mismatch; a.stats[4 * b + 2] = n - s_match - s_mismatch; a.stats[4 * b + 3] = n;
        a.used[b] = 1;
    }
}

static int cigar_shape(int batch, int max_cigar) {
    if (batch < 1 || max_cigar < 1) return WN_ERR_BAD_SHAPE;
    if (batch > 65535 || max_cigar > kCgMaxCigar) return WN_ERR_UNSUPPORTED;
    return WN_OK;
}

}  // namespace wn
using namespace wn;

int wn_cigar_encode(const unsigned char* ops, long long ops_stride, const int* ops_len, const int* lo, const int* ref_lengths,
                    const int* strand, const int* query_lengths, const unsigned char* keep, int batch, int max_query_len, int max_ops,
                    int reference_len, int eqx, int max_cigar, unsigned* cigar, long long cigar_stride, int* n_cigar, int* fields,
                    signed char* used, int* bad, wn_stream_t stream) {
    if (const int s = check_op_rows(batch, max_query_len, max_ops, ops_stride, 0,
                                    reference_len >= 1 && max_cigar >= 1 && cigar_stride >= 0 && (eqx == 0 || eqx == 1),
                                    reference_len <= kMaxReference && max_cigar <= kCgMaxCigar,
                                    ops && ops_len && lo && ref_lengths && strand && query_lengths && cigar && n_cigar && fields && used))
        return s;
    CigarEncodeArgs a = {};
    a.ops = ops; a.ops_len = ops_len; a.lo = lo; a.ref_len = ref_lengths; a.strand = strand; a.query_len = query_lengths; a.keep = keep;
    a.ops_stride = ops_stride; a.cigar_stride = cigar_stride; a.cigar = cigar; a.n_cigar = n_cigar; a.fields = fields; a.used = used;
    a.bad = bad; a.B = batch; a.M = max_query_len; a.max_ops = max_ops; a.R = reference_len; a.eqx = eqx; a.max_cigar = max_cigar;
    hipLaunchKernelGGL(cigar_encode_kernel, dim3(batch), dim3(kPThreads), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "cigar_encode");
    return WN_OK;
}

size_t wn_cigar_decode_workspace_bytes(int batch, int max_cigar) {
    if (cigar_shape(batch, max_cigar) != WN_OK) return 0;
    return ((size_t)batch * 3 * (size_t)max_cigar * sizeof(int) + 15) / 16 * 16;
}

int wn_cigar_decode(const unsigned* cigar, long long cigar_stride, const int* n_cigar, const int* pos, const int* strand,
                    const int* reference, int reference_len, const int* query, long long query_stride, const int* query_lengths,
                    int batch, int max_cigar, int max_query_len, int max_ops, int strict, unsigned char* ops, long long ops_stride,
                    int* ops_len, int* ref_lengths, int* stats, signed char* used, void* workspace, size_t workspace_bytes, int* bad,
                    wn_stream_t stream) {
    if (const int s = check_op_rows(batch, max_query_len, max_ops, ops_stride, query_stride,
                                    reference_len >= 1 && max_cigar >= 1 && cigar_stride >= 0 && (strict == 0 || strict == 1),
                                    reference_len <= kMaxReference && max_cigar <= kCgMaxCigar,
                                    cigar && n_cigar && pos && strand && reference && query && query_lengths && ops && ops_len &&
                                        ref_lengths && stats && used && workspace))
        return s;
    if (workspace_bytes < wn_cigar_decode_workspace_bytes(batch, max_cigar) || ((uintptr_t)workspace & 15u)) return WN_ERR_WORKSPACE;
    CigarDecodeArgs a = {};
    a.cigar = cigar; a.n_cigar = n_cigar; a.pos = pos; a.strand = strand; a.reference = reference; a.query = query;
    a.query_len = query_lengths; a.cigar_stride = cigar_stride; a.query_stride = query_stride; a.ops_stride = ops_stride; a.ops = ops;
    a.ops_len = ops_len; a.ref_len = ref_lengths; a.stats = stats; a.used = used; a.offsets = (int*)workspace; a.bad = bad;
    a.B = batch; a.R = reference_len; a.max_cigar = max_cigar; a.M = max_query_len; a.max_ops = max_ops; a.strict = strict;
    hipLaunchKernelGGL(cigar_decode_kernel, dim3(batch), dim3(kPThreads), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "cigar_decode");
    return WN_OK;
}
