// Realignment of reads against the called haplotypes: the two steps around wn_pair_align.  The DP itself is
// wn_pair_align's, run once per haplotype between the two kernels of this file.
//
//   haplotype_windows_kernel   grid (batch, H), 256 threads, ONE WORKGROUP PER (READ, HAPLOTYPE), positions in tiles of 256.  A
//                              position gives one op and up to 1 + max_ins labels, so where it lands is a running sum: two of them,
//                              labels and ops, through block_scan.  Pass 1 sums the totals of EVERY haplotype of the read (a read
//                              that is bad on one is bad on both, so that `used` and *bad are per read, and a reverse-strand row is
//                              written from the back); pass 2 scans this workgroup's haplotype and writes.  The workgroup of
//                              haplotype 0 writes used[b] and counts *bad.
//   lift_ops_kernel            grid (batch), 256 threads, ONE WORKGROUP PER READ.  A is the picked read -> haplotype row, Hh the
//                              haplotype -> reference row; SLOT j in [0, Lh] is what the composition emits for haplotype label j:
//                              the reference labels Hh skips before it (3s), the read labels A skips before it (4s), then the shared
//                              column (slot Lh: the trailing runs only).  Two validating walks (wn_opscan.h; both rows are walked
//                              front to back) record per haplotype label its reference index and whether Hh aligns it (w_r), and its
//                              read index and whether A aligns it (w_q).  An output column consumes a reference label, a read label
//                              or both, so the columns before slot j are (reference labels before) + (read labels before) - m[j],
//                              m[j] the both-aligned slots below j: ONE scan over the slots (w_m).  Then every column of either row
//                              writes itself: a 3 of Hh at (its reference index) + (read labels before its slot) - m, a 4 of A at (its
//                              read index) + w_r - m, the shared column at w_r + w_q - m.  No thread loops over a run.  A last pass
//                              over the written row counts matches, mismatches and gap runs and finds the two end runs.
//                              The workspace is 3 int32 per haplotype index and read; it is written and read by the same
//                              workgroup only, with a barrier between.
// No floating point, no scratch, no workgroup waits on another, nothing is read back.  No value of an op, a length, a position, a
// pick or an ins_len is used as an index before it is checked.
#include <cstdint>

#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_opscan.h"

namespace wn {

constexpr int kRMaxHaplotypes = 2;
constexpr int kRAligned = 1 << 30;            // of a w_r / w_q word: the column is an op 1 or 2; indices stay below 2^17
constexpr int kRPoison = INT_MIN;             // the score of a bad row, as wn_pair_align's

struct WindowArgs {
    const unsigned char* call;          // [H][R]
    const unsigned char* ins_len;       // [H][R]
    const unsigned char* ins_bases;     // [H][R][max_ins]; nullptr with max_ins == 0
    const int* reference;               // [R]
    const int *lo, *ref_len, *strand;   // [B]
    int* labels;                        // [H][B][cap]
    int* lengths;                       // [H][B]
    unsigned char* ops;                 // [H][B][cap]
    int* ops_len;                       // [H][B]
    signed char* used;                  // [B]
    int* bad;
    int H, B, R, max_ins, cap;
};

__global__ __launch_bounds__(kPThreads) void haplotype_windows_kernel(const WindowArgs a) {
    __shared__ int s_scan[2][2][kPWaves];
    __shared__ int s_sum[kPWaves][2 * kRMaxHaplotypes + 1];
    const int b = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row = (size_t)h * a.B + b;
    int* labels = a.labels + row * a.cap;
    unsigned char* ops = a.ops + row * a.cap;
    const int strand = a.strand[b], n = a.ref_len[b], lo = a.lo[b];

    int state = 1, n_ops = 0, n_labels = 0;                          // the same in every thread
    if (strand < 0 || n == 0) {
        state = 0;                                                   // skipped: nothing else of the read is looked at
    } else if (strand > 1 || lo < 0 || n < 0 || (long long)lo + n > a.R) {
        state = -1;
    } else {
        // ---- pass 1: the totals of every haplotype of the read
        int t_ops[kRMaxHaplotypes] = {0, 0}, t_lab[kRMaxHaplotypes] = {0, 0}, over = 0;
        for (int t0 = 0; t0 < n; t0 += kPThreads) {
            const int k = t0 + tid;
            if (k >= n) continue;
#pragma unroll
            for (int g = 0; g < kRMaxHaplotypes; ++g) {
                if (g >= a.H) continue;
                const size_t p = (size_t)g * a.R + lo + k;
                const int v = a.call[p], e = a.ins_len[p];
                over |= e > a.max_ins ? 1 : 0;
                const int e_in = k < n - 1 ? e : 0;                  // the insertion after the last position is outside the window
                t_ops[g] += 1 + e_in;
                t_lab[g] += (v != 0 ? 1 : 0) + e_in;
            }
        }
        wave_reduce_each(OpAdd(), t_ops[0], t_lab[0], t_ops[1], t_lab[1]);
        over = wave_reduce(over, OpOr());
        if (lane == 0) { s_sum[wave][0] = t_ops[0]; s_sum[wave][1] = t_lab[0]; s_sum[wave][2] = t_ops[1]; s_sum[wave][3] = t_lab[1]; s_sum[wave][4] = over; }
        __syncthreads();
        int sum[2 * kRMaxHaplotypes + 1] = {0, 0, 0, 0, 0};
#pragma unroll
        for (int w = 0; w < kPWaves; ++w)
#pragma unroll
            for (int q = 0; q < 2 * kRMaxHaplotypes + 1; ++q) sum[q] += s_sum[w][q];
        if (sum[4] != 0 || sum[0] > a.cap || sum[2] > a.cap) state = -1;     // an ins_len above max_ins, or a row that does not fit
        n_ops = h == 0 ? sum[0] : sum[2];
        n_labels = h == 0 ? sum[1] : sum[3];
    }
    if (state != 1) n_ops = n_labels = 0;
    if (tid == 0) {
        a.lengths[row] = n_labels;
        a.ops_len[row] = n_ops;
        if (h == 0) {
            a.used[b] = (signed char)state;
            if (state < 0 && a.bad) atomicAdd(a.bad, 1);
        }
    }
    for (int k = n_labels + tid; k < a.cap; k += kPThreads) labels[k] = 0;   // the tails; the whole row of a skipped or bad read
    for (int k = n_ops + tid; k < a.cap; k += kPThreads) ops[k] = 0;
    if (state != 1) return;

    // ---- pass 2: where every position lands, and the writes.  The scan slots alternate from tile to tile (wn_wave_dev.h)
    const unsigned char* call = a.call + (size_t)h * a.R;
    const unsigned char* ins_len = a.ins_len + (size_t)h * a.R;
    const bool rev = strand == 1;
    int base_ops = 0, base_lab = 0, tile = 0;
    for (int t0 = 0; t0 < n; t0 += kPThreads, ++tile) {
        const int k = t0 + tid;
        const bool active = k < n;
        const int p = lo + (active ? k : 0);
        const int v = active ? (int)call[p] : 0;
        int e = active && k < n - 1 ? (int)ins_len[p] : 0;
        e = e <= a.max_ins ? e : 0;                                  // checked in pass 1; never an index beyond the row
        const int has = v != 0 ? 1 : 0;
        int tot_ops, tot_lab;
        const int at_op = base_ops + block_scan<kPWaves>(active ? 1 + e : 0, tid, s_scan[tile & 1][0], &tot_ops);
        const int at_lab = base_lab + block_scan<kPWaves>(active ? has + e : 0, tid, s_scan[tile & 1][1], &tot_lab);
        base_ops += tot_ops;
        base_lab += tot_lab;
        if (!active) continue;
        const auto put_op = [&](int at, int op) {
            const int x = rev ? n_ops - 1 - at : at;
            if ((unsigned)x < (unsigned)n_ops) ops[x] = (unsigned char)op;
        };
        const auto put_label = [&](int at, int label) {
            const int x = rev ? n_labels - 1 - at : at;
            if ((unsigned)x < (unsigned)n_labels) labels[x] = rev && label >= 1 && label <= 4 ? 5 - label : label;
        };
        put_op(at_op, v == 0 ? 3 : v == a.reference[p] ? 1 : 2);
        if (has) put_label(at_lab, v);
        for (int t = 0; t < e; ++t) {                                // at most max_ins <= 8
            put_op(at_op + 1 + t, 4);
            put_label(at_lab + has + t, a.ins_bases[((size_t)h * a.R + p) * a.max_ins + t]);
        }
    }
}

struct LiftArgs {
    const unsigned char* a_ops;         // row (h, b) at a_ops + h * a_hap_stride + b * a_stride
    const int* a_len;                   // [H][B]
    const unsigned char* h_ops;         // likewise
    const int *h_len, *hap_len;         // [H][B]
    const signed char* used;            // [B]
    const int *pick, *ref, *ref_len, *query, *query_len;
    unsigned char* out;
    int *out_len, *score, *stats, *work, *bad;
    long long a_hap_stride, a_stride, h_hap_stride, h_stride, ref_stride, query_stride, out_stride;
    int H, B, N, M, a_max_ops, max_hap_ops, max_hap_len, max_ops;
    int match, mismatch, gap_open, gap_extend, free_ends;
};

// a row that is skipped (ops_len 0, zeros) or bad (ops_len 0, stats -1, the poisoned score, counted once)
__device__ __forceinline__ void lift_nothing(const LiftArgs& a, int b, int tid, unsigned char* out, bool bad) {
    for (int k = tid; k < a.max_ops; k += kPThreads) out[k] = 0;
    if (tid != 0) return;
    a.out_len[b] = 0;
    a.score[b] = bad ? kRPoison : 0;
    for (int q = 0; q < 4; ++q) a.stats[4 * b + q] = bad ? -1 : 0;
    if (bad && a.bad) atomicAdd(a.bad, 1);
}

__global__ __launch_bounds__(kPThreads) void lift_ops_kernel(const LiftArgs a) {
    __shared__ int s_slot[2][2][kPWaves];
    __shared__ int s_lo[2], s_hi[2], s_bad[2];
    __shared__ int s_scan[2][kPWaves];
    __shared__ int s_sum[kPWaves][5];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned char* out = a.out + (long long)b * a.out_stride;
    const int state = a.used[b];
    if (state == 0) return lift_nothing(a, b, tid, out, false);      // a skipped window passes through

    const int h = a.pick[b], n_ref = a.ref_len[b], n_query = a.query_len[b];
    bool header_ok = state == 1 && h >= 0 && h < a.H && n_ref >= 1 && n_ref <= a.N && n_query >= 0 && n_query <= a.M;
    int n_a = 0, n_h = 0, L = 0;
    if (header_ok) {
        const size_t r = (size_t)h * a.B + b;
        n_a = a.a_len[r]; n_h = a.h_len[r]; L = a.hap_len[r];
        header_ok = n_a >= 0 && n_a <= a.a_max_ops && n_h >= 0 && n_h <= a.max_hap_ops && L >= 0 && L <= a.max_hap_len;
    }
    const int hh = header_ok ? h : 0;
    if (!header_ok) L = 0;
    // Hh: `ref` is the reference window, `query` the haplotype; A: `ref` is the haplotype, `query` the read
    const OpRow row_h = op_row(a.h_ops + hh * a.h_hap_stride + b * a.h_stride, header_ok, n_h, n_ref, L, false);
    const OpRow row_a = op_row(a.a_ops + hh * a.a_hap_stride + b * a.a_stride, header_ok, n_a, L, n_query, false);
    const size_t slots = (size_t)a.max_hap_len + 1;
    int* w_r = a.work + (size_t)b * 3 * slots;                       // reference index | kRAligned of haplotype label j; [L]: n_ref
    int* w_q = w_r + slots;                                          // read index | kRAligned;                         [L]: n_query
    int* w_m = w_q + slots;                                          // the both-aligned slots below j
    if (tid == 0) {
        s_lo[0] = s_lo[1] = INT_MAX; s_hi[0] = s_hi[1] = -1; s_bad[0] = s_bad[1] = header_ok ? 0 : 1;    // validate_begin, twice
        if (header_ok) { w_r[L] = n_ref; w_q[L] = n_query; }         // the tail slot; the walks write below L only
    }
    __syncthreads();
    OpWalk walk{s_slot};
    const OpSpan span_h = validate_ops(row_h, tid, &walk, &s_lo[0], &s_hi[0], &s_bad[0], [&](const OpCol& c, bool, bool in_hap) {
        if (in_hap) w_r[c.j] = c.i | (c.op <= 2 ? kRAligned : 0);    // c.j < L: checked
        return true;
    });
    const OpSpan span_a = validate_ops(row_a, tid, &walk, &s_lo[1], &s_hi[1], &s_bad[1], [&](const OpCol& c, bool in_hap, bool) {
        if (in_hap) w_q[c.i] = c.j | (c.op <= 2 ? kRAligned : 0);
        return true;
    });
    if (span_h.bad || span_a.bad) return lift_nothing(a, b, tid, out, true);     // validate_ops' barrier is behind every write above

    // ---- the scan over the slots
    int m = 0;
    for (int t0 = 0, tile = 0; t0 <= L; t0 += kPThreads, ++tile) {
        const int j = t0 + tid;
        const int both = j < L && (w_r[j] & w_q[j] & kRAligned) ? 1 : 0;
        int tot;
        const int below = block_scan<kPWaves>(both, tid, s_scan[tile & 1], &tot);
        if (j <= L) w_m[j] = m + below;
        m += tot;
    }
    const int total = n_ref + n_query - m;                           // >= 1: n_ref >= 1 and m <= min(n_ref, n_query)
    if (total > a.max_ops) return lift_nothing(a, b, tid, out, true);
    __syncthreads();                                                 // w_m before the columns read it

    // ---- every column of either row writes itself
    const int* ref = a.ref + (long long)b * a.ref_stride;
    const int* query = a.query + (long long)b * a.query_stride;
    const auto put = [&](int at, int op) { if ((unsigned)at < (unsigned)total) out[at] = (unsigned char)op; };
    walk_ops(row_h, tid, &walk, [&](const OpCol& c) {
        if (!c.active || c.op != 3) return;
        const int before = c.j > 0 ? w_q[c.j - 1] : 0;               // the read labels before the slot: the last one's index, and itself
        put(c.i + (before & (kRAligned - 1)) + (before >> 30) - w_m[c.j], 3);
    });
    walk_ops(row_a, tid, &walk, [&](const OpCol& c) {
        if (!c.active) return;
        const int word = w_r[c.i], at = c.j + (word & (kRAligned - 1)) - w_m[c.i];
        if (c.op == 4) return put(at, 4);                            // behind the 3s of its slot
        const bool in_read = c.op <= 2, in_ref = (word & kRAligned) != 0;
        if (in_read && in_ref) put(at, ref[word & (kRAligned - 1)] == query[c.j] ? 1 : 2);       // compared afresh
        else if (in_read) put(at, 4);
        else if (in_ref) put(at, 3);
    });
    for (int k = total + tid; k < a.max_ops; k += kPThreads) out[k] = 0;
    __syncthreads();                                                 // the row before it is counted

    // ---- the stats, the gap runs and the two end runs
    const int first_op = out[0], last_op = out[total - 1];
    int matches = 0, mismatches = 0, runs = 0, neg_first = -total, last = -1;      // the first column unlike out[0], the last unlike out[total - 1]
    for (int k = tid; k < total; k += kPThreads) {
        const int v = out[k], left = k > 0 ? (int)out[k - 1] : 0;
        matches += v == 1 ? 1 : 0;
        mismatches += v == 2 ? 1 : 0;
        runs += v >= 3 && v != left ? 1 : 0;
        if (v != first_op && -k > neg_first) neg_first = -k;
        if (v != last_op) last = k;
    }
    wave_reduce_each(OpAdd(), matches, mismatches, runs);
    wave_reduce_each(OpMax(), neg_first, last);
    if (lane == 0) { s_sum[wave][0] = matches; s_sum[wave][1] = mismatches; s_sum[wave][2] = runs; s_sum[wave][3] = neg_first; s_sum[wave][4] = last; }
    __syncthreads();
    if (tid != 0) return;
    matches = mismatches = runs = 0;
    for (int w = 0; w < kPWaves; ++w) {
        matches += s_sum[w][0]; mismatches += s_sum[w][1]; runs += s_sum[w][2];
        neg_first = s_sum[w][3] > neg_first ? s_sum[w][3] : neg_first;
        last = s_sum[w][4] > last ? s_sum[w][4] : last;
    }
    const int gaps = total - matches - mismatches, head = -neg_first;      // head == total: one run is the whole row
    int cost = runs * a.gap_open + (gaps - runs) * a.gap_extend;
    if (a.free_ends) {
        if (first_op >= 3) cost -= a.gap_open + (head - 1) * a.gap_extend;
        if (last_op >= 3 && head < total) cost -= a.gap_open + (total - 1 - last - 1) * a.gap_extend;
    }
    a.out_len[b] = total;
    a.score[b] = a.match * matches + a.mismatch * mismatches - cost;
    a.stats[4 * b] = matches; a.stats[4 * b + 1] = mismatches; a.stats[4 * b + 2] = gaps; a.stats[4 * b + 3] = total;
}

static int check_lift_shape(int haplotypes, int batch, int max_hap_len) {
    if (haplotypes < 1 || batch < 1 || max_hap_len < 1) return WN_ERR_BAD_SHAPE;
    if (haplotypes > kRMaxHaplotypes || batch > 65535 || max_hap_len > kPaMaxRef) return WN_ERR_UNSUPPORTED;
    return WN_OK;
}

}  // namespace wn
using namespace wn;

int wn_haplotype_windows(const unsigned char* call, const unsigned char* ins_len, const unsigned char* ins_bases, const int* reference,
                         const int* lo, const int* ref_lengths, const int* strand, int haplotypes, int batch, int reference_len, int max_ins,
                         int max_hap_ops, int* labels, int* lengths, unsigned char* ops, int* ops_len, signed char* used, int* bad,
                         wn_stream_t stream) {
    if (haplotypes < 1 || batch < 1 || reference_len < 1 || max_ins < 0 || max_hap_ops < 1) return WN_ERR_BAD_SHAPE;
    if (haplotypes > kRMaxHaplotypes || batch > 65535 || reference_len > kMaxReference || max_ins > kMaxIns || max_hap_ops > kPaMaxRef)
        return WN_ERR_UNSUPPORTED;
    if (!call || !ins_len || (max_ins > 0 && !ins_bases) || !reference || !lo || !ref_lengths || !strand || !labels || !lengths || !ops ||
        !ops_len || !used)
        return WN_ERR_NULL;
    WindowArgs a = {};
    a.call = call; a.ins_len = ins_len; a.ins_bases = ins_bases; a.reference = reference; a.lo = lo; a.ref_len = ref_lengths; a.strand = strand;
    a.labels = labels; a.lengths = lengths; a.ops = ops; a.ops_len = ops_len; a.used = used; a.bad = bad;
    a.H = haplotypes; a.B = batch; a.R = reference_len; a.max_ins = max_ins; a.cap = max_hap_ops;
    hipLaunchKernelGGL(haplotype_windows_kernel, dim3(batch, haplotypes), dim3(kPThreads), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "haplotype_windows");
    return WN_OK;
}

// three int32 per haplotype index 0..max_hap_len and read
size_t wn_lift_ops_workspace_bytes(int batch, int max_hap_len) {
    if (check_lift_shape(1, batch, max_hap_len) != WN_OK) return 0;
    return (size_t)batch * 3 * ((size_t)max_hap_len + 1) * sizeof(int);
}

int wn_lift_ops(const unsigned char* a_ops, long long a_hap_stride, long long a_stride, const int* a_ops_len, int a_max_ops,
                const unsigned char* hap_ops, long long hap_hap_stride, long long hap_stride, const int* hap_ops_len, const int* hap_lengths,
                int max_hap_ops, int max_hap_len, const signed char* used, const int* pick, const int* ref, long long ref_stride,
                const int* ref_lengths, const int* query, long long query_stride, const int* query_lengths, int haplotypes, int batch,
                int max_ref_len, int max_query_len, int max_ops, int match, int mismatch, int gap_open, int gap_extend, int end_gaps_free,
                unsigned char* ops, long long ops_stride, int* ops_len, int* score, int* stats, void* workspace, size_t workspace_bytes,
                int* bad, wn_stream_t stream) {
    if (const int s = check_lift_shape(haplotypes, batch, max_hap_len); s == WN_ERR_BAD_SHAPE) return s;
    if (a_max_ops < 1 || max_hap_ops < 1 || max_ref_len < 1 || max_query_len < 1 || max_ops < 1 || a_hap_stride < 0 || a_stride < 0 ||
        hap_hap_stride < 0 || hap_stride < 0 || ref_stride < 0 || query_stride < 0 || ops_stride < 0 || (end_gaps_free != 0 && end_gaps_free != 1))
        return WN_ERR_BAD_SHAPE;
    if (const int s = check_lift_shape(haplotypes, batch, max_hap_len)) return s;
    if (a_max_ops > kPaMaxOps || max_hap_ops > kPaMaxRef || max_ref_len > kPaMaxRef || max_query_len > kPaMaxQuery || max_ops > kPaMaxOps)
        return WN_ERR_UNSUPPORTED;
    if (const int s = check_affine_costs(match, mismatch, gap_open, gap_extend)) return s;
    if (!a_ops || !a_ops_len || !hap_ops || !hap_ops_len || !hap_lengths || !used || !pick || !ref || !ref_lengths || !query || !query_lengths ||
        !ops || !ops_len || !score || !stats || !workspace)
        return WN_ERR_NULL;
    if (workspace_bytes < wn_lift_ops_workspace_bytes(batch, max_hap_len) || (reinterpret_cast<uintptr_t>(workspace) & 3))
        return WN_ERR_WORKSPACE;
    LiftArgs a = {};
    a.a_ops = a_ops; a.a_len = a_ops_len; a.h_ops = hap_ops; a.h_len = hap_ops_len; a.hap_len = hap_lengths; a.used = used; a.pick = pick;
    a.ref = ref; a.ref_len = ref_lengths; a.query = query; a.query_len = query_lengths; a.out = ops; a.out_len = ops_len; a.score = score;
    a.stats = stats; a.work = (int*)workspace; a.bad = bad;
    a.a_hap_stride = a_hap_stride; a.a_stride = a_stride; a.h_hap_stride = hap_hap_stride; a.h_stride = hap_stride; a.ref_stride = ref_stride;
    a.query_stride = query_stride; a.out_stride = ops_stride;
    a.H = haplotypes; a.B = batch; a.N = max_ref_len; a.M = max_query_len; a.a_max_ops = a_max_ops; a.max_hap_ops = max_hap_ops;
    a.max_hap_len = max_hap_len; a.max_ops = max_ops;
    a.match = match; a.mismatch = mismatch; a.gap_open = gap_open; a.gap_extend = gap_extend; a.free_ends = end_gaps_free;
    hipLaunchKernelGGL(lift_ops_kernel, dim3(batch), dim3(kPThreads), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "lift_ops");
    return WN_OK;
}
