// Quality calibration tables and the error profile of aligned reads: walks the op string wn_pair_align
// wrote for a (reference, query) pair, decides for every query base whether it was a match, a mismatch or an insertion, and
// tabulates that against the quality and the dwell the caller claims for the base; reference labels against a gap are the
// deletions.  All arithmetic is integer.
//
//   quality_profile_kernel   grid (batch), 256 threads, ONE WORKGROUP PER READ, two passes over the read's ops in tiles of 256
//                            columns.  Column c of a tile belongs to thread c % 256.  Its reference index i_c / query index j_c
//                            is the number of earlier columns that consume a reference / query label: per tile one wave ballot
//                            each, the popcount of the lanes below, the four wave totals through LDS (two slots, by tile
//                            parity: one barrier per tile), and a running base carried from tile to tile (tile_scan in
//                            wn_opscan.h, whose header says what a valid op row is; pass 1 below is KEPT BY HAND: section 7u).
//                            Pass 1 validates every column (op code, i_c / j_c against the lengths BEFORE the loads, the labels
//                            against [0, classes), op 1 / 2 against the labels, qual <= 93, dwell >= 0), finds the first and
//                            last match-or-mismatch column and the two totals.  A bad read stops there: its rows are cleared,
//                            it is counted, nothing else is touched.
//                            Pass 2 rescans, writes outcome / ref_index with plain stores, counts the five column kinds with
//                            ballots, and adds into three tables held in LDS ((classes + 1)^2 + 94 * 3 + 33 * 3 dwords, at
//                            most 18.4 KB) with LDS integer adds.  At the end the non-zero entries go to the global int64 tables
//                            with 64-bit integer atomic adds: integer addition commutes, so two runs are bitwise identical.
//
// No floating point, no workspace, no scratch.  No value of an op, a label, a length, a qual or a dwell is used as an index
// before it is checked.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"
#include "wn_opscan.h"
#include <limits.h>

namespace wn {

constexpr int kPMaxClasses = 64;
constexpr int kPDwellRows = 33;               // dwell 0..31, and 32 for everything above
constexpr int kPTableMax = (kPMaxClasses + 1) * (kPMaxClasses + 1) + 3 * kPQualRows + 3 * kPDwellRows;

struct ProfileArgs {
    const unsigned char* ops;           // row b at ops + b * ops_stride
    const int* ops_len;
    const int* ref;
    const int* ref_len;
    const int* query;
    const int* query_len;
    const unsigned char* qual;          // or nullptr
    const int* dwell;                   // or nullptr
    long long ops_stride, ref_stride, query_stride, qual_stride, dwell_stride;
    unsigned long long* q_counts;       // [94][3] or nullptr
    unsigned long long* dwell_counts;   // [33][3] or nullptr
    unsigned long long* confusion;      // [C + 1][C + 1] or nullptr
    int* read_counts;                   // [B][5] or nullptr
    unsigned char* outcome;             // [B][M] or nullptr
    int* ref_index;                     // [B][M] or nullptr
    int* bad;
    int B, N, M, max_ops, C, count_ends;
};

__global__ __launch_bounds__(kPThreads) void quality_profile_kernel(const ProfileArgs a) {
    __shared__ int s_table[kPTableMax];
    __shared__ int s_slot[2][2][kPWaves];
    __shared__ int s_lo, s_hi, s_bad;
    __shared__ int s_count[5];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int C1 = a.C + 1;
    int* const s_conf = s_table;
    int* const s_qual = s_table + C1 * C1;
    int* const s_dwell = s_qual + 3 * kPQualRows;
    const int table_size = C1 * C1 + 3 * kPQualRows + 3 * kPDwellRows;

    const int n_ops = a.ops_len[b], n_ref = a.ref_len[b], n_query = a.query_len[b];
    const bool lengths_ok = n_ops >= 0 && n_ops <= a.max_ops && n_ref >= 0 && n_ref <= a.N && n_query >= 0 && n_query <= a.M;
    const unsigned char* ops = a.ops + (long long)b * a.ops_stride;
    const int* ref = a.ref + (long long)b * a.ref_stride;
    const int* query = a.query + (long long)b * a.query_stride;
    const unsigned char* qual = a.qual ? a.qual + (long long)b * a.qual_stride : nullptr;
    const int* dwell = a.dwell ? a.dwell + (long long)b * a.dwell_stride : nullptr;
    const int n = lengths_ok ? n_ops : 0;                            // nothing of a read with a bad length is looked at

    for (int k = tid; k < table_size; k += kPThreads) s_table[k] = 0;
    if (tid == 0) { s_lo = INT_MAX; s_hi = -1; s_bad = lengths_ok ? 0 : 1; }
    if (tid < 5) s_count[tid] = 0;
    __syncthreads();

    // ---- pass 1: validate, first / last match-or-mismatch column, totals
    bool ok = true;
    int lo = INT_MAX, hi = -1, base_ref = 0, base_query = 0, tile = 0;
    for (int t0 = 0; t0 < n; t0 += kPThreads, ++tile) {
        const int c = t0 + tid;
        const bool active = c < n;
        const int op = active ? (int)ops[c] : 0;
        const bool is_ref = op >= 1 && op <= 3, is_query = op == 1 || op == 2 || op == 4;
        int i, j;
        tile_scan(is_ref, is_query, tid, s_slot[tile & 1], &base_ref, &base_query, &i, &j);
        if (!active) continue;
        if (op < 1 || op > 4) { ok = false; continue; }
        int r = -1, q = -2;
        if (is_ref) {
            if (i < n_ref) { r = ref[i]; ok = ok && r >= 0 && r < a.C; } else ok = false;
        }
        if (is_query) {
            if (j < n_query) {
                q = query[j];
                ok = ok && q >= 0 && q < a.C;
                if (qual && qual[j] >= kPQualRows) ok = false;
                if (dwell && dwell[j] < 0) ok = false;
            } else ok = false;
        }
        if (op <= 2) {
            if ((op == 1) != (r == q)) ok = false;                   // r = -1, q = -2 where a label was not loaded: ok is false already
            lo = c < lo ? c : lo;
            hi = c > hi ? c : hi;
        }
    }
    if (base_ref != n_ref || base_query != n_query) ok = false;      // the ops consume exactly the labels
    if (!ok) atomicOr(&s_bad, 1);
    if (hi >= 0) { atomicMin(&s_lo, lo); atomicMax(&s_hi, hi); }
    __syncthreads();
    const bool bad = s_bad != 0;
    const long long row = (long long)b * a.M;

    if (bad) {
        for (int j = tid; j < a.M; j += kPThreads) {
            if (a.outcome) a.outcome[row + j] = 0;
            if (a.ref_index) a.ref_index[row + j] = -1;
        }
        if (tid < 5 && a.read_counts) a.read_counts[b * 5 + tid] = -1;
        if (tid == 0 && a.bad) atomicAdd(a.bad, 1);
        return;
    }

    // ---- pass 2: outcomes, counts, tables.  The labels, quals and dwells are loaded again and index LDS on the strength of pass 1's
    // check of the same words: the inputs must not change while the launch runs (stream order gives that)
    const int first = a.count_ends ? 0 : s_lo, last = a.count_ends ? INT_MAX : s_hi;   // no such column: first > every c
    int n_match = 0, n_mismatch = 0, n_ins = 0, n_del = 0, n_end = 0;
    base_ref = base_query = 0;
    tile = 0;
    for (int t0 = 0; t0 < n; t0 += kPThreads, ++tile) {
        const int c = t0 + tid;
        const bool active = c < n;
        const int op = active ? (int)ops[c] : 0;
        const bool is_ref = op >= 1 && op <= 3, is_query = op == 1 || op == 2 || op == 4;
        int i, j;
        tile_scan(is_ref, is_query, tid, s_slot[tile & 1], &base_ref, &base_query, &i, &j);
        const bool end = c < first || c > last;
        const bool in_ref = is_ref && i < n_ref, in_query = is_query && j < n_query;      // held in pass 1; kept before the loads
        const bool pair = op <= 2 && in_ref && in_query, ins = op == 4 && in_query && !end, del = op == 3 && in_ref && !end;
        n_match += __popcll(__ballot(pair && op == 1));
        n_mismatch += __popcll(__ballot(pair && op == 2));
        n_ins += __popcll(__ballot(ins));
        n_del += __popcll(__ballot(del));
        n_end += __popcll(__ballot(active && op >= 3 && end));
        if (in_query) {
            if (a.outcome) a.outcome[row + j] = (unsigned char)(op <= 2 ? op : end ? 4 : 3);
            if (a.ref_index) a.ref_index[row + j] = op <= 2 ? i : -1;
        }
        const int r = in_ref ? ref[i] : 0, q = in_query ? query[j] : 0;
        if (pair || ins) {
            const int col = pair ? op - 1 : 2;
            if (a.confusion) atomicAdd(&s_conf[(pair ? r : a.C) * C1 + q], 1);
            if (a.q_counts) atomicAdd(&s_qual[3 * (int)qual[j] + col], 1);
            if (a.dwell_counts) {
                const int d = dwell[j];
                atomicAdd(&s_dwell[3 * (d < kPDwellRows - 1 ? d : kPDwellRows - 1) + col], 1);
            }
        } else if (del) {
            if (a.confusion) atomicAdd(&s_conf[r * C1 + a.C], 1);
        }
    }
    for (int j = n_query + tid; j < a.M; j += kPThreads) {
        if (a.outcome) a.outcome[row + j] = 0;
        if (a.ref_index) a.ref_index[row + j] = -1;
    }
    if (lane == 0) {
        atomicAdd(&s_count[0], n_match);
        atomicAdd(&s_count[1], n_mismatch);
        atomicAdd(&s_count[2], n_ins);
        atomicAdd(&s_count[3], n_del);
        atomicAdd(&s_count[4], n_end);
    }
    __syncthreads();
    if (tid < 5 && a.read_counts) a.read_counts[b * 5 + tid] = s_count[tid];
    for (int k = tid; k < table_size; k += kPThreads) {
        const int v = s_table[k];
        if (v == 0) continue;
        if (k < C1 * C1) {
            if (a.confusion) atomicAdd(a.confusion + k, (unsigned long long)v);
        } else if (k < C1 * C1 + 3 * kPQualRows) {
            if (a.q_counts) atomicAdd(a.q_counts + (k - C1 * C1), (unsigned long long)v);
        } else {
            if (a.dwell_counts) atomicAdd(a.dwell_counts + (k - C1 * C1 - 3 * kPQualRows), (unsigned long long)v);
        }
    }
}

}  // namespace wn
using namespace wn;

int wn_quality_profile(const unsigned char* ops, long long ops_stride, const int* ops_len, const int* ref, long long ref_stride,
                       const int* ref_lengths, const int* query, long long query_stride, const int* query_lengths,
                       const unsigned char* qual, long long qual_stride, const int* dwell, long long dwell_stride, int batch,
                       int max_ref_len, int max_query_len, int max_ops, int classes, int count_ends, long long* q_counts,
                       long long* dwell_counts, long long* confusion, int* read_counts, unsigned char* outcome, int* ref_index,
                       int* bad, wn_stream_t stream) {
    if (batch < 1 || max_ref_len < 1 || max_query_len < 1 || max_ops < 1 || classes < 1) return WN_ERR_BAD_SHAPE;
    if (ops_stride < 0 || ref_stride < 0 || query_stride < 0 || qual_stride < 0 || dwell_stride < 0) return WN_ERR_BAD_SHAPE;
    if (count_ends < 0 || count_ends > 1) return WN_ERR_BAD_SHAPE;
    if (classes > kPMaxClasses || max_query_len > kPaMaxQuery || max_ref_len > kPaMaxRef) return WN_ERR_UNSUPPORTED;
    if (max_ops > max_ref_len + max_query_len || batch > 65535) return WN_ERR_UNSUPPORTED;
    if (!ops || !ops_len || !ref || !ref_lengths || !query || !query_lengths) return WN_ERR_NULL;
    if ((q_counts != nullptr) != (qual != nullptr) || (dwell_counts != nullptr) != (dwell != nullptr)) return WN_ERR_NULL;
    if (!q_counts && !dwell_counts && !confusion && !read_counts && !outcome && !ref_index) return WN_ERR_NULL;
    ProfileArgs a = {};
    a.ops = ops; a.ops_len = ops_len; a.ref = ref; a.ref_len = ref_lengths; a.query = query; a.query_len = query_lengths;
    a.qual = qual; a.dwell = dwell;
    a.ops_stride = ops_stride; a.ref_stride = ref_stride; a.query_stride = query_stride; a.qual_stride = qual_stride;
    a.dwell_stride = dwell_stride;
    a.q_counts = (unsigned long long*)q_counts; a.dwell_counts = (unsigned long long*)dwell_counts;
    a.confusion = (unsigned long long*)confusion;
    a.read_counts = read_counts; a.outcome = outcome; a.ref_index = ref_index; a.bad = bad;
    a.B = batch; a.N = max_ref_len; a.M = max_query_len; a.max_ops = max_ops; a.C = classes; a.count_ends = count_ends;
    hipLaunchKernelGGL(quality_profile_kernel, dim3(batch), dim3(kPThreads), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "quality_profile");
    return WN_OK;
}
