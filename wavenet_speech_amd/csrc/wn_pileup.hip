// Pileup, consensus and variant calls from mapped reads: walks the op string wn_pair_align wrote for a
// (reference window, read) pair and adds what the read shows at every forward-strand position of the reference into tables over
// the reference; then calls a consensus base and an insertion per position by integer rules and writes the consensus row.
//
//   pileup_kernel          grid (batch), 256 threads, ONE WORKGROUP PER READ: the walk of wn_opscan.h (validate_ops with qual <= 93
//                          as its own check, then a second pass by hand over the same loader and scan), plus the adds.  A
//                          reverse-strand read is WALKED BACK TO FRONT: walk index w is column n - 1 - w, query index
//                          n_query - 1 - j, label 5 - v.  Every column, and every insertion run with its slot order, then arrives
//                          in forward orientation, and the forward position of a column is lo + i on both strands.
//                          Pass 2 rescans.  An aligned column or a deletion adds 1 to counts[lo + i][strand][.].  An op-4 column
//                          is slot w - prev - 1 of the insertion after lo + i - 1, prev the last column before it that is not an
//                          op 4 (a third ballot: the highest lane below, the waves' last ones through LDS, a running value from
//                          tile to tile).  The first column after a run adds the run's length, w - 1 - prev.  All adds are
//                          32-bit integer atomics to global memory: integer addition commutes, so two runs are bitwise identical.
//   consensus_call_kernel  grid (tiles of 256 positions), one position per thread: the call, the insertion, the flags, and the
//                          tile's emitted total (block_scan of wn_wave_dev.h).
//   consensus_scan_kernel  one workgroup: the exclusive prefix sum of the tile totals in place, the grand total to offsets[R].
//   consensus_emit_kernel  grid (tiles): offsets[p] = the tile's offset + the scan within the tile, then the labels.
// Three launches in stream order; no workgroup waits on another.  No floating point, no workspace, no scratch.  No value of an op,
// a label, a length, a position or a qual is used as an index before it is checked.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_opscan.h"

namespace wn {

constexpr int kUMaxDen = 1 << 15;
constexpr int kUScanTile = kPThreads;         // positions per workgroup of the call and emit kernels

struct PileupArgs {
    ReadBatch r;
    int* counts;                        // [R][2][6]
    int* ins_lengths;                   // [R][max_ins + 1]
    int* ins_bases;                     // [R][max_ins][4], nullptr with max_ins = 0
    signed char* used;
    int* bad;
    int max_ins;
};

__global__ __launch_bounds__(kPThreads) void pileup_kernel(const PileupArgs a) {
    __shared__ int s_slot[2][2][kPWaves];
    __shared__ int s_lo, s_hi, s_bad;
    __shared__ int s_last[2][kPWaves];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    const int strand = a.r.strand[b], n_ref = a.r.ref_len[b];
    if (read_skipped(strand, n_ref, a.r.keep, b)) {                  // nothing else of the read is looked at
        if (tid == 0) a.used[b] = 0;
        return;
    }
    const int n_ops = a.r.ops_len[b], n_query = a.r.query_len[b], lo = a.r.lo[b];
    const bool header_ok = head_ok(strand, n_ref, lo >= 0 && (long long)lo + n_ref <= a.r.R, n_query, a.r.M, n_ops, a.r.max_ops);
    const OpRow row = op_row(a.r.ops + (long long)b * a.r.ops_stride, header_ok, n_ops, n_ref, n_query, strand == 1);
    const int n = row.n;
    const bool rev = row.rev;
    const int* query = a.r.query + (long long)b * a.r.query_stride;
    const unsigned char* qual = a.r.qual ? a.r.qual + (long long)b * a.r.qual_stride : nullptr;

    validate_begin(tid, header_ok, &s_lo, &s_hi, &s_bad);
    __syncthreads();

    // ---- pass 1: validate, first / last aligned walk index, totals
    OpWalk walk{s_slot};
    const OpSpan span = validate_ops(row, tid, &walk, &s_lo, &s_hi, &s_bad, [&](const OpCol& c, bool, bool in_query) {
        return !(in_query && qual && qual[rev ? n_query - 1 - c.j : c.j] >= kPQualRows);
    });
    if (span.bad) {
        if (tid == 0) a.used[b] = -1;
        report_bad(tid, a.bad);
        return;
    }
    const int first = span.first, last = span.last;
    if (tid == 0) a.used[b] = last >= 0 ? 1 : 0;
    if (last < 0) return;                                            // no aligned column: end columns only

    // ---- pass 2: the adds.  Ops, labels and quals are loaded again; every index below was checked in pass 1 on the same words (the
    // inputs must not change while the launch runs: stream order gives that) and is checked again before it is used.  The loop is
    // this kernel's own: the third ballot's wave values go to LDS before the barrier inside the scan
    const unsigned long long below = (1ull << lane) - 1ull;
    const int ins_cols = a.max_ins + 1;
    int last_non4 = -1;
    walk.base_ref = walk.base_query = 0;
    for (int t0 = 0; t0 < n; t0 += kPThreads) {
        OpCol c = row.load(t0 + tid);
        const int w = c.w, op = c.op, slot = walk.tile & 1;
        const unsigned long long m_non4 = __ballot(c.active && op != 4);
        if (lane == 0) s_last[slot][wave] = m_non4 ? t0 + wave * 64 + 63 - __clzll((long long)m_non4) : -1;
        walk.scan(&c, tid);                                          // the barrier is in here
        const int i = c.i, j = c.j;
        int prev = last_non4;                                        // the last walk index before w whose op is not 4
#pragma unroll
        for (int v = 0; v < kPWaves; ++v) {
            const int l = s_last[slot][v];
            if (l >= 0) {
                last_non4 = l;
                if (v < wave) prev = l;
            }
        }
        if (m_non4 & below) prev = t0 + wave * 64 + 63 - __clzll((long long)(m_non4 & below));
        if (!c.active || w < first || w > last) continue;            // end columns enter nothing
        int col = 5;                                                 // of the query label: 0..3 a base on the forward strand, 5 other
        if (c.is_query && j < n_query) {
            const int jq = rev ? n_query - 1 - j : j;
            const int v = query[jq];
            if (v >= 1 && v <= 4 && !(qual && (int)qual[jq] < a.r.min_qual)) col = rev ? 4 - v : v - 1;
        }
        if (op != 4) {
            if (i < n_ref) atomicAdd(a.counts + ((size_t)(lo + i) * 2 + strand) * 6 + (op == 3 ? 4 : col), 1);
            if (w > first && prev != w - 1 && i >= 1 && i <= n_ref) {                             // an insertion run ends here
                const int len = w - 1 - prev;                        // prev >= first: len >= 1
                atomicAdd(a.ins_lengths + (size_t)(lo + i - 1) * ins_cols + (len < ins_cols ? len : ins_cols) - 1, 1);
            }
        } else {
            const int k = w - prev - 1;                              // first < w < last: prev >= first, k >= 0
            if (k < a.max_ins && col < 4 && i >= 1 && i <= n_ref)
                atomicAdd(a.ins_bases + ((size_t)(lo + i - 1) * a.max_ins + k) * 4 + col, 1);
        }
    }
}

struct CallArgs {
    const int* counts;
    const int* ins_lengths;
    const int* ins_bases;
    const int* reference;
    unsigned char* call;
    unsigned char* ins_len;
    unsigned char* ins_out;             // [R][max_ins], nullptr with max_ins = 0
    unsigned char* flags;
    int* alt_count;                     // [R][2]
    int* tile_offsets;
    int R, max_ins, min_depth, num, den;
};

__global__ __launch_bounds__(kPThreads) void consensus_call_kernel(const CallArgs a) {
    __shared__ int s_w[kPWaves];
    const int tid = threadIdx.x;
    const long long p = (long long)blockIdx.x * kUScanTile + tid;
    int emitted = 0;
    if (p < a.R) {
        const int* c = a.counts + p * 12;
        int cnt[5], fwd[5];
        long long d = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            fwd[k] = c[k];
            cnt[k] = c[k] + c[6 + k];
            d += cnt[k];
        }
        int r = a.reference[p];
        r = r < 0 ? 0 : r > 255 ? 255 : r;
        const bool ref_is_base = r >= 1 && r <= 4;
        int flags = 0, called = ref_is_base ? r - 1 : -1;            // the candidate whose counts are reported, -1 none
        int label = r;
        if (d < a.min_depth) {
            flags |= WN_CALL_LOW_DEPTH;
        } else {
            int best = 0, best_count = cnt[0], ref_count = -1;       // selects, not indexed registers: no scratch
#pragma unroll
            for (int k = 1; k < 5; ++k) {
                best = cnt[k] > best_count ? k : best;
                best_count = cnt[k] > best_count ? cnt[k] : best_count;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) ref_count = k == r - 1 ? cnt[k] : ref_count;
            if (ref_count == best_count) best = r - 1;               // ties go to the reference base first
            if ((long long)best_count * a.den > (long long)a.num * d) {
                called = best;
                label = best < 4 ? best + 1 : 0;
                if (best == 4) flags |= WN_CALL_DELETION;
                else if (label != r) flags |= WN_CALL_SUBSTITUTION;
            } else {
                flags |= WN_CALL_AMBIGUOUS;
            }
        }
        int alt0 = 0, alt1 = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            alt0 = k == called ? fwd[k] : alt0;
            alt1 = k == called ? cnt[k] - fwd[k] : alt1;
        }
        // the insertion after p
        const int* il = a.ins_lengths + p * (a.max_ins + 1);
        long long n_ins = 0;
        int len = 0, len_count = -1;
        for (int k = 0; k <= a.max_ins; ++k) {
            const int v = il[k];
            n_ins += v;
            if (v > len_count) { len_count = v; len = k + 1 < a.max_ins ? k + 1 : a.max_ins; }
        }
        int n_out = 0;
        if (d >= a.min_depth && n_ins * a.den > (long long)a.num * d) {
            bool open = true;
            for (int k = 0; k < a.max_ins; ++k) {
                const int* s = a.ins_bases + (p * a.max_ins + k) * 4;
                int bb = 0, bc = s[0];
#pragma unroll
                for (int q = 1; q < 4; ++q) {
                    const int v = s[q];
                    bb = v > bc ? q : bb;
                    bc = v > bc ? v : bc;
                }
                open = open && k < len && bc > 0;                    // the first slot with no count ends the insertion
                a.ins_out[p * a.max_ins + k] = (unsigned char)(open ? bb + 1 : 0);
                n_out += open ? 1 : 0;
            }
        } else {
            for (int k = 0; k < a.max_ins; ++k) a.ins_out[p * a.max_ins + k] = 0;
        }
        if (n_out > 0) flags |= WN_CALL_INSERTION;
        a.call[p] = (unsigned char)label;
        a.ins_len[p] = (unsigned char)n_out;
        a.flags[p] = (unsigned char)flags;
        a.alt_count[2 * p] = alt0;
        a.alt_count[2 * p + 1] = alt1;
        emitted = (label != 0 ? 1 : 0) + n_out;
    }
    int total;
    block_scan<kPWaves>(emitted, tid, s_w, &total);
    if (tid == 0) a.tile_offsets[blockIdx.x] = total;
}

// one workgroup: thread t owns `chunk` consecutive tiles
__global__ __launch_bounds__(kPThreads) void consensus_scan_kernel(int* tile_offsets, int n_tiles, int* total_out) {
    __shared__ int s_w[kPWaves];
    const int tid = threadIdx.x;
    const int chunk = (n_tiles + kPThreads - 1) / kPThreads;
    const int t0 = tid * chunk < n_tiles ? tid * chunk : n_tiles;
    const int t1 = t0 + chunk < n_tiles ? t0 + chunk : n_tiles;
    int sum = 0;
    for (int t = t0; t < t1; ++t) sum += tile_offsets[t];
    int total;
    int run = block_scan<kPWaves>(sum, tid, s_w, &total);
    for (int t = t0; t < t1; ++t) {
        const int v = tile_offsets[t];
        tile_offsets[t] = run;
        run += v;
    }
    if (tid == 0) *total_out = total;
}

struct EmitArgs {
    const unsigned char* call;
    const unsigned char* ins_len;
    const unsigned char* ins_out;
    const int* tile_offsets;
    int* offsets;
    int* consensus;
    int R, max_ins, capacity;
};

__global__ __launch_bounds__(kPThreads) void consensus_emit_kernel(const EmitArgs a) {
    __shared__ int s_w[kPWaves];
    const int tid = threadIdx.x;
    const long long p = (long long)blockIdx.x * kUScanTile + tid;
    int label = 0, n_out = 0;
    if (p < a.R) {
        label = a.call[p];
        n_out = a.ins_len[p];
        n_out = n_out < a.max_ins ? n_out : a.max_ins;
    }
    int total;
    long long at = (long long)a.tile_offsets[blockIdx.x] + block_scan<kPWaves>((label != 0 ? 1 : 0) + n_out, tid, s_w, &total);
    if (p >= a.R) return;
    a.offsets[p] = (int)at;
    if (label != 0) {
        if (at >= 0 && at < a.capacity) a.consensus[at] = label;
        ++at;
    }
    for (int k = 0; k < n_out; ++k, ++at)
        if (at >= 0 && at < a.capacity) a.consensus[at] = a.ins_out[p * a.max_ins + k];
}

}  // namespace wn
using namespace wn;

int wn_pileup(const unsigned char* ops, long long ops_stride, const int* ops_len, const int* lo, const int* ref_lengths,
              const int* strand, const int* query, long long query_stride, const int* query_lengths, const unsigned char* qual,
              long long qual_stride, const unsigned char* keep, int batch, int max_query_len, int max_ops, int reference_len,
              int min_qual, int max_ins, int* counts, int* ins_lengths, int* ins_bases, signed char* used, int* bad,
              wn_stream_t stream) {
    PileupArgs a = {};
    a.r = read_batch(ops, ops_stride, ops_len, lo, ref_lengths, strand, query, query_stride, query_lengths, qual, qual_stride, keep, batch,
                     max_query_len, max_ops, reference_len, min_qual);
    if (const int s = check_read_batch(a.r, max_ins >= 0, min_qual < kPQualRows && max_ins <= kMaxIns,
                                       counts && ins_lengths && used && (max_ins <= 0 || ins_bases)))
        return s;
    a.counts = counts; a.ins_lengths = ins_lengths; a.ins_bases = ins_bases; a.used = used; a.bad = bad; a.max_ins = max_ins;
    hipLaunchKernelGGL(pileup_kernel, dim3(batch), dim3(kPThreads), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "pileup");
    return WN_OK;
}

static int consensus_shape(int reference_len, int max_ins) {
    if (reference_len < 1 || max_ins < 0) return WN_ERR_BAD_SHAPE;
    if (reference_len > kMaxReference || max_ins > kMaxIns) return WN_ERR_UNSUPPORTED;
    return WN_OK;
}

int wn_consensus_call(const int* counts, const int* ins_lengths, const int* ins_bases, const int* reference, int reference_len,
                      int max_ins, int min_depth, int num, int den, unsigned char* call, unsigned char* ins_len,
                      unsigned char* ins_out, unsigned char* flags, int* alt_count, int* tile_offsets, int* total,
                      wn_stream_t stream) {
    if (reference_len < 1 || max_ins < 0 || min_depth < 1 || num < 0 || den < 1) return WN_ERR_BAD_SHAPE;
    if (const int s = consensus_shape(reference_len, max_ins)) return s;
    if (den > kUMaxDen || num > den) return WN_ERR_UNSUPPORTED;
    if (!counts || !ins_lengths || !reference || !call || !ins_len || !flags || !alt_count || !tile_offsets || !total)
        return WN_ERR_NULL;
    if (max_ins > 0 && (!ins_bases || !ins_out)) return WN_ERR_NULL;
    CallArgs a = {};
    a.counts = counts; a.ins_lengths = ins_lengths; a.ins_bases = ins_bases; a.reference = reference;
    a.call = call; a.ins_len = ins_len; a.ins_out = ins_out; a.flags = flags; a.alt_count = alt_count; a.tile_offsets = tile_offsets;
    a.R = reference_len; a.max_ins = max_ins; a.min_depth = min_depth; a.num = num; a.den = den;
    const int n_tiles = cdiv(reference_len, kUScanTile);
    hipLaunchKernelGGL(consensus_call_kernel, dim3(n_tiles), dim3(kPThreads), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "consensus_call");
    hipLaunchKernelGGL(consensus_scan_kernel, dim3(1), dim3(kPThreads), 0, (hipStream_t)stream, tile_offsets, n_tiles, total);
    WN_HIP(hipGetLastError(), "consensus_scan");
    return WN_OK;
}

int wn_consensus_emit(const unsigned char* call, const unsigned char* ins_len, const unsigned char* ins_out,
                      const int* tile_offsets, int reference_len, int max_ins, int capacity, int* offsets, int* consensus,
                      wn_stream_t stream) {
    if (reference_len < 1 || max_ins < 0 || capacity < 0) return WN_ERR_BAD_SHAPE;
    if (const int s = consensus_shape(reference_len, max_ins)) return s;
    if (!call || !ins_len || !tile_offsets || !offsets) return WN_ERR_NULL;
    if ((max_ins > 0 && !ins_out) || (capacity > 0 && !consensus)) return WN_ERR_NULL;
    EmitArgs a = {};
    a.call = call; a.ins_len = ins_len; a.ins_out = ins_out; a.tile_offsets = tile_offsets; a.offsets = offsets;
    a.consensus = consensus; a.R = reference_len; a.max_ins = max_ins; a.capacity = capacity;
    hipLaunchKernelGGL(consensus_emit_kernel, dim3(cdiv(reference_len, kUScanTile)), dim3(kPThreads), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "consensus_emit");
    return WN_OK;
}
