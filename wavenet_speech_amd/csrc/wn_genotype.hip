// Genotype likelihoods and diploid calls from mapped reads: the walk of wn_opscan.h with pileup_kernel's
// checks, adding quality-weighted evidence instead of counts, and a call per position over the 15 unordered pairs of {A, G, C, T,
// deletion}.
//
//   pileup_evidence_kernel  grid (batch), 256 threads, ONE WORKGROUP PER READ: validate_ops with pileup_kernel's window and qual
//                           checks, so that `used` and *bad agree with it, then walk_ops (a reverse-strand read walked back to
//                           front), without the third ballot -- insertion slots are not needed.  The
//                           weight table W[3][94] travels BY VALUE in the kernel-argument struct and is copied to LDS once: no
//                           allocation, no copy call, graph-capturable.  A column that pileup_kernel counts under base k adds
//                           W[HOM, HET, MIS][min(q, cap[b])] to evidence[lo + i][k][0..2], a deletion column W[.][min(gap_qual,
//                           cap[b])] under allele 4: three 64-bit integer atomics to 24 contiguous bytes.  Integer addition
//                           commutes, so two runs are bitwise identical.
//   genotype_call_kernel    grid (tiles of 256 positions), one position per thread: the 15 costs from 15 loaded int64 with selects
//                           (fully unrolled: no indexed registers), the least and the second least, the alleles and flags, and the
//                           insertion genotype with its sequence.  No scan and no consensus row: a diploid call has no single
//                           consensus.
// No floating point, no workspace, no scratch.  No value of an op, a label, a length, a position, a qual or a cap is used as an
// index before it is checked; a capped qual is min(q, cap) with q <= 93 checked, so at most 93 whatever the cap holds.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_opscan.h"

namespace wn {

constexpr int kGMaxWeight = 1 << 20;
constexpr int kGMaxPrior = 1 << 30;
constexpr int kGWeights = 3 * kPQualRows;     // rows HOM, HET, MIS
constexpr int kGTile = kPThreads;             // positions per workgroup of the call kernel

struct EvidenceArgs {
    ReadBatch r;
    const unsigned char* cap;           // or nullptr
    unsigned long long* evidence;       // [R][5][3]
    signed char* used;
    int* bad;
    int flat_qual, gap_qual;
    int w[kGWeights];                   // by value: 1128 bytes of the kernel-argument segment
};

__global__ __launch_bounds__(kPThreads) void pileup_evidence_kernel(const EvidenceArgs a) {
    __shared__ int s_slot[2][2][kPWaves];
    __shared__ int s_lo, s_hi, s_bad;
    __shared__ int s_w[kGWeights];
    const int b = blockIdx.x, tid = threadIdx.x;

    const int strand = a.r.strand[b], n_ref = a.r.ref_len[b];
    if (read_skipped(strand, n_ref, a.r.keep, b)) {                  // nothing else of the read is looked at
        if (tid == 0) a.used[b] = 0;
        return;
    }
    const int n_ops = a.r.ops_len[b], n_query = a.r.query_len[b], lo = a.r.lo[b];
    const bool header_ok = head_ok(strand, n_ref, lo >= 0 && (long long)lo + n_ref <= a.r.R, n_query, a.r.M, n_ops, a.r.max_ops);
    const OpRow row = op_row(a.r.ops + (long long)b * a.r.ops_stride, header_ok, n_ops, n_ref, n_query, strand == 1);
    const bool rev = row.rev;
    const int* query = a.r.query + (long long)b * a.r.query_stride;
    const unsigned char* qual = a.r.qual ? a.r.qual + (long long)b * a.r.qual_stride : nullptr;

    for (int t = tid; t < kGWeights; t += kPThreads) s_w[t] = a.w[t];
    validate_begin(tid, header_ok, &s_lo, &s_hi, &s_bad);
    __syncthreads();

    // ---- pass 1: pileup_kernel's
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

    // ---- pass 2: the adds.  Every index below was checked in pass 1 on the same words and is checked again before it is used
    const int cap = a.cap ? (int)a.cap[b] : kPQualRows - 1;
    const int q_gap = a.gap_qual < cap ? a.gap_qual : cap;           // gap_qual and flat_qual are at most 93: checked on the host
    walk_ops(row, tid, &walk, [&](const OpCol& c) {
        const int w = c.w, i = c.i, j = c.j;
        if (!c.active || w < first || w > last || !c.is_ref || i >= n_ref) return;                // end and insertion columns enter nothing
        int k = 4, q = q_gap;
        if (c.op != 3) {
            k = 5;                                                   // `other`, as in pileup_kernel
            if (j < n_query) {
                const int jq = rev ? n_query - 1 - j : j;
                const int v = query[jq];
                const int qb = qual ? (int)qual[jq] : a.flat_qual;   // min_qual sees the uncapped qual
                if (v >= 1 && v <= 4 && !(qual && qb < a.r.min_qual)) {
                    k = rev ? 4 - v : v - 1;
                    q = qb < cap ? qb : cap;
                }
            }
        }
        if (k > 4 || q < 0 || q >= kPQualRows) return;
        unsigned long long* e = a.evidence + ((size_t)(lo + i) * 5 + k) * 3;
        atomicAdd(e, (unsigned long long)s_w[q]);
        atomicAdd(e + 1, (unsigned long long)s_w[kPQualRows + q]);
        atomicAdd(e + 2, (unsigned long long)s_w[2 * kPQualRows + q]);
    });
}

struct GenotypeArgs {
    const long long* evidence;
    const int* counts;
    const int* ins_lengths;
    const int* ins_bases;
    const int* reference;
    unsigned char* alleles;             // [R][2]
    int* gq;
    int* qual;
    unsigned char* flags;
    unsigned char* ins_copies;
    unsigned char* ins_len;
    unsigned char* ins_out;             // [R][max_ins], nullptr with max_ins = 0
    int* ins_gq;
    int* ins_qual;
    long long* costs;                   // [R][15] or nullptr
    int R, max_ins, min_depth, alt_prior, hom_g, het_g, mis_g;
};

__device__ __forceinline__ int clamp_i32(long long v) { return v > INT_MAX ? INT_MAX : (int)v; }

__global__ __launch_bounds__(kPThreads) void genotype_call_kernel(const GenotypeArgs a) {
    const long long p = (long long)blockIdx.x * kGTile + threadIdx.x;
    if (p >= a.R) return;
    const long long* ev = a.evidence + p * 15;
    long long hom[5], het[5], mis[5], mis_all = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        hom[k] = ev[3 * k];
        het[k] = ev[3 * k + 1];
        mis[k] = ev[3 * k + 2];
        mis_all += mis[k];
    }
    const int* c = a.counts + p * 12;
    long long d = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) d += (long long)c[k] + c[6 + k];
    int r = a.reference[p];
    r = r < 0 ? 0 : r > 255 ? 255 : r;
    const bool ref_is_base = r >= 1 && r <= 4;
    const long long prior = ref_is_base ? a.alt_prior : 0;           // no hom-ref genotype: no prior at all

    // the 15 genotypes (x <= y) in lexicographic order; the least by (cost, is not hom-ref, index), and the second-least cost
    long long least = LLONG_MAX, second = LLONG_MAX, cost_ref = 0;
    int best_x = 0, best_y = 0;
    bool best_is_ref = false;
    int g = 0;
#pragma unroll
    for (int x = 0; x < 5; ++x) {
#pragma unroll
        for (int y = x; y < 5; ++y, ++g) {
            const bool is_ref = x == y && x == r - 1;
            const long long like = x == y ? hom[x] + (mis_all - mis[x]) : het[x] + het[y] + (mis_all - mis[x] - mis[y]);
            const long long cost = like + (is_ref ? 0 : prior);
            if (a.costs) a.costs[p * 15 + g] = cost;
            cost_ref = is_ref ? cost : cost_ref;
            const bool wins = cost < least || (cost == least && is_ref && !best_is_ref);
            second = wins ? least : cost < second ? cost : second;
            best_x = wins ? x : best_x;
            best_y = wins ? y : best_y;
            best_is_ref = wins ? is_ref : best_is_ref;
            least = wins ? cost : least;
        }
    }
    const bool deep = d >= a.min_depth;
    int flags = 0, l0 = r, l1 = r, gq = 0, qual = 0;
    if (!deep) {
        flags = WN_CALL_LOW_DEPTH;
    } else if (ref_is_base) {
        l0 = best_x < 4 ? best_x + 1 : 0;
        l1 = best_y < 4 ? best_y + 1 : 0;
        gq = clamp_i32(second - least);
        qual = clamp_i32(cost_ref - least);
        if ((l0 != 0 && l0 != r) || (l1 != 0 && l1 != r)) flags |= WN_CALL_SUBSTITUTION;
        if (l1 == 0) flags |= WN_CALL_DELETION;                      // x <= y: the deletion, allele 4, is the second
        if (best_x != best_y) flags |= WN_CALL_HET;
    }

    // the insertion after p: 0, 1 or 2 copies
    const int* il = a.ins_lengths + p * (a.max_ins + 1);
    long long n_ins = 0;
    int len = 0, len_count = -1;
    for (int k = 0; k <= a.max_ins; ++k) {
        const int v = il[k];
        n_ins += v;
        if (v > len_count) { len_count = v; len = k + 1 < a.max_ins ? k + 1 : a.max_ins; }
    }
    const long long m = d > n_ins ? d - n_ins : 0;
    const long long c0 = n_ins * a.mis_g + m * a.hom_g;
    const long long c1 = (n_ins + m) * a.het_g + a.alt_prior;
    const long long c2 = n_ins * a.hom_g + m * a.mis_g + a.alt_prior;
    int copies = 0;
    long long i_least = c0, i_second = c1;
    if (c1 < i_least) { copies = 1; i_second = i_least; i_least = c1; }
    if (c2 < i_least) { copies = 2; i_second = i_least; i_least = c2; }
    else if (c2 < i_second) i_second = c2;
    if (!deep) copies = 0;
    const int by_cost = copies;
    int n_out = 0;
    bool open = copies >= 1;
    for (int k = 0; k < a.max_ins; ++k) {
        const int* s = a.ins_bases + (p * a.max_ins + k) * 4;
        int bb = 0, bc = s[0];
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            const int v = s[q];
            bb = v > bc ? q : bb;
            bc = v > bc ? v : bc;
        }
        open = open && k < len && bc > 0;                            // the first slot with no count ends the insertion
        a.ins_out[p * a.max_ins + k] = (unsigned char)(open ? bb + 1 : 0);
        n_out += open ? 1 : 0;
    }
    if (n_out == 0) copies = 0;                                      // an empty sequence: nothing is called
    if (copies >= 1) flags |= WN_CALL_INSERTION;
    if (copies == 1) flags |= WN_CALL_INS_HET;
    const bool ins_scored = deep && !(by_cost >= 1 && n_out == 0);
    a.alleles[2 * p] = (unsigned char)l0;
    a.alleles[2 * p + 1] = (unsigned char)l1;
    a.gq[p] = gq;
    a.qual[p] = qual;
    a.flags[p] = (unsigned char)flags;
    a.ins_copies[p] = (unsigned char)copies;
    a.ins_len[p] = (unsigned char)n_out;
    a.ins_gq[p] = ins_scored ? clamp_i32(i_second - i_least) : 0;
    a.ins_qual[p] = ins_scored ? clamp_i32(c0 - i_least) : 0;
}

// every weight in [0, 2^20]
static bool weights_ok(const int* w) {
    for (int t = 0; t < kGWeights; ++t)
        if (w[t] < 0 || w[t] > kGMaxWeight) return false;
    return true;
}

}  // namespace wn
using namespace wn;

int wn_pileup_evidence(const unsigned char* ops, long long ops_stride, const int* ops_len, const int* lo, const int* ref_lengths,
                       const int* strand, const int* query, long long query_stride, const int* query_lengths,
                       const unsigned char* qual, long long qual_stride, const unsigned char* keep, int batch, int max_query_len,
                       int max_ops, int reference_len, const unsigned char* cap, const int* weights_host, int flat_qual, int gap_qual,
                       int min_qual, long long* evidence, signed char* used, int* bad, wn_stream_t stream) {
    EvidenceArgs a = {};
    a.r = read_batch(ops, ops_stride, ops_len, lo, ref_lengths, strand, query, query_stride, query_lengths, qual, qual_stride, keep, batch,
                     max_query_len, max_ops, reference_len, min_qual);
    if (const int s = check_read_batch(a.r, flat_qual >= 0 && gap_qual >= 0,
                                       min_qual < kPQualRows && flat_qual < kPQualRows && gap_qual < kPQualRows,
                                       weights_host && evidence && used))
        return s;
    if (!weights_ok(weights_host)) return WN_ERR_UNSUPPORTED;
    a.cap = cap; a.evidence = (unsigned long long*)evidence; a.used = used; a.bad = bad; a.flat_qual = flat_qual; a.gap_qual = gap_qual;
    for (int t = 0; t < kGWeights; ++t) a.w[t] = weights_host[t];
    hipLaunchKernelGGL(pileup_evidence_kernel, dim3(batch), dim3(kPThreads), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "pileup_evidence");
    return WN_OK;
}

int wn_genotype_call(const long long* evidence, const int* counts, const int* ins_lengths, const int* ins_bases, const int* reference,
                     int reference_len, int max_ins, int min_depth, int alt_prior, const int* weights_host, int gap_qual,
                     unsigned char* alleles, int* gq, int* qual, unsigned char* flags, unsigned char* ins_copies, unsigned char* ins_len,
                     unsigned char* ins_out, int* ins_gq, int* ins_qual, long long* costs, wn_stream_t stream) {
    if (reference_len < 1 || max_ins < 0 || min_depth < 1 || gap_qual < 0) return WN_ERR_BAD_SHAPE;
    if (reference_len > kMaxReference || max_ins > kMaxIns || gap_qual >= kPQualRows) return WN_ERR_UNSUPPORTED;
    if (alt_prior < 0 || alt_prior > kGMaxPrior) return WN_ERR_UNSUPPORTED;
    if (!evidence || !counts || !ins_lengths || !reference || !weights_host || !alleles || !gq || !qual || !flags || !ins_copies ||
        !ins_len || !ins_gq || !ins_qual)
        return WN_ERR_NULL;
    if (max_ins > 0 && (!ins_bases || !ins_out)) return WN_ERR_NULL;
    if (!weights_ok(weights_host)) return WN_ERR_UNSUPPORTED;
    GenotypeArgs a = {};
    a.evidence = evidence; a.counts = counts; a.ins_lengths = ins_lengths; a.ins_bases = ins_bases; a.reference = reference;
    a.alleles = alleles; a.gq = gq; a.qual = qual; a.flags = flags; a.ins_copies = ins_copies; a.ins_len = ins_len; a.ins_out = ins_out;
    a.ins_gq = ins_gq; a.ins_qual = ins_qual; a.costs = costs;
    a.R = reference_len; a.max_ins = max_ins; a.min_depth = min_depth; a.alt_prior = alt_prior;
    a.hom_g = weights_host[gap_qual]; a.het_g = weights_host[kPQualRows + gap_qual]; a.mis_g = weights_host[2 * kPQualRows + gap_qual];
    hipLaunchKernelGGL(genotype_call_kernel, dim3(cdiv(reference_len, kGTile)), dim3(kPThreads), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "genotype_call");
    return WN_OK;
}
