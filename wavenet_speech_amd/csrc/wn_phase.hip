// Read-backed phasing of diploid calls and haplotags: the walk of wn_opscan.h with pileup_kernel's checks,
// looking only at the columns that land on a heterozygous site, then a greedy best-link forest over the sites and a tag per read.
//
//   phase_links_kernel   grid (batch), 256 threads, ONE WORKGROUP PER READ: validate_ops with pileup_kernel's window and qual checks,
//                        so that `used` and *bad agree with it, then walk_ops.  A column that pileup_evidence_kernel adds for and
//                        whose forward position is a site is an OBSERVATION (site s, allele x in {0, 1, neither}, weight q' =
//                        min(q, cap[b]) <= 93).  The walk meets a read's sites in ascending order and each at most once, so the
//                        observations of a tile are compacted in walk order (a ballot, the waves' counts through LDS) into a ring of
//                        512 entries -- the 256 of the tile and more than `reach` <= 8 before them -- and the partner of an
//                        observation at site s - d, if the read has one, is among the `reach` entries before it.  One thread per
//                        observation looks back and adds min(q', q'') to links[s][d - 1][x xor x'']: 64-bit integer atomics.
//                        The ring holds observations, not positions: 3 KB for a window of any length.
//   haplotag_kernel      the same walk three times: the checks; the arg-max of (q', least site) over the read's observations in
//                        phased sets, a packed sortable 64-bit word through wave_reduce and LDS; the sums of that set.
//   phase_parent_kernel  one thread per site: the greatest |cis - trans| of its `reach` look-backs, ties to the nearest.
//   phase_jump_kernel    one round of pointer doubling over (parent, parity) packed in an int; ceil(log2 S) launches, ping-pong.
//   phase_root_kernel / phase_size_kernel   root, parity, ps, and the set's size: an integer atomic at the root, then a gather.
// No floating point, no scratch, no workgroup waits on another.  No value of an op, a label, a length, a position, a qual, a cap or a
// site index is used as an index before it is checked.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_opscan.h"

namespace wn {

constexpr int kHMaxReach = 8;
constexpr int kHRing = 512;                   // a power of two >= 256 + kHMaxReach
constexpr int kHNeither = 2;
constexpr int kHParityBit = 1 << 30;          // of a packed jump: site indices stay below 2^26

struct PhaseReads {                     // what wn_phase_links and wn_haplotag take alike
    ReadBatch r;
    const unsigned char* cap;           // or nullptr
    const int* site_of;                 // [R]
    const unsigned char* alleles;       // [S][2]
    int S, flat_qual, gap_qual;
};

struct ReadView {                       // an opened read, the same in every thread
    OpRow row;
    const int* query;
    const unsigned char* qual;
    int lo, n_ref, n_query, first, last, cap, q_gap;
};

// pileup_kernel's prologue and pass 1 -> 0 skipped or no aligned column, -1 bad, 1 to be walked.  BARRIERS: one between
// validate_begin and validate_ops, and validate_ops' own.  Every thread of the workgroup calls it.
__device__ __forceinline__ int open_read(const PhaseReads& a, int b, int tid, OpWalk* walk, int* s_lo, int* s_hi, int* s_bad, ReadView* v) {
    const int strand = a.r.strand[b], n_ref = a.r.ref_len[b];
    if (read_skipped(strand, n_ref, a.r.keep, b)) return 0;          // nothing else of the read is looked at
    const int n_ops = a.r.ops_len[b], n_query = a.r.query_len[b], lo = a.r.lo[b];
    const bool header_ok = head_ok(strand, n_ref, lo >= 0 && (long long)lo + n_ref <= a.r.R, n_query, a.r.M, n_ops, a.r.max_ops);
    v->row = op_row(a.r.ops + (long long)b * a.r.ops_stride, header_ok, n_ops, n_ref, n_query, strand == 1);
    v->query = a.r.query + (long long)b * a.r.query_stride;
    v->qual = a.r.qual ? a.r.qual + (long long)b * a.r.qual_stride : nullptr;
    v->lo = lo; v->n_ref = n_ref; v->n_query = n_query;
    const unsigned char* qual = v->qual;
    const bool rev = v->row.rev;
    validate_begin(tid, header_ok, s_lo, s_hi, s_bad);
    __syncthreads();
    const OpSpan span = validate_ops(v->row, tid, walk, s_lo, s_hi, s_bad, [&](const OpCol& c, bool, bool in_query) {
        return !(in_query && qual && qual[rev ? n_query - 1 - c.j : c.j] >= kPQualRows);
    });
    if (span.bad) return -1;
    v->first = span.first; v->last = span.last;
    v->cap = a.cap ? (int)a.cap[b] : kPQualRows - 1;
    v->q_gap = a.gap_qual < v->cap ? a.gap_qual : v->cap;            // gap_qual and flat_qual are at most 93: checked on the host
    return span.last >= 0 ? 1 : 0;
}

struct Obs { int s, x, q; };            // s < 0: the column is no observation; x: 0, 1 or kHNeither; q <= 93

// what a column of pass 2 shows: pileup_evidence_kernel's column rules, then the site.  Every index was checked in pass 1 on the
// same words and is checked again before it is used.
__device__ __forceinline__ Obs observe(const PhaseReads& a, const ReadView& v, const OpCol& c) {
    const int i = c.i, j = c.j;
    if (!c.active || c.w < v.first || c.w > v.last || !c.is_ref || i >= v.n_ref) return {-1, 0, 0};   // end and insertion columns
    int label = 0, q = v.q_gap;
    if (c.op != 3) {
        label = -1;                                                  // `other`, as in pileup_kernel
        if (j < v.n_query) {
            const int jq = v.row.rev ? v.n_query - 1 - j : j;
            const int t = v.query[jq];
            const int qb = v.qual ? (int)v.qual[jq] : a.flat_qual;   // min_qual sees the uncapped qual
            if (t >= 1 && t <= 4 && !(v.qual && qb < a.r.min_qual)) {
                label = v.row.rev ? 5 - t : t;
                q = qb < v.cap ? qb : v.cap;
            }
        }
    }
    if (label < 0 || q < 0 || q >= kPQualRows) return {-1, 0, 0};
    const int s = a.site_of[v.lo + i];                               // lo >= 0, lo + n_ref <= R: the header
    if (s < 0 || s >= a.S) return {-1, 0, 0};
    const int a0 = a.alleles[2 * (size_t)s], a1 = a.alleles[2 * (size_t)s + 1];
    return {s, label == a0 ? 0 : label == a1 ? 1 : kHNeither, q};
}

struct LinkArgs {
    PhaseReads p;
    unsigned long long* links;          // [S][reach][2]
    int* observed;                      // [S][3]
    signed char* used;
    int* bad;
    int reach;
};

__global__ __launch_bounds__(kPThreads) void phase_links_kernel(const LinkArgs a) {
    __shared__ int s_slot[2][2][kPWaves];
    __shared__ int s_lo, s_hi, s_bad;
    __shared__ int s_cnt[kPWaves];
    __shared__ int s_site[kHRing];
    __shared__ unsigned short s_code[kHRing];                        // x << 7 | q
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    OpWalk walk{s_slot};
    ReadView v;
    const int state = open_read(a.p, b, tid, &walk, &s_lo, &s_hi, &s_bad, &v);
    if (tid == 0) a.used[b] = (signed char)state;
    if (state < 0) report_bad(tid, a.bad);
    if (state != 1) return;

    // ---- pass 2.  Two barriers per tile: the waves' counts, then the ring's entries.  s_cnt is written again only behind the next
    // tile's scan barrier, which every wave reaches after it has read the counts; a ring entry is overwritten 512 observations later
    const unsigned long long below = (1ull << lane) - 1ull;
    int base = 0;                                                    // the observations before the tile
    walk_ops(v.row, tid, &walk, [&](const OpCol& c) {
        const Obs o = observe(a.p, v, c);
        const bool has = o.s >= 0;
        const unsigned long long m = __ballot(has);
        if (lane == 0) s_cnt[wave] = __popcll(m);
        __syncthreads();
        int off, tot;
        wave_offsets<kPWaves>(s_cnt, wave, &off, &tot);
        const int k = base + off + __popcll(m & below);
        if (has) {
            s_site[k & (kHRing - 1)] = o.s;
            s_code[k & (kHRing - 1)] = (unsigned short)(o.x << 7 | o.q);
            atomicAdd(a.observed + (size_t)o.s * 3 + o.x, 1);
        }
        __syncthreads();
        if (has && o.x != kHNeither) {
            for (int e = 1; e <= a.reach && e <= k; ++e) {           // sites ascend along the walk: the partner at s - d is at most d back
                const int at = (k - e) & (kHRing - 1), d = o.s - s_site[at];
                if (d > a.reach) break;
                const int x2 = s_code[at] >> 7, q2 = s_code[at] & 127;
                if (d >= 1 && x2 != kHNeither)
                    atomicAdd(a.links + (((size_t)o.s * a.reach + d - 1) * 2 + (o.x ^ x2)), (unsigned long long)(o.q < q2 ? o.q : q2));
            }
        }
        base += tot;
    });
}

struct TagArgs {
    PhaseReads p;
    const int* pos;                     // [S]
    const int* root;
    const unsigned char* parity;
    const int* set_size;
    unsigned char* hp;
    int* ps;
    int* weight;                        // [B][2]
    int* n_sites;                       // [B][2]
    int* bad;
};

// a read that is skipped, bad or shows no site of a phased set
__device__ __forceinline__ void untagged(const TagArgs& a, int b, int tid) {
    if (tid != 0) return;
    a.hp[b] = 0; a.ps[b] = -1;
    a.weight[2 * b] = a.weight[2 * b + 1] = a.n_sites[2 * b] = a.n_sites[2 * b + 1] = 0;
}

__global__ __launch_bounds__(kPThreads) void haplotag_kernel(const TagArgs a) {
    __shared__ int s_slot[2][2][kPWaves];
    __shared__ int s_lo, s_hi, s_bad;
    __shared__ unsigned long long s_best[kPWaves];
    __shared__ int s_sum[kPWaves][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    OpWalk walk{s_slot};
    ReadView v;
    const int state = open_read(a.p, b, tid, &walk, &s_lo, &s_hi, &s_bad, &v);
    if (state < 0) report_bad(tid, a.bad);
    if (state != 1) return untagged(a, b, tid);
    // ---- pass 2: the most confident observation, (q' + 1) above the complement of the site: greatest q', then least site
    unsigned long long best = 0;                                     // 0: no observation
    walk_ops(v.row, tid, &walk, [&](const OpCol& c) {
        const Obs o = observe(a.p, v, c);
        if (o.s < 0 || o.x == kHNeither || a.set_size[o.s] <= 1) return;
        const unsigned long long key = (unsigned long long)(o.q + 1) << 32 | (0xFFFFFFFFu - (unsigned)o.s);
        best = key > best ? key : best;
    });
    best = wave_reduce(best, OpMax());
    if (lane == 0) s_best[wave] = best;
    __syncthreads();
    best = s_best[0];
#pragma unroll
    for (int w = 1; w < kPWaves; ++w) best = s_best[w] > best ? s_best[w] : best;
    if (best == 0) return untagged(a, b, tid);                       // the same in every thread
    const int at = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));      // a site observe() returned: below S
    const int set = a.root[at];
    // ---- pass 3: the sums of that set
    int w0 = 0, w1 = 0, n_in = 0, n_out = 0;
    walk_ops(v.row, tid, &walk, [&](const OpCol& c) {
        const Obs o = observe(a.p, v, c);
        const bool counts = o.s >= 0 && o.x != kHNeither && a.set_size[o.s] > 1;
        const bool inside = counts && a.root[o.s] == set;
        const int h = inside ? (o.x ^ a.parity[o.s]) & 1 : 0;
        n_in += inside ? 1 : 0;
        n_out += counts && !inside ? 1 : 0;
        w0 += inside && h == 0 ? o.q : 0;
        w1 += inside && h == 1 ? o.q : 0;
    });
    wave_reduce_each(OpAdd(), w0, w1, n_in, n_out);
    if (lane == 0) { s_sum[wave][0] = w0; s_sum[wave][1] = w1; s_sum[wave][2] = n_in; s_sum[wave][3] = n_out; }
    __syncthreads();
    if (tid == 0) {
        int t0 = 0, t1 = 0, t2 = 0, t3 = 0;
#pragma unroll
        for (int w = 0; w < kPWaves; ++w) { t0 += s_sum[w][0]; t1 += s_sum[w][1]; t2 += s_sum[w][2]; t3 += s_sum[w][3]; }
        a.hp[b] = (unsigned char)(t0 > t1 ? 1 : t0 < t1 ? 2 : 0);
        a.ps[b] = set >= 0 && set < a.p.S ? a.pos[set] : -1;
        a.weight[2 * b] = t0; a.weight[2 * b + 1] = t1;
        a.n_sites[2 * b] = t2; a.n_sites[2 * b + 1] = t3;
    }
}

// ---- the chain -------------------------------------------------------------------------------------------------------------------
struct ChainArgs {
    const long long* links;             // [S][reach][2]
    const int* pos;
    int* parent;
    unsigned char* flip;
    int* margin;
    int* root;
    unsigned char* parity;
    int* ps;
    int* set_size;
    int* jump;                          // the packed (parent, parity) of the first round
    int S, reach, min_margin;
};

__global__ __launch_bounds__(kPThreads) void phase_parent_kernel(const ChainArgs a) {
    const long long s = (long long)blockIdx.x * kPThreads + threadIdx.x;
    if (s >= a.S) return;
    unsigned long long best = 0;
    int best_d = 0, best_flip = 0;
    for (int d = 1; d <= a.reach && d <= s; ++d) {
        const long long cis = a.links[(s * a.reach + d - 1) * 2], trans = a.links[(s * a.reach + d - 1) * 2 + 1];
        const unsigned long long m = trans > cis ? (unsigned long long)trans - (unsigned long long)cis
                                                 : (unsigned long long)cis - (unsigned long long)trans;
        if (best_d == 0 || m > best) { best = m; best_d = d; best_flip = trans > cis ? 1 : 0; }          // ties to the least d
    }
    const bool is_root = best_d == 0 || best < (unsigned long long)a.min_margin;
    const int parent = is_root ? (int)s : (int)s - best_d, flip = is_root ? 0 : best_flip;
    a.parent[s] = parent;
    a.flip[s] = (unsigned char)flip;
    a.margin[s] = is_root ? 0 : best > (unsigned long long)INT_MAX ? INT_MAX : (int)best;
    a.jump[s] = parent | (flip ? kHParityBit : 0);
    a.set_size[s] = 0;                                               // phase_root_kernel counts into the roots' cells
}

// out[s] = in[in[s]]: the pointer twice as far, the parities xor-ed
__global__ __launch_bounds__(kPThreads) void phase_jump_kernel(const int* in, int* out, int S) {
    const long long s = (long long)blockIdx.x * kPThreads + threadIdx.x;
    if (s >= S) return;
    const int mine = in[s], next = in[mine & (kHParityBit - 1)];
    out[s] = (next & (kHParityBit - 1)) | ((mine ^ next) & kHParityBit);
}

__global__ __launch_bounds__(kPThreads) void phase_root_kernel(const int* jump, const ChainArgs a) {
    const long long s = (long long)blockIdx.x * kPThreads + threadIdx.x;
    if (s >= a.S) return;
    const int root = jump[s] & (kHParityBit - 1);
    a.root[s] = root;
    a.parity[s] = (unsigned char)(jump[s] & kHParityBit ? 1 : 0);
    a.ps[s] = a.pos[root];
    atomicAdd(a.set_size + root, 1);
}

// only the roots' cells are read, and a root writes its own value back: no cell is read after another thread has changed it
__global__ __launch_bounds__(kPThreads) void phase_size_kernel(const int* root, int* set_size, int S) {
    const long long s = (long long)blockIdx.x * kPThreads + threadIdx.x;
    if (s >= S) return;
    set_size[s] = set_size[root[s]];
}

static PhaseReads phase_reads(const ReadBatch& r, const unsigned char* cap, const int* site_of, const unsigned char* alleles, int n_sites,
                              int flat_qual, int gap_qual) {
    return {r, cap, site_of, alleles, n_sites, flat_qual, gap_qual};
}
// the verdicts wn_phase_links and wn_haplotag add to check_read_batch's
static bool phase_shape_ok(const PhaseReads& p) { return p.flat_qual >= 0 && p.gap_qual >= 0 && p.S >= 1; }
static bool phase_supported(const PhaseReads& p) {
    return p.r.min_qual < kPQualRows && p.flat_qual < kPQualRows && p.gap_qual < kPQualRows && p.S <= p.r.R;
}

}  // namespace wn
using namespace wn;

int wn_phase_links(const unsigned char* ops, long long ops_stride, const int* ops_len, const int* lo, const int* ref_lengths,
                   const int* strand, const int* query, long long query_stride, const int* query_lengths, const unsigned char* qual,
                   long long qual_stride, const unsigned char* keep, int batch, int max_query_len, int max_ops, int reference_len,
                   const unsigned char* cap, int flat_qual, int gap_qual, int min_qual, const int* site_of, const unsigned char* alleles,
                   int n_sites, int reach, long long* links, int* observed, signed char* used, int* bad, wn_stream_t stream) {
    LinkArgs a = {};
    a.p = phase_reads(read_batch(ops, ops_stride, ops_len, lo, ref_lengths, strand, query, query_stride, query_lengths, qual, qual_stride,
                                 keep, batch, max_query_len, max_ops, reference_len, min_qual),
                      cap, site_of, alleles, n_sites, flat_qual, gap_qual);
    if (const int s = check_read_batch(a.p.r, phase_shape_ok(a.p) && reach >= 1, phase_supported(a.p) && reach <= kHMaxReach,
                                       site_of && alleles && links && observed && used))
        return s;
    a.links = (unsigned long long*)links; a.observed = observed; a.used = used; a.bad = bad; a.reach = reach;
    hipLaunchKernelGGL(phase_links_kernel, dim3(batch), dim3(kPThreads), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "phase_links");
    return WN_OK;
}

int wn_haplotag(const unsigned char* ops, long long ops_stride, const int* ops_len, const int* lo, const int* ref_lengths,
                const int* strand, const int* query, long long query_stride, const int* query_lengths, const unsigned char* qual,
                long long qual_stride, const unsigned char* keep, int batch, int max_query_len, int max_ops, int reference_len,
                const unsigned char* cap, int flat_qual, int gap_qual, int min_qual, const int* site_of, const unsigned char* alleles,
                int n_sites, const int* pos, const int* root, const unsigned char* parity, const int* set_size, unsigned char* hp, int* ps,
                int* weight, int* n_observed, int* bad, wn_stream_t stream) {
    TagArgs a = {};
    a.p = phase_reads(read_batch(ops, ops_stride, ops_len, lo, ref_lengths, strand, query, query_stride, query_lengths, qual, qual_stride,
                                 keep, batch, max_query_len, max_ops, reference_len, min_qual),
                      cap, site_of, alleles, n_sites, flat_qual, gap_qual);
    if (const int s = check_read_batch(a.p.r, phase_shape_ok(a.p), phase_supported(a.p),
                                       site_of && alleles && pos && root && parity && set_size && hp && ps && weight && n_observed))
        return s;
    a.pos = pos; a.root = root; a.parity = parity; a.set_size = set_size; a.hp = hp; a.ps = ps; a.weight = weight; a.n_sites = n_observed;
    a.bad = bad;
    hipLaunchKernelGGL(haplotag_kernel, dim3(batch), dim3(kPThreads), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "haplotag");
    return WN_OK;
}

int wn_phase_chain(const long long* links, const int* pos, int n_sites, int reach, int min_margin, int* parent, unsigned char* flip,
                   int* margin, int* root, unsigned char* parity, int* ps, int* set_size, int* work, wn_stream_t stream) {
    if (n_sites < 1 || reach < 1 || min_margin < 0) return WN_ERR_BAD_SHAPE;
    if (n_sites > kMaxReference || reach > kHMaxReach) return WN_ERR_UNSUPPORTED;
    if (!links || !pos || !parent || !flip || !margin || !root || !parity || !ps || !set_size || !work) return WN_ERR_NULL;
    ChainArgs a = {};
    a.links = links; a.pos = pos; a.parent = parent; a.flip = flip; a.margin = margin; a.root = root; a.parity = parity; a.ps = ps;
    a.set_size = set_size; a.jump = work; a.S = n_sites; a.reach = reach; a.min_margin = min_margin;
    const dim3 grid(cdiv(n_sites, kPThreads)), block(kPThreads);
    hipLaunchKernelGGL(phase_parent_kernel, grid, block, 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "phase_parent");
    int* jump[2] = {work, work + n_sites};
    int from = 0;
    for (long long far = 1; far < n_sites; far *= 2, from ^= 1) {    // ceil(log2 S) rounds: the deepest site lies S - 1 steps from its root
        hipLaunchKernelGGL(phase_jump_kernel, grid, block, 0, (hipStream_t)stream, jump[from], jump[from ^ 1], n_sites);
        WN_HIP(hipGetLastError(), "phase_jump");
    }
    hipLaunchKernelGGL(phase_root_kernel, grid, block, 0, (hipStream_t)stream, jump[from], a);
    WN_HIP(hipGetLastError(), "phase_root");
    hipLaunchKernelGGL(phase_size_kernel, grid, block, 0, (hipStream_t)stream, root, set_size, n_sites);
    WN_HIP(hipGetLastError(), "phase_size");
    return WN_OK;
}
