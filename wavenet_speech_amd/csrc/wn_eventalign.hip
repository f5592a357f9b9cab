// Event alignment with skips under the k-mer pore model: the DETECTED events of a read (wn_event_detect,
// section 7m) against the k-mers of its KNOWN bases.  Between consecutive events the path stays (the detector cut one k-mer in
// two), steps, or skips one or two k-mers (the detector missed boundaries), each move at its own cost, and an event costs the exact
// sum over its samples of what wn_signal_align (section 7k) charges a sample -- formed from (n, sum q, sum q^2) alone.  What
// nanopolish `eventalign` is.  Everything is an integer.
//
//   event_align_kernel   one workgroup per read on the banded-path core of wn_band_dev.h (slots, band entry, closing, trace
//                        windows), two phases in one launch.  What is this kernel's own:
//
//     forward   cost_e(j) = min_m (cost_{e-1}(j - m) + move_cost[m]) + event_cost(e, model[kmer_j]), m in 0..3, over the states of
//               the band [lo(e), lo(e) + W).  lo rises by up to THREE per event (N <= 3 (E - 1) + 1), so up to three states enter
//               the band in one step.  A predecessor j - m is taken only if it lay inside the band of event e - 1: with
//               pj = j - lo(e - 1), iff 0 <= pj - m < W -- this one test covers the state that has just entered (its slot still
//               holds the cost of the state that left), the states below the old band and the wrap of the slots.  THREE values
//               cross threads per step: the last three slots of the left neighbour, cyclic over the band, through a
//               double-buffered LDS row and ONE workgroup barrier per step.  The eight 2-bit backpointers of a thread are one
//               16-bit store to the workspace, bp[b][e][W / 8].  Events are staged 256 at a time into LDS as (n, sum, sumsq) and
//               validated there, S^2 <= n Q in a 128-bit product.
//     trace     the path moves at most three states per event, so a chunk's window is 49 bytes per event; one lane walks the 64
//               steps in LDS, then the threads write event_state, the starts (in samples, from ev_starts) of the states that
//               begin in the chunk -- a skipped state begins where its successor does -- and count the moves and the events on
//               the band's edge.
//
// Ties (tests/event_align_ref.py holds the same rule): the stay first, each larger move only if strictly cheaper, move cost
// included.  No value of a length, a label or an event is used as an index before it is checked; a read found bad anywhere in the
// forward phase gets its outputs from the fill at the end, never from the trace.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"
#include "wn_band_dev.h"

namespace wn {

constexpr int kEaTile = 256;                  // events staged into LDS at a time
constexpr int kEaMaxMove = 3;                 // states a path advances per event at the most
constexpr int kEaWinBytes = kBandWinBytes<2, kEaMaxMove>;            // 2-bit backpointers, three states per event at the most: 49
constexpr int kEaMaxSignal = 1 << 24;         // T_b
constexpr int kEaMaxEvents = 1 << 20;         // events and states per read
constexpr int kEaMaxEventLen = 65536;
constexpr int kEaMoveLimit = 1 << 30;         // a move's cost stays below
constexpr long long kEaQMax = kSigQLimit - 1;
// a path's cost stays below 2^24 (2^31 + 2^30) + 2^20 2^30 < 2^56 < kPathInf

// the dynamic LDS of a workgroup, in this order: int64 first
constexpr size_t kEaEdgeBytes = 2 * kEaMaxMove * kBandMaxThreads * sizeof(long long);
constexpr size_t kEaFixedLds = kEaEdgeBytes + 2 * kEaTile * sizeof(long long) + (kEaTile + kBandCodes + kBandTrace + 4) * sizeof(int);
static_assert(kBandTrace * kEaWinBytes <= (int)kEaEdgeBytes, "the trace window reuses the edge rows");

struct EventAlignArgs {
    const int* n_events;
    const int* ev_starts;               // [B][max_events + 1]
    const long long* ev_sum;            // [B][max_events]
    const long long* ev_sumsq;
    const int* labels;
    const int* label_lengths;
    const int* model;                   // [4^k][3]: level, weight, offset
    long long labels_stride;
    int B, max_events, max_labels, max_states, k, first, weight_shift, max_cost, band, max_move;
    int move_cost[4];
    int* starts;                        // [B][max_states + 1]
    long long* score;                   // [B]
    int* event_state;                   // [B][max_events] or nullptr
    int* move_counts;                   // [B][4]
    int* band_hits;                     // [B]
    unsigned char* bp;                  // workspace: [B][max_events][band / 4]
    int* bad;
};

// min((D weight) >> S, n max_cost) + n offset with D = Q - 2 level S1 + n level^2, the exact sum of (q - level)^2 over the event's
// samples: 0 <= D < 2^64 for a valid event, so arithmetic modulo 2^64 is exact; the 95-bit product is compared before it is narrowed
__device__ __forceinline__ long long ea_event_cost(int n, long long s1, long long q2, int level, int weight, int offset, int S,
                                                   unsigned long long cap) {
    const unsigned long long l = (unsigned long long)(long long)level;
    const unsigned long long D = (unsigned long long)q2 - 2ull * l * (unsigned long long)s1 + (unsigned long long)n * l * l;
    const unsigned __int128 sh = ((unsigned __int128)D * (unsigned)weight) >> S;
    const long long c = sh < (unsigned __int128)cap ? (long long)sh : (long long)cap;
    return c + (long long)n * offset;
}

// an event of the table that the costs may use: n in [1, 65536], |S| <= n (2^23 - 1), 0 <= Q <= n (2^23 - 1)^2, S^2 <= n Q
__device__ __forceinline__ bool ea_event_ok(long long n, long long s1, long long q2) {
    if (n < 1 || n > kEaMaxEventLen) return false;
    const long long lim = n * kEaQMax;                               // < 2^39
    if (s1 < -lim || s1 > lim || q2 < 0 || q2 > lim * kEaQMax) return false;
    const unsigned long long a = (unsigned long long)(s1 < 0 ? -s1 : s1);
    return (unsigned __int128)a * a <= (unsigned __int128)(unsigned long long)n * (unsigned long long)q2;
}

__global__ __launch_bounds__(kBandMaxThreads) void event_align_kernel(const EventAlignArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ea_smem[];
    long long* s_edge = reinterpret_cast<long long*>(ea_smem);       // [2][3][kBandMaxThreads]: every thread's last three slots, by step parity
    long long* s_sum = s_edge + 2 * kEaMaxMove * kBandMaxThreads;    // [kEaTile]
    long long* s_sq = s_sum + kEaTile;                               // [kEaTile]
    int* s_len = reinterpret_cast<int*>(s_sq + kEaTile);             // [kEaTile]
    int* s_code = s_len + kEaTile;                                   // [kBandCodes]
    int* s_path = s_code + kBandCodes;                               // [kBandTrace + 1]: [0] the state before the chunk, [1 + f]
    int* s_model = s_path + kBandTrace + 4;                          // [4^k][3]
    unsigned char* s_win = reinterpret_cast<unsigned char*>(s_edge); // [kBandTrace][kEaWinBytes]: the trace runs after the last edge row is read
    __shared__ long long s_fin;
    __shared__ int s_bad, s_hits, s_cnt[4];
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int W = a.band, nact = W / kBandPer, k = a.k, S = a.weight_shift;
    const int E = a.n_events[b], Lb = a.label_lengths[b];
    const long long n64 = (long long)Lb - (k - 1) - 2 * a.first;
    const bool bad_len = E < 0 || E > a.max_events || Lb < 0 || Lb > a.max_labels || n64 > a.max_states;
    const bool none = !bad_len && (E < 1 || n64 < 1 || n64 - 1 > (long long)a.max_move * (E - 1));
    int* st_out = a.starts + (long long)b * (a.max_states + 1);
    int* es_out = a.event_state ? a.event_state + (long long)b * a.max_events : nullptr;
    if (bad_len || none) {                                           // workgroup-uniform: nothing else of the read is looked at
        band_refuse(bad_len, st_out, a.max_states + 1, es_out, a.max_events, a.score + b, a.band_hits + b, a.bad, tid, nthr);
        if (tid < 4) a.move_counts[4 * b + tid] = bad_len ? -1 : 0;
        return;
    }
    const int N = (int)n64;                                          // 1 <= N <= max_move (E - 1) + 1

    for (int i = tid; i < (3 << (2 * k)); i += nthr) s_model[i] = a.model[i];
    if (tid == 0) { s_bad = 0; s_hits = 0; s_fin = kPathInf; }
    if (tid < 4) s_cnt[tid] = 0;
    __syncthreads();

    const int* lab = a.labels + (long long)b * a.labels_stride + a.first;        // state j is the window lab[j .. j + k)
    int lvl[kBandPer], wgt[kBandPer], off[kBandPer];
    long long d[kBandPer];
    unsigned alive;
    bool ok = true;
    band_arm(s_model, lab, k, N, W, tid, lvl, wgt, off, d, alive, ok);           // N + k - 1 = Lb - 2 first: inside the labels

    const int* es = a.ev_starts + (long long)b * (a.max_events + 1);
    const long long* esum = a.ev_sum + (long long)b * a.max_events;
    const long long* esq = a.ev_sumsq + (long long)b * a.max_events;
    const int Tb = es[E];                                            // E <= max_events: inside the row
    if (es[0] < 0 || Tb > kEaMaxSignal) ok = false;
    const long long mc0 = a.move_cost[0], mc1 = a.move_cost[1], mc2 = a.move_cost[2], mc3 = a.move_cost[3];
    unsigned char* bprow = a.bp + (long long)b * a.max_events * (W / 4);
    BandCursor cur(N, E, W);
    for (int e = 0; e < E; ++e) {
        const int ke = e & (kEaTile - 1);
        if (ke == 0) {                                               // the barrier of step e - 1: the old tile is no longer read
            for (int i = tid; i < kEaTile && e + i < E; i += nthr) {
                long long n = (long long)es[e + i + 1] - es[e + i], s1 = esum[e + i], q2 = esq[e + i];
                if (!ea_event_ok(n, s1, q2)) { ok = false; n = 1; s1 = 0; q2 = 0; }
                s_len[i] = (int)n; s_sum[i] = s1; s_sq[i] = q2;
            }
            __syncthreads();
        }
        int delta = 0;                                               // lo(e) - lo(e - 1), 0..3; workgroup-uniform
        if (e > 0) {
            const int r = cur.lo, slot = cur.lo_slot;
            delta = cur.advance();                                   // N < 3 E: at most three
            for (int i = 0; i < delta; ++i)
                band_enter(r + i, slot + i >= W ? slot + i - W : slot + i, s_model, s_code, lab, k, N, W, tid, nthr, lvl, wgt, off, ok);
        }
        const int n = s_len[ke];
        const long long s1 = s_sum[ke], q2 = s_sq[ke];
        const unsigned long long cap = (unsigned long long)n * (unsigned)a.max_cost;
        long long p1 = kPathInf, p2 = kPathInf, p3 = kPathInf;       // cost_{e-1} of the one, two and three slots to the left
        if (e > 0) {
            const long long* row = s_edge + ((e - 1) & 1) * kEaMaxMove * kBandMaxThreads;
            const int left = tid == 0 ? nact - 1 : tid - 1;
            p3 = row[left]; p2 = row[kBandMaxThreads + left]; p1 = row[2 * kBandMaxThreads + left];
        }
        int rel = kBandPer * tid - cur.lo_slot;                      // this slot's state is lo + rel
        if (rel < 0) rel += W;
        unsigned bits = 0;
#pragma unroll
        for (int i = 0; i < kBandPer; ++i) {
            const int pj = rel + delta;                              // the state's place in the band of event e - 1: inside iff 0 <= pj - m < W
            const long long cur = d[i];
            long long best = kPathInf;
            unsigned mv = 0;
            if (mc0 >= 0 && (unsigned)pj < (unsigned)W && cur < kPathInf) best = cur + mc0;
            if ((unsigned)(pj - 1) < (unsigned)W && p1 < kPathInf && p1 + mc1 < best) { best = p1 + mc1; mv = 1; }
            if (mc2 >= 0 && (unsigned)(pj - 2) < (unsigned)W && p2 < kPathInf && p2 + mc2 < best) { best = p2 + mc2; mv = 2; }
            if (mc3 >= 0 && (unsigned)(pj - 3) < (unsigned)W && p3 < kPathInf && p3 + mc3 < best) { best = p3 + mc3; mv = 3; }
            if (e == 0) { best = kBandPer * tid + i == 0 ? 0 : kPathInf; mv = 0; }      // paths start in state 0
            long long nd = kPathInf;
            if (((alive >> i) & 1u) && best < kPathInf) nd = best + ea_event_cost(n, s1, q2, lvl[i], wgt[i], off[i], S, cap);
            d[i] = nd;
            bits |= mv << (2 * i);
            p3 = p2; p2 = p1; p1 = cur;
            rel = rel + 1 == W ? 0 : rel + 1;
        }
        {
            long long* row = s_edge + (e & 1) * kEaMaxMove * kBandMaxThreads;
            row[tid] = d[kBandPer - 3]; row[kBandMaxThreads + tid] = d[kBandPer - 2]; row[2 * kBandMaxThreads + tid] = d[kBandPer - 1];
        }
        if (tid < nact) reinterpret_cast<unsigned short*>(bprow)[(long long)e * nact + tid] = (unsigned short)bits;
        __syncthreads();                                             // one barrier per step: the row of step e - 1 is free again
    }
    band_close(d, ok, N, W, tid, &s_fin, &s_bad);

    const long long fin = s_fin;
    const bool poisoned = s_bad != 0;
    if (poisoned || fin >= kPathInf) {
        band_refuse(poisoned, st_out, a.max_states + 1, es_out, a.max_events, a.score + b, a.band_hits + b, a.bad, tid, nthr);
        if (tid < 4) a.move_counts[4 * b + tid] = poisoned ? -1 : 0;
        return;
    }
    for (int j = N + tid; j <= a.max_states; j += nthr) st_out[j] = Tb;
    if (es_out)
        for (int e = E + tid; e < a.max_events; e += nthr) es_out[e] = -1;

    int s_end = N - 1, hits = 0;
    for (int e0 = (E - 1) / kBandTrace * kBandTrace; e0 >= 0; e0 -= kBandTrace) {
        const int nf = min(kBandTrace, E - e0);
        const int g0 = band_load_window<2, kEaMaxMove>(s_win, bprow, e0, nf, s_end, W, tid, nthr);       // (s_end - 192, s_end]
        __syncthreads();                                             // window loaded; s_path of the previous chunk was read
        if (tid == 0) {
            int s = s_end;
            for (int f = nf - 1; f >= 0; --f) {
                s_path[f + 1] = s;
                const unsigned w = s_win[f * kEaWinBytes + ((s >> 2) - g0)];
                const int mv = (int)((w >> (2 * (s & 3))) & 3u);
                s -= mv < s ? mv : s;                                // row 0 holds zeros: the state of event 0 stays
            }
            s_path[0] = e0 > 0 ? s : -1;
        }
        __syncthreads();
        for (int f = tid; f < nf; f += nthr) {
            const int before = s_path[f], pi = s_path[f + 1], e = e0 + f;
            if (es_out) es_out[e] = pi;
            if (e > 0) atomicAdd(&s_cnt[pi - before], 1);
            const int t = es[e];
            for (int j = before + 1; j <= pi; ++j) st_out[j] = t;    // a skipped state is empty: it begins where its successor does
            if (band_on_edge(pi, band_lo(e, N, E, W), N, W)) ++hits;
        }
        s_end = s_path[0];
    }
    if (hits) atomicAdd(&s_hits, hits);
    __syncthreads();
    if (tid < 4) a.move_counts[4 * b + tid] = s_cnt[tid];
    if (tid == 0) {
        a.score[b] = fin;
        a.band_hits[b] = s_hits;
    }
}

static bool ea_move_ok(int cost) { return cost == -1 || (cost >= 0 && cost < kEaMoveLimit); }

}  // namespace wn
using namespace wn;

// workspace: backpointers, 2 bits per (event, band slot), [B][max_events][band / 4] bytes
size_t wn_event_align_workspace_bytes(int batch, int max_events, int band) {
    return band_sizes_ok(batch, max_events, kEaMaxEvents, band) ? band_workspace_bytes(batch, max_events, band, 2) : 0;
}

int wn_event_align(const int* n_events, const int* ev_starts, const long long* ev_sum, const long long* ev_sumsq, const int* labels,
                   long long labels_stride, const int* label_lengths, const int* model, int batch, int max_events, int max_labels,
                   int max_states, int k, int first, int frac_bits, int weight_shift, int max_cost, int band, int move_cost0,
                   int move_cost1, int move_cost2, int move_cost3, int* starts, long long* score, int* event_state, int* move_counts,
                   int* band_hits, void* workspace, size_t workspace_bytes, int* bad, wn_stream_t stream) {
    if (batch < 1 || max_events < 1 || max_labels < 1 || max_states < 1 || labels_stride < 0) return WN_ERR_BAD_SHAPE;
    if (const int e = band_check_params(k, first, frac_bits, weight_shift, max_cost, band)) return e;
    if (move_cost1 < 0 || !ea_move_ok(move_cost0) || !ea_move_ok(move_cost1) || !ea_move_ok(move_cost2) || !ea_move_ok(move_cost3))
        return WN_ERR_UNSUPPORTED;
    if (batch > 65535 || max_events > kEaMaxEvents || max_states > kEaMaxEvents) return WN_ERR_UNSUPPORTED;
    if (!n_events || !ev_starts || !ev_sum || !ev_sumsq || !labels || !label_lengths || !model || !starts || !score || !move_counts ||
        !band_hits || !workspace)
        return WN_ERR_NULL;
    if (workspace_bytes < wn_event_align_workspace_bytes(batch, max_events, band) || ((size_t)workspace & 15)) return WN_ERR_WORKSPACE;

    EventAlignArgs a = {};
    a.n_events = n_events; a.ev_starts = ev_starts; a.ev_sum = ev_sum; a.ev_sumsq = ev_sumsq; a.labels = labels;
    a.label_lengths = label_lengths; a.model = model; a.labels_stride = labels_stride;
    a.B = batch; a.max_events = max_events; a.max_labels = max_labels; a.max_states = max_states; a.k = k; a.first = first;
    a.weight_shift = weight_shift; a.max_cost = max_cost; a.band = band;
    a.move_cost[0] = move_cost0; a.move_cost[1] = move_cost1; a.move_cost[2] = move_cost2; a.move_cost[3] = move_cost3;
    a.max_move = move_cost3 >= 0 ? 3 : move_cost2 >= 0 ? 2 : 1;
    a.starts = starts; a.score = score; a.event_state = event_state; a.move_counts = move_counts; a.band_hits = band_hits;
    a.bp = (unsigned char*)workspace; a.bad = bad;

    hipStream_t st = (hipStream_t)stream;
    const size_t lds = kEaFixedLds + (size_t)(3 << (2 * k)) * sizeof(int);       // 18.3 KiB and the table: 66.3 KiB at k = 6
    WN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(event_align_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
           "event_align attribute");
    hipLaunchKernelGGL(event_align_kernel, dim3((unsigned)batch), dim3(band_threads(band)), lds, st, a);
    WN_HIP(hipGetLastError(), "event_align");
    return WN_OK;
}
