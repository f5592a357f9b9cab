// Indel left-alignment of the op strings wn_pair_align wrote: every gap run of a row moves as far toward the
// START OF THE FORWARD STRAND as the two sequences allow, so that forward and reverse reads pile the gaps of a repeat alike.  The
// definition is in include/wavenet_amd.h; tests/leftalign_ref.py states it as plain loops and the kernel equals it bit for bit.
//
//   left_align_kernel   grid (batch), 256 threads, ONE WORKGROUP PER READ, the row in tiles of 256 columns (wn_opscan.h).  A
//                       reverse-strand read is walked back to front by index arithmetic, as pileup_kernel does: walk index w is
//                       column n - 1 - w, reference index n_ref - 1 - i, query index n_query - 1 - j.
//     copy      the whole row goes to ops_out byte by byte, whatever it holds; a skipped or a bad read ends there.
//     validate  the validating pass of wn_opscan.h without the window and the qual, KEPT BY HAND here: op
//               codes, i / j against the lengths, the totals, and the first and last aligned walk index.
//     passes    every pass is ONE SWEEP OVER THE TILES FROM THE LAST TO THE FIRST, in place on ops_out.  What a column needs lies
//               at or above it: D, the first column above whose op differs (the end of its stretch); c, the first gap column
//               above (with v = op[c] and l = D(c) - c: the next run); and NS, the first STOPPER at or above it.  A stopper is a
//               gap column, a column at or before `first`, an aligned column whose next run starts at or after `last`, or an
//               aligned column w whose label differs from the one l further on in the run's own sequence (a for v = 3, b for
//               v = 4, at w's own i or j: between the barrier and the run every column consumes both).  The run at c then shifts
//               by the number of non-stoppers directly below it, and an aligned column w is a MOVER -- one of the s columns the
//               run passes -- exactly if NS(w) = c.  All three are first-set-bit searches in ballots, across the waves through
//               LDS and across tiles through a carried state of the columns above the tile: the op and D of its first column,
//               (c, v, D(c)) of its first gap column, its first stopper.
//               The rewrite is the movers' alone: mover w writes v over its own column (A), then -- a barrier later -- its op at
//               w + l (B).  Column p of the territory (g, c + l) so ends as op[p - l] if p - l is a mover, else as v if it is a
//               mover or a column of the run, which is the definition: the run at [c - s, c - s + l), the s columns after it.
//               IN PLACE IS SAFE: a tile's columns are in registers before anything is written into it (a column is loaded once
//               per pass, at the top of its tile's step); a write goes to the mover's own tile or a later one, which this pass
//               has read already; territories are disjoint, so a column has at most one B writer, and its A write comes first
//               (the same step before the barrier, or an earlier step).  Index sums (i, j) are taken on the pass's input.
//               A pass in which no column moved ends the loop (settled); __syncthreads_or is that vote and the fence between
//               one pass's stores and the next one's loads, which stay inside the workgroup.
// One launch; no workgroup waits on another.  No floating point, no workspace, no scratch, no atomics but the bad count.  No value
// of an op, a label or a length is used as an index before it is checked.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_opscan.h"
#include <limits.h>

namespace wn {

constexpr int kLMaxPasses = 64;
constexpr int kLNone = INT_MAX;

struct LeftAlignArgs {
    const unsigned char* ops_in;        // row b at ops_in + b * ops_stride
    unsigned char* ops_out;             // row b at ops_out + b * out_stride
    const int* ops_len;
    const int* ref;
    const int* ref_len;
    const int* query;
    const int* query_len;
    const int* strand;
    long long ops_stride, out_stride, ref_stride, query_stride;
    int* passes;
    signed char* settled;
    int* bad;
    int B, N, M, max_ops, max_passes;
};

// the lowest set lane of a ballot as a walk index, kLNone for an empty one
__device__ __forceinline__ int first_set(unsigned long long m, int wave_base) { return m ? wave_base + __ffsll((long long)m) - 1 : kLNone; }

__global__ __launch_bounds__(kPThreads) void left_align_kernel(const LeftAlignArgs a) {
    __shared__ int s_slot[2][2][kPWaves];
    __shared__ int s_first_op[kPWaves], s_first_diff[kPWaves], s_first_gap[kPWaves], s_first_stop[kPWaves];
    __shared__ int s_end[kPThreads];              // D of the tile's columns
    __shared__ unsigned char s_op[kPThreads];
    __shared__ int s_lo, s_hi, s_bad;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    const unsigned char* in = a.ops_in + (long long)b * a.ops_stride;
    unsigned char* out = a.ops_out + (long long)b * a.out_stride;
    for (int c = tid; c < a.max_ops; c += kPThreads) out[c] = in[c];

    const int strand = a.strand[b], n_ref = a.ref_len[b];
    if (strand < 0 || n_ref == 0) {                                  // skipped: nothing else of the read is looked at
        if (tid == 0) { a.passes[b] = 0; a.settled[b] = 1; }
        return;
    }
    const int n_ops = a.ops_len[b], n_query = a.query_len[b];
    const bool head_ok = strand <= 1 && n_ref > 0 && n_ref <= a.N && n_query >= 0 && n_query <= a.M && n_ops >= 0 && n_ops <= a.max_ops;
    const int n = head_ok ? n_ops : 0;                               // nothing of a read with a bad header is looked at
    const bool rev = strand == 1;
    const int* ref = a.ref + (long long)b * a.ref_stride;
    const int* query = a.query + (long long)b * a.query_stride;

    if (tid == 0) { s_lo = INT_MAX; s_hi = -1; s_bad = head_ok ? 0 : 1; }
    __syncthreads();

    // ---- validate: op codes, i / j against the lengths, the totals; the first / last aligned walk index
    bool ok = true;
    int first = INT_MAX, last = -1, base_ref = 0, base_query = 0, slot = 0;
    for (int t0 = 0; t0 < n; t0 += kPThreads, slot ^= 1) {
        const int w = t0 + tid;
        const bool active = w < n;
        const int op = active ? (int)in[rev ? n - 1 - w : w] : 0;
        const bool is_ref = op >= 1 && op <= 3, is_query = op == 1 || op == 2 || op == 4;
        int i, j;
        tile_scan(is_ref, is_query, tid, s_slot[slot], &base_ref, &base_query, &i, &j);
        if (!active) continue;
        if (op < 1 || op > 4) { ok = false; continue; }
        if (is_ref && i >= n_ref) ok = false;
        if (is_query && j >= n_query) ok = false;
        if (op <= 2) {
            first = w < first ? w : first;
            last = w > last ? w : last;
        }
    }
    if (base_ref != n_ref || base_query != n_query) ok = false;      // the ops consume exactly the labels
    if (!ok) atomicOr(&s_bad, 1);
    if (last >= 0) { atomicMin(&s_lo, first); atomicMax(&s_hi, last); }
    __syncthreads();                                                 // and the copy of the row is in place for every wave
    if (s_bad != 0) {
        if (tid == 0) {
            a.passes[b] = 0;
            a.settled[b] = -1;
            if (a.bad) atomicAdd(a.bad, 1);
        }
        return;
    }
    first = s_lo;
    last = s_hi;

    // ---- the passes.  The ops are loaded again from ops_out; every index below was checked above on the same values (a pass only
    // permutes the columns between two aligned ones) and is checked again before it is used
    const unsigned long long above = lane == 63 ? 0ull : ~0ull << (lane + 1), at_or_above = ~0ull << lane;
    const int top = last >= 0 ? (n - 1) / kPThreads * kPThreads : -1;
    int n_passes = 0, settled = 0;
    for (int pass = 0; pass < a.max_passes; ++pass) {
        int carry_op = 0, carry_end = n;                             // of the first column above the tile: its op and D
        int gap_c = kLNone, gap_v = 0, gap_end = 0;                  // of the first gap column above the tile
        int stop_c = kLNone;                                         // the first stopper above the tile
        int after_ref = n_ref, after_query = n_query;                // labels consumed up to the end of the tile
        bool moved = false;
        for (int t0 = top; t0 >= 0; t0 -= kPThreads, slot ^= 1) {
            const int w = t0 + tid, wave_base = t0 + wave * 64;
            const bool active = w < n;
            const int col = rev ? n - 1 - w : w;
            const int op = active ? (int)out[col] : 0;
            const bool is_ref = op >= 1 && op <= 3, is_query = op == 1 || op == 2 || op == 4;
            const unsigned long long m1 = __ballot(op == 1), m2 = __ballot(op == 2), m3 = __ballot(op == 3), m4 = __ballot(op == 4);
            const unsigned long long m_gap = m3 | m4;
            const unsigned long long mine = op == 1 ? m1 : op == 2 ? m2 : op == 3 ? m3 : op == 4 ? m4 : ~(m1 | m2 | m_gap);
            if (lane == 0) {
                s_first_op[wave] = op;
                s_first_diff[wave] = first_set(~mine, wave_base);
                s_first_gap[wave] = first_set(m_gap, wave_base);
            }
            int tile_ref = 0, tile_query = 0, i, j;
            tile_scan(is_ref, is_query, tid, s_slot[slot], &tile_ref, &tile_query, &i, &j);      // barrier 1 is in here
            after_ref -= tile_ref;
            after_query -= tile_query;
            i += after_ref;
            j += after_query;

            int end = first_set(~mine & above, wave_base);           // D: where this column's stretch of one op ends
            int c = first_set(m_gap & above, wave_base);             // the first gap column above
            bool open = end == kLNone;
#pragma unroll
            for (int v = 1; v < kPWaves; ++v) {
                if (v <= wave) continue;
                if (open) {
                    if (s_first_op[v] != op) { end = t0 + v * 64; open = false; }
                    else if (s_first_diff[v] != kLNone) { end = s_first_diff[v]; open = false; }
                }
                if (c == kLNone) c = s_first_gap[v];
            }
            if (open) end = carry_op != op ? t0 + kPThreads : carry_end;
            s_end[tid] = end;
            s_op[tid] = (unsigned char)op;
            __syncthreads();                                         // barrier 2

            int v = gap_v, run_end = gap_end;                        // the next run: its op and where it ends
            if (c != kLNone) { v = s_op[c - t0]; run_end = s_end[c - t0]; }
            else c = gap_c;
            const bool candidate = active && (op == 1 || op == 2) && w > first && c < last;
            const int l = candidate ? run_end - c : 0;
            bool stop = true;
            if (candidate && (v == 3 || v == 4) && l > 0) {
                const int* seq = v == 3 ? ref : query;
                const int len = v == 3 ? n_ref : n_query, x = v == 3 ? i : j;
                if (x >= 0 && (long long)x + l < len) stop = seq[rev ? len - 1 - x : x] != seq[rev ? len - 1 - x - l : x + l];
            }
            const unsigned long long m_stop = __ballot(stop);
            if (lane == 0) s_first_stop[wave] = first_set(m_stop, wave_base);
            // the state of this tile for the ones below it (the same in every thread)
            carry_op = s_op[0];
            carry_end = s_end[0];
            int tile_gap = kLNone;
#pragma unroll
            for (int u = kPWaves - 1; u >= 0; --u) tile_gap = s_first_gap[u] != kLNone ? s_first_gap[u] : tile_gap;
            if (tile_gap != kLNone) { gap_c = tile_gap; gap_v = s_op[tile_gap - t0]; gap_end = s_end[tile_gap - t0]; }
            __syncthreads();                                         // barrier 3

            int ns = first_set(m_stop & at_or_above, wave_base);
            int tile_stop = kLNone;
#pragma unroll
            for (int u = kPWaves - 1; u >= 0; --u) {
                const int f = s_first_stop[u];
                if (f != kLNone) {
                    tile_stop = f;
                    if (u > wave && (m_stop & at_or_above) == 0) ns = f;         // descending u: the lowest wave above wins
                }
            }
            if (ns == kLNone) ns = stop_c;
            if (tile_stop != kLNone) stop_c = tile_stop;
            const bool mover = !stop && ns == c && (long long)w + l < n;
            if (mover) out[col] = (unsigned char)v;                  // (A)
            __syncthreads();                                         // barrier 4: A before B, also across waves
            if (mover) out[rev ? n - 1 - (w + l) : w + l] = (unsigned char)op;   // (B)
            moved = moved || mover;
        }
        if (__syncthreads_or(moved ? 1 : 0) == 0) { settled = 1; break; }
        ++n_passes;
    }
    if (tid == 0) { a.passes[b] = n_passes; a.settled[b] = (signed char)settled; }
}

}  // namespace wn
using namespace wn;

int wn_gap_left_align(const unsigned char* ops_in, long long ops_stride, const int* ops_len, const int* ref, long long ref_stride,
                      const int* ref_lengths, const int* query, long long query_stride, const int* query_lengths, const int* strand,
                      int batch, int max_ref_len, int max_query_len, int max_ops, int max_passes, unsigned char* ops_out,
                      long long out_stride, int* passes, signed char* settled, void* workspace, size_t workspace_bytes, int* bad,
                      wn_stream_t stream) {
    (void)workspace, (void)workspace_bytes;                          // the passes run in place on ops_out: none is needed
    if (const int s = check_op_rows(batch, max_query_len, max_ops, ops_stride, query_stride,
                                    max_ref_len >= 1 && max_passes >= 1 && ref_stride >= 0 && out_stride >= 0,
                                    max_ref_len <= kPaMaxRef && max_passes <= kLMaxPasses,
                                    ops_in && ops_len && ref && ref_lengths && query && query_lengths && strand && ops_out && passes && settled))
        return s;
    if (ops_out == ops_in) return WN_ERR_UNSUPPORTED;                // the input stays as it is: no aliasing
    LeftAlignArgs a = {};
    a.ops_in = ops_in; a.ops_out = ops_out; a.ops_len = ops_len; a.ref = ref; a.ref_len = ref_lengths; a.query = query;
    a.query_len = query_lengths; a.strand = strand;
    a.ops_stride = ops_stride; a.out_stride = out_stride; a.ref_stride = ref_stride; a.query_stride = query_stride;
    a.passes = passes; a.settled = settled; a.bad = bad;
    a.B = batch; a.N = max_ref_len; a.M = max_query_len; a.max_ops = max_ops; a.max_passes = max_passes;
    hipLaunchKernelGGL(left_align_kernel, dim3(batch), dim3(kPThreads), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "gap_left_align");
    return WN_OK;
}
