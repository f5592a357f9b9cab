// The walk over an op string of wn_pair_align, once: one workgroup of 256 threads per read, the ops in tiles
// of 256 columns, and the reference / query index of every column as a ballot prefix sum.  Device code only.  pileup_kernel and
// pileup_evidence_kernel, which must mark the same reads, are built on it.  left_align_kernel and quality_profile_kernel use
// tile_scan and keep a hand-written copy of the validating pass (their timings, section 7u): a change to the definition below is
// made there too, and tests/test_gpu_opwalk.py holds all four to one verdict per row.
//
// A VALID OP ROW.  A read has n_ops op columns, n_ref reference and n_query query labels.  Walk index w is column w, or column
// n_ops - 1 - w of a reverse-strand read (rev).  Op 1 and 2 (aligned) and 3 consume a reference label, op 1, 2 and 4 a query label;
// i and j of a column are the labels consumed before it.  Every walker holds a row to
//   the header    0 <= n_ops <= max_ops and 0 <= n_query <= M; with a strand also strand <= 1, n_ref > 0 and the caller's window
//                 condition (head_ok).  Nothing of a read with a bad header is looked at: its row has n = 0.
//   every column  the op in 1..4; i < n_ref where it consumes a reference label and j < n_query where it consumes a query label,
//                 BEFORE anything is loaded at i or j;
//   the totals    the ops consume exactly n_ref and n_query labels,
// and each adds, through validate_ops' hook, which may load at i / j only where in_ref / in_query says so:
//   pileup_kernel, pileup_evidence_kernel   window lo >= 0 and lo + n_ref <= R; qual <= 93 (with qual)
//   left_align_kernel                       window n_ref <= N; nothing per column
//   quality_profile_kernel                  no strand, 0 <= n_ref <= N; labels in [0, classes), op 1 / 2 against the labels,
//                                           qual <= 93, dwell >= 0
// A read with strand < 0, n_ref == 0 or keep[b] == 0 is skipped before any of this (read_skipped; left_align_kernel has no keep,
// quality_profile_kernel no strand: it skips nothing); the caller writes its own `skipped` and `bad` outputs beside report_bad.
//
// BARRIERS (the rule of section 7r: a helper holds only the barriers that produce its result).  tile_scan: one.  walk_ops: one per
// tile, tile_scan's.  validate_ops: one per tile and one at the end, after which lo / hi / bad are read.
// validate_begin: none -- the caller puts one barrier between it and validate_ops, with whatever else it initialises in LDS.
// SLOTS.  tile_scan's two slots alternate by OpWalk::tile, which counts every tile the workgroup scans through all its passes and is
// never reset: a slot is written again two tiles later at the earliest, with the barrier of the tile between.  A reset would be
// safe only behind a barrier that every wave passes after its last read of the slots, such as the one that ends validate_ops.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>

#include "wn_wave_dev.h"

namespace wn {

constexpr int kPThreads = 256;                // threads of a workgroup = op columns of a tile
constexpr int kPWaves = kPThreads / 64;
constexpr int kPQualRows = 94;                // qual 0..93

// The exclusive prefix sums of two 0/1 values over the 256 columns of a tile, on top of the running bases, which move on by
// the tile's totals.  Every thread of the workgroup calls it; `slot` alternates from tile to tile.
__device__ __forceinline__ void tile_scan(bool is_ref, bool is_query, int tid, int (*slot)[kPWaves], int* base_ref,
                                          int* base_query, int* i_c, int* j_c) {
    const int lane = tid & 63, wave = tid >> 6;
    const unsigned long long m_ref = __ballot(is_ref), m_query = __ballot(is_query);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (lane == 0) {
        slot[0][wave] = __popcll(m_ref);
        slot[1][wave] = __popcll(m_query);
    }
    __syncthreads();
    int off_ref, off_query, tot_ref, tot_query;
    wave_offsets<kPWaves>(slot[0], wave, &off_ref, &tot_ref);
    wave_offsets<kPWaves>(slot[1], wave, &off_query, &tot_query);
    *i_c = *base_ref + off_ref + __popcll(m_ref & below);
    *j_c = *base_query + off_query + __popcll(m_query & below);
    *base_ref += tot_ref;
    *base_query += tot_query;
}

// ---- the row of a read and a column of it ---------------------------------------------------------------------------------------
struct OpCol {
    int w, op, i, j;                          // walk index, op (0 where inactive), labels consumed before it (after tile_scan)
    bool active, is_ref, is_query;
};

struct OpRow {
    const unsigned char* ops;
    int n, n_ref, n_query;                    // n: the op columns that are walked, 0 with a bad header
    bool rev;
    __device__ __forceinline__ int column(int w) const { return rev ? n - 1 - w : w; }
    // the column at walk index w, classified; i and j are tile_scan's to fill
    __device__ __forceinline__ OpCol load(int w) const {
        const bool active = w < n;
        const int op = active ? (int)ops[column(w)] : 0;
        return {w, op, 0, 0, active, op >= 1 && op <= 3, op == 1 || op == 2 || op == 4};
    }
};

__device__ __forceinline__ bool read_skipped(int strand, int n_ref, const unsigned char* keep, int b) {
    return strand < 0 || n_ref == 0 || (keep && keep[b] == 0);
}
__device__ __forceinline__ bool head_ok(int strand, int n_ref, bool window_ok, int n_query, int M, int n_ops, int max_ops) {
    return strand <= 1 && n_ref > 0 && window_ok && n_query >= 0 && n_query <= M && n_ops >= 0 && n_ops <= max_ops;
}
__device__ __forceinline__ OpRow op_row(const unsigned char* ops, bool header_ok, int n_ops, int n_ref, int n_query, bool rev) {
    return {ops, header_ok ? n_ops : 0, n_ref, n_query, rev};
}

// ---- the walk -------------------------------------------------------------------------------------------------------------------
struct OpWalk {                               // what a workgroup carries through its walks, the same in every thread
    int (*slot)[2][kPWaves];                  // the kernel's `__shared__ int s_slot[2][2][kPWaves]`, tile_scan's two slots
    int tile = 0;                             // tiles scanned so far: the slot is tile & 1 (SLOTS above)
    int base_ref = 0, base_query = 0;         // the labels consumed before the tile; after a walk, the totals
    __device__ __forceinline__ void scan(OpCol* c, int tid) {
        tile_scan(c->is_ref, c->is_query, tid, slot[tile & 1], &base_ref, &base_query, &c->i, &c->j);
        ++tile;
    }
};

// One pass over the row front to back: body(column) in every thread for every tile, inactive columns included (the body's
// ballots need them), with i and j filled in.
template <class Body>
__device__ __forceinline__ void walk_ops(const OpRow& r, int tid, OpWalk* walk, Body&& body) {
    walk->base_ref = walk->base_query = 0;
    for (int t0 = 0; t0 < r.n; t0 += kPThreads) {
        OpCol c = r.load(t0 + tid);
        walk->scan(&c, tid);
        body(c);
    }
}

struct OpSpan {
    int first, last;                          // the first and last aligned (op 1 or 2) walk index; last < 0: there is none
    bool bad;
};

// lo, hi, bad: three `__shared__ int` of the kernel (one LDS variable of 12 bytes would be padded to 16)
__device__ __forceinline__ void validate_begin(int tid, bool header_ok, int* lo, int* hi, int* bad) {
    if (tid == 0) { *lo = INT_MAX; *hi = -1; *bad = header_ok ? 0 : 1; }
}

// The validating pass: what every walker checks (above), and extra(column, in_ref, in_query) -> "still good" for what the caller
// adds.  The verdict and the span are the same in every thread.
template <class Extra>
__device__ __forceinline__ OpSpan validate_ops(const OpRow& r, int tid, OpWalk* walk, int* lo, int* hi, int* bad, Extra&& extra) {
    bool ok = true;
    int first = INT_MAX, last = -1;
    walk_ops(r, tid, walk, [&](const OpCol& c) {
        if (!c.active) return;
        if (c.op < 1 || c.op > 4) { ok = false; return; }
        const bool in_ref = c.is_ref && c.i < r.n_ref, in_query = c.is_query && c.j < r.n_query;    // checked before used as an index
        if (c.is_ref != in_ref || c.is_query != in_query) ok = false;
        if (!extra(c, in_ref, in_query)) ok = false;
        if (c.op <= 2) {
            first = c.w < first ? c.w : first;
            last = c.w > last ? c.w : last;
        }
    });
    if (walk->base_ref != r.n_ref || walk->base_query != r.n_query) ok = false;                     // the ops consume exactly the labels
    if (!ok) atomicOr(bad, 1);
    if (last >= 0) { atomicMin(lo, first); atomicMax(hi, last); }
    __syncthreads();
    return {*lo, *hi, *bad != 0};
}

__device__ __forceinline__ void report_bad(int tid, int* bad) { if (tid == 0 && bad) atomicAdd(bad, 1); }

}  // namespace wn
