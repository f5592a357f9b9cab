// The banded-path core that the signal alignment (wn_sigalign.hip) and the event alignment
// (wn_eventalign.hip, section 7n) share.  ONE definition each: both make the starts that wn_kmer_events consumes and both document
// the same lo() in the C header, so a band that differed between them would be a silent divergence.
//
// A read has n steps (samples or events) and N states (k-mers); a monotone path may be in state j at step i iff
// lo(i) <= j < lo(i) + W, the band of width W around the diagonal.
//
//   slots     state j lives in SLOT j mod W.  A workgroup has W / 8 threads at work (rounded up to whole waves: one wave up to
//             W = 512, four at 2048) and every thread owns 8 consecutive slots with their running costs (int64) and their three
//             model integers in registers, so the band advances without moving anything.  The per-slot arrays are only ever
//             indexed by unrolled constants -- `if (i == (slot & 7))` selects, never `x[slot & 7]` -- so that they stay registers.
//   entry     when lo rises past state r, state r + W enters the band in the slot r mod W that r leaves: band_enter re-arms that
//             slot's model row from the k-mer codes of the next 256 entering states, staged in LDS whenever r is a multiple of 256.
//             The staging has a barrier on BOTH sides: the leading one because several rises can share a step (the code of state
//             r - 1 + W may have been fetched in this same step); where lo rises by at most one per step it is not needed, and
//             costs one barrier per 256 rises against the 256 or more per-step barriers of the recurrence between them.
//             What the recurrence makes of the slot's old cost in the step of the entry is the kernel's own business.
//   closing   band_close picks the cost of state N - 1 out of its slot and poisons the read if any thread saw bad input;
//             band_refuse is the one fill of a read without a result (bad, or no alignment).
//   trace     backwards in chunks of kBandTrace steps.  A path that moves at most M states per step and ends a chunk in state s
//             needs the backpointers of the states (s - 64 M, s] only: band_load_window brings those bytes of every row of the
//             chunk into LDS.  Walking the window (1-bit against 2-bit backpointers) and what is written per step differ between
//             the kernels and sharing them would take a policy type, so each kernel keeps its own walk.
//
// Device functions are __forceinline__ and take the per-slot registers by reference; everything a kernel can decide differently
// (LDS layout, recurrence, costs, input staging, outputs) stays in its own file.
#pragma once
#include "../../include/wavenet_amd.h"
#include "wn_signal_dev.h"

namespace wn {

constexpr int kBandPer = 8;                   // consecutive band slots per thread
constexpr int kBandMaxThreads = 256;          // band 2048
constexpr int kBandMin = 64;
constexpr int kBandMax = 2048;                // and a multiple of 64
constexpr int kBandCodes = 256;               // k-mer codes staged for the states that enter the band next
constexpr int kBandTrace = 64;                // steps walked at a time by the trace

// lo(i): the first state of the band at step i of n, N states, width W
__host__ __device__ __forceinline__ int band_lo(long long i, int N, int n, int W) {
    const long long c = ((2 * i + 1) * (long long)N) / (2 * (long long)n);
    const long long top = N > W ? N - W : 0;
    long long lo = c - W / 2;
    lo = lo < 0 ? 0 : lo;
    return (int)(lo > top ? top : lo);
}

// band_lo carried from step to step without a division: (2 i + 1) N = c 2 n + rem.  Starts at step 0, where lo = 0.
struct BandCursor {
    long long rem, two_N, two_n;
    int c, lo, lo_slot, top, W;                                      // lo_slot = lo mod W
    __host__ __device__ __forceinline__ BandCursor(int N, int n, int W_)
        : rem(N), two_N(2ll * N), two_n(2ll * n), c(0), lo(0), lo_slot(0), top(N > W_ ? N - W_ : 0), W(W_) {}
    // to the next step; returns lo(i) - lo(i - 1) >= 0.  The loop runs N / n times rounded up at the most: once where N <= n
    __host__ __device__ __forceinline__ int advance() {
        rem += two_N;
        while (rem >= two_n) { rem -= two_n; ++c; }
        int ln = c - W / 2;
        ln = ln < 0 ? 0 : ln;
        ln = ln > top ? top : ln;
        const int delta = ln - lo;                                   // the centre never falls and the clamps are monotone: >= 0
        lo = ln;
        lo_slot = lo_slot + delta >= W ? lo_slot + delta - W : lo_slot + delta;
        return delta;
    }
};

// the path's state pi at a step whose band starts at lo lies on the band's edge while the band could have been wider there
__host__ __device__ __forceinline__ bool band_on_edge(int pi, int lo, int N, int W) {
    return (pi == lo && lo > 0) || (pi == lo + W - 1 && lo + W < N);
}

// this thread's slots 8 tid .. 8 tid + 7 start as the states of the same numbers; state j is the window lab[j .. j + k)
__device__ __forceinline__ void band_arm(const int* s_model, const int* lab, int k, int N, int W, int tid, int (&lvl)[kBandPer],
                                         int (&wgt)[kBandPer], int (&off)[kBandPer], long long (&d)[kBandPer], unsigned& alive,
                                         bool& ok) {
    alive = 0;
#pragma unroll
    for (int i = 0; i < kBandPer; ++i) {
        const int j = kBandPer * tid + i;
        lvl[i] = 0; wgt[i] = 1; off[i] = 0;
        d[i] = kPathInf;
        if (tid < W / kBandPer && j < N) {                           // j + k <= N + k - 1: inside the labels
            const int code = kmer_code(lab + j, k, &ok);
            sa_model_row(s_model, code, &lvl[i], &wgt[i], &off[i], &ok);
            alive |= 1u << i;
        }
    }
}

// lo rises past state r: state r + W <= N - 1 enters the band in slot `slot` = r mod W.  Workgroup-uniform; holds barriers
__device__ __forceinline__ void band_enter(int r, int slot, const int* s_model, int* s_code, const int* lab, int k, int N, int W,
                                           int tid, int nthr, int (&lvl)[kBandPer], int (&wgt)[kBandPer], int (&off)[kBandPer],
                                           bool& ok) {
    if ((r & (kBandCodes - 1)) == 0) {
        __syncthreads();                                             // the code of state r - 1 + W has been read
        for (int u = tid; u < kBandCodes; u += nthr) {
            const long long j = (long long)W + r + u;
            int code = 0;
            if (j < N) code = kmer_code(lab + j, k, &ok);
            s_code[u] = code;
        }
        __syncthreads();
    }
    if ((slot >> 3) == tid) {
        int l, w, o;
        sa_model_row(s_model, s_code[r & (kBandCodes - 1)], &l, &w, &o, &ok);
#pragma unroll
        for (int u = 0; u < kBandPer; ++u) {                         // selects of values, not eight guarded stores: through the
            const bool hit = u == (slot & 7);                        // references those compile to a switch with a copy of the
            const int pl = lvl[u], pw = wgt[u], po = off[u];         // slot registers per arm, 1 % of event_align's step
            lvl[u] = hit ? l : pl; wgt[u] = hit ? w : pw; off[u] = hit ? o : po;
        }
    }
}

// after the last step: the cost of state N - 1 into *s_fin, a thread's bad input into *s_bad; behind its barrier both, and this
// workgroup's backpointer rows, are visible
__device__ __forceinline__ void band_close(const long long (&d)[kBandPer], bool ok, int N, int W, int tid, long long* s_fin,
                                           int* s_bad) {
    const int fs = (N - 1) % W;                                      // the slot of the last state
    if ((fs >> 3) == tid) {
#pragma unroll
        for (int i = 0; i < kBandPer; ++i)
            if (i == (fs & 7)) *s_fin = d[i];
    }
    if (!ok) atomicOr(s_bad, 1);
    __syncthreads();
}

// a read without a result: starts [n_starts] and the optional per-step states [n_steps] -1; a bad read scores kPathBadRead with
// band_hits -1 and is counted, a read without an alignment kPathNone with band_hits 0.  score and band_hits are the read's own
__device__ __forceinline__ void band_refuse(bool bad_read, int* starts, int n_starts, int* steps, int n_steps, long long* score,
                                            int* band_hits, int* bad, int tid, int nthr) {
    for (int j = tid; j < n_starts; j += nthr) starts[j] = -1;
    if (steps)
        for (int i = tid; i < n_steps; i += nthr) steps[i] = -1;
    if (tid == 0) {
        *score = bad_read ? kPathBadRead : kPathNone;
        *band_hits = bad_read ? -1 : 0;
        if (bad_read && bad) atomicAdd(bad, 1);
    }
}

// backpointer bytes per step of a trace window: kBits per slot, a path that moves kMaxMove states per step at the most
template <int kBits, int kMaxMove>
constexpr int kBandWinBytes = kMaxMove * kBandTrace * kBits / 8 + 1;

// the window (s_end - kMaxMove 64, s_end] of the nf rows from step i0 on into s_win [nf][kBandWinBytes]; a row of the workspace
// is W kBits / 8 bytes and the byte of state j is (j mod W) kBits / 8.  Returns the window's first byte, before the wrap
template <int kBits, int kMaxMove>
__device__ __forceinline__ int band_load_window(unsigned char* s_win, const unsigned char* bprow, int i0, int nf, int s_end, int W,
                                                int tid, int nthr) {
    constexpr int kWin = kBandWinBytes<kBits, kMaxMove>;
    const int row = W * kBits / 8;
    const int g0 = max(s_end - (kMaxMove * kBandTrace - 1), 0) * kBits / 8;
    for (int i = tid; i < nf * kWin; i += nthr) {
        const int f = i / kWin, g = g0 + (i - f * kWin);
        s_win[i] = bprow[(long long)(i0 + f) * row + g % row];
    }
    return g0;
}

// host: what both entry points check of a band and its parameters, and what they size by it
inline bool band_ok(int band) { return band >= kBandMin && band <= kBandMax && band % 64 == 0; }

inline bool band_sizes_ok(int batch, int rows, int max_rows, int band) {
    return batch >= 1 && batch <= 65535 && rows >= 1 && rows <= max_rows && band_ok(band);
}

// the backpointers, [batch][rows][band bits_per_slot / 8] bytes
inline size_t band_workspace_bytes(int batch, int rows, int band, int bits_per_slot) {
    return ((size_t)batch * (size_t)rows * (size_t)(band * bits_per_slot / 8) + 15) / 16 * 16;
}

inline int band_threads(int band) { return (band / kBandPer + 63) / 64 * 64; }   // one wave up to band 512, four at 2048

inline int band_check_params(int k, int first, int frac_bits, int weight_shift, int max_cost, int band) {
    if (k < 1 || k > kSigMaxK || first < 0 || first > kSigMaxFirst || frac_bits < 0 || frac_bits > kSigMaxFrac) return WN_ERR_UNSUPPORTED;
    if (weight_shift < 16 || weight_shift > 63 || max_cost < 1) return WN_ERR_UNSUPPORTED;
    return band_ok(band) ? WN_OK : WN_ERR_UNSUPPORTED;
}

}  // namespace wn
