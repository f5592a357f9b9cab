// Signal-to-base alignment under the k-mer pore model: raw samples against the k-mers of KNOWN bases, the
// minimum-cost monotone path (every sample stays in its k-mer or steps to the next one, no skips) inside a band around the
// diagonal.  What nanopolish `eventalign` does before the reference's utils/dump_distributions.py reads its output, and the
// segmentation that wn_kmer_events (wn_events.hip, section 7j) takes.  Everything after the quantisation of a sample is integer.
//
//   signal_align_kernel<T>   one workgroup per read, band / 8 threads at work (rounded up to whole waves), two phases in one launch.
//
//     forward   cost_t(j) = min(cost_{t-1}(j), cost_{t-1}(j-1)) + sample_cost(q_t, model[kmer_j]) over the states of the band
//               [lo(t), lo(t) + W).  State j lives in SLOT j mod W and every thread owns 8 consecutive slots with their running
//               costs (int64) and their three model integers in registers, so the band advances without moving anything: when
//               lo rises by one (it never rises by more), the slot of the state that left is re-armed for state lo + W - 1 --
//               its stay predecessor is +inf for this one step and its model row is fetched from the table in LDS.  One value
//               crosses threads per step: the last slot of the left neighbour, cyclic over the band, through a double-buffered
//               LDS row and ONE workgroup barrier per step (with band <= 512 the workgroup is one wave).  The state at lo(t)
//               has no step predecessor unless lo has just risen (lo(t) - 1 was outside the band at t - 1).  The eight 1-bit
//               backpointers of a thread are one byte store to the workspace, bp[b][t][W / 8].  Samples are quantised 1024 at a
//               time into LDS, the k-mer codes of the states about to enter the band 256 at a time; both passes validate.
//     trace     backwards in chunks of 64 samples.  The path moves at most one state per sample, so a chunk that ends in state
//               s reads the backpointer bytes of the states (s - 64, s] only: 9 bytes per sample, loaded into LDS by all
//               threads; one lane walks the 64 steps in LDS, then the threads write sample_state, the starts of the states that
//               begin in the chunk and count the samples on the band's edge.
//
// Ties (tests/signal_align_ref.py holds the same rule): the stay predecessor is taken first, the step predecessor replaces it
// only if strictly smaller.  No value of a length, a label or a sample is used as an index before it is checked; a read found
// bad anywhere in the forward phase gets its outputs from the fill at the end, never from the trace.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"
#include "wn_signal_dev.h"

namespace wn {

constexpr int kSaPer = 8;                     // consecutive band slots per thread
constexpr int kSaMaxThreads = 256;            // band 2048
constexpr int kSaSamples = 1024;              // samples quantised into LDS at a time
constexpr int kSaCodes = 256;                 // k-mer codes staged for the states that enter the band next
constexpr int kSaTrace = 64;                  // samples walked at a time by the trace
constexpr int kSaWinBytes = kSaTrace / 8 + 1; // backpointer bytes per sample of a trace window
constexpr int kSaMinBand = 64;
constexpr int kSaMaxBand = 2048;
constexpr int kSaMaxSignal = 1 << 24;
constexpr int kSaMaxEvents = 1 << 20;
constexpr long long kSaInf = 1ll << 62;       // a path's cost stays below 2^24 (2^31 + 2^30) < 2^56
constexpr long long kSaNoAlignment = 0x7fffffffffffffffll;
constexpr long long kSaBadRead = -0x7fffffffffffffffll - 1;

struct SigAlignArgs {
    const void* signal;
    const int* signal_lengths;
    const float* scale_shift;           // [B][2] or nullptr
    const int* labels;
    const int* label_lengths;
    const int* model;                   // [4^k][3]: level, weight, offset
    long long signal_stride, labels_stride;
    int B, max_signal, max_labels, max_events, k, first, weight_shift, max_cost, band;
    double two_f;                       // 2^frac_bits
    int* starts;                        // [B][max_events + 1]
    long long* score;                   // [B]
    int* band_hits;                     // [B]
    int* sample_state;                  // [B][max_signal] or nullptr
    unsigned char* bp;                  // workspace: [B][max_signal][band / 8]
    int* bad;
};

// lo(t): the first state of the band at sample t
__device__ __forceinline__ int sa_band_lo(long long t, int N, int T, int W) {
    const long long c = ((2 * t + 1) * (long long)N) / (2 * (long long)T);
    const long long top = N > W ? N - W : 0;
    long long lo = c - W / 2;
    lo = lo < 0 ? 0 : lo;
    return (int)(lo > top ? top : lo);
}

template <typename T>
__global__ __launch_bounds__(kSaMaxThreads) void signal_align_kernel(const SigAlignArgs a) {
    extern __shared__ __attribute__((aligned(16))) char sa_smem[];
    int* s_model = reinterpret_cast<int*>(sa_smem);                  // [4^k][3]
    __shared__ int s_q[kSaSamples];
    __shared__ int s_code[kSaCodes];
    __shared__ long long s_edge[2][kSaMaxThreads];                   // every thread's last slot, by step parity
    __shared__ unsigned char s_win[kSaTrace * kSaWinBytes];
    __shared__ int s_path[kSaTrace + 1];                             // [0] the state before the chunk, [1 + f]
    __shared__ long long s_fin;
    __shared__ int s_bad, s_hits;
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int W = a.band, nact = W / kSaPer, k = a.k, S = a.weight_shift, max_cost = a.max_cost;
    const int Tn = a.signal_lengths[b], Lb = a.label_lengths[b];
    const long long n64 = (long long)Lb - (k - 1) - 2 * a.first;
    const bool bad_len = Tn < 0 || Tn > a.max_signal || Lb < 0 || Lb > a.max_labels || n64 > a.max_events;
    const bool none = !bad_len && (n64 < 1 || Tn < n64);
    int* st_out = a.starts + (long long)b * (a.max_events + 1);
    int* ss_out = a.sample_state ? a.sample_state + (long long)b * a.max_signal : nullptr;
    if (bad_len || none) {                                           // workgroup-uniform: nothing else of the read is looked at
        for (int j = tid; j <= a.max_events; j += nthr) st_out[j] = -1;
        if (ss_out)
            for (int t = tid; t < a.max_signal; t += nthr) ss_out[t] = -1;
        if (tid == 0) {
            a.score[b] = bad_len ? kSaBadRead : kSaNoAlignment;
            a.band_hits[b] = bad_len ? -1 : 0;
            if (bad_len && a.bad) atomicAdd(a.bad, 1);
        }
        return;
    }
    const int N = (int)n64, Tb = Tn;                                 // 1 <= N <= Tb

    for (int i = tid; i < (3 << (2 * k)); i += nthr) s_model[i] = a.model[i];
    if (tid == 0) { s_bad = 0; s_hits = 0; s_fin = kSaInf; }
    __syncthreads();

    // this thread's slots 8 tid .. 8 tid + 7 start as the states of the same numbers
    const int* lab = a.labels + (long long)b * a.labels_stride + a.first;        // state j is the window lab[j .. j + k)
    int lvl[kSaPer], wgt[kSaPer], off[kSaPer];
    long long d[kSaPer];
    unsigned alive = 0;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < kSaPer; ++i) {
        const int j = kSaPer * tid + i;
        lvl[i] = 0; wgt[i] = 1; off[i] = 0;
        d[i] = kSaInf;
        if (tid < nact && j < N) {                                   // j + k <= N + k - 1 = Lb - 2 first: inside the labels
            const int code = kmer_code(lab + j, k, &ok);
            sa_model_row(s_model, code, &lvl[i], &wgt[i], &off[i], &ok);
            alive |= 1u << i;
        }
    }

    const T* sig = (const T*)a.signal + (long long)b * a.signal_stride;
    const bool scaled = a.scale_shift != nullptr;
    const double scale = scaled ? (double)a.scale_shift[2 * b] : 1.0, shift = scaled ? (double)a.scale_shift[2 * b + 1] : 0.0;
    unsigned char* bprow = a.bp + (long long)b * a.max_signal * nact;
    const long long two_n = 2ll * N, two_t = 2ll * Tb;
    const int top = N > W ? N - W : 0;
    long long rem = N;                                               // (2 t + 1) N = c 2 T + rem
    int c = 0, lo = 0, lo_slot = 0;                                  // lo_slot = lo mod W
    for (int t = 0; t < Tb; ++t) {
        const int ks = t & (kSaSamples - 1);
        if (ks == 0) {                                               // the barrier of step t - 1: the old chunk is no longer read
            for (int i = tid; i < kSaSamples && t + i < Tb; i += nthr) {
                int q = 0;
                if (!quantise(sig[t + i], scaled, scale, shift, a.two_f, &q)) { ok = false; q = 0; }
                s_q[i] = q;
            }
            __syncthreads();
        }
        bool rose = false;
        int rearm = -1;
        if (t > 0) {                                                 // workgroup-uniform
            rem += two_n;
            if (rem >= two_t) { rem -= two_t; ++c; }                 // N <= Tb: c rises by at most one
            int ln = c - W / 2;
            ln = ln < 0 ? 0 : ln;
            ln = ln > top ? top : ln;
            if (ln > lo) {
                rose = true;
                rearm = lo_slot;
                lo = ln;
                lo_slot = lo_slot + 1 == W ? 0 : lo_slot + 1;
                const int r = lo - 1;                                // state r + W <= N - 1 enters the band in slot `rearm`
                if ((r & (kSaCodes - 1)) == 0) {
                    for (int i = tid; i < kSaCodes; i += nthr) {
                        const long long j = (long long)W + r + i;
                        int code = 0;
                        if (j < N) code = kmer_code(lab + j, k, &ok);
                        s_code[i] = code;
                    }
                    __syncthreads();
                }
                if ((rearm >> 3) == tid) {
                    int l, w, o;
                    sa_model_row(s_model, s_code[r & (kSaCodes - 1)], &l, &w, &o, &ok);
#pragma unroll
                    for (int i = 0; i < kSaPer; ++i)
                        if (i == (rearm & 7)) { lvl[i] = l; wgt[i] = w; off[i] = o; }
                }
            }
        }
        const int q = s_q[ks];
        long long prev = kSaInf;                                     // cost_{t-1} of the slot to the left
        if (t > 0) prev = s_edge[(t - 1) & 1][tid == 0 ? nact - 1 : tid - 1];
        unsigned bits = 0;
#pragma unroll
        for (int i = 0; i < kSaPer; ++i) {
            const int sl = kSaPer * tid + i;
            long long m = d[i];
            long long step = prev;
            prev = d[i];
            if (rose && sl == rearm) m = kSaInf;                     // the state that enters was outside the band at t - 1
            if (!rose && sl == lo_slot) step = kSaInf;               // and so was the state below lo
            unsigned bp = 0;
            if (step < m) { m = step; bp = 1; }
            if (t == 0) { m = sl == 0 ? 0 : kSaInf; bp = 0; }        // paths start in state 0
            long long n = kSaInf;
            if (((alive >> i) & 1u) && m < kSaInf) n = m + sa_sample_cost(q, lvl[i], wgt[i], off[i], S, max_cost);
            d[i] = n;
            bits |= bp << i;
        }
        s_edge[t & 1][tid] = d[kSaPer - 1];
        if (tid < nact) bprow[(long long)t * nact + tid] = (unsigned char)bits;
        __syncthreads();                                             // one barrier per step: the row of step t - 1 is free again
    }
    {
        const int fs = (N - 1) % W;                                  // the slot of the last state
        if ((fs >> 3) == tid) {
#pragma unroll
            for (int i = 0; i < kSaPer; ++i)
                if (i == (fs & 7)) s_fin = d[i];
        }
    }
    if (!ok) atomicOr(&s_bad, 1);
    __syncthreads();                                                 // s_fin, s_bad and this workgroup's backpointer rows are visible

    const long long fin = s_fin;
    const bool poisoned = s_bad != 0;
    if (poisoned || fin >= kSaInf) {
        for (int j = tid; j <= a.max_events; j += nthr) st_out[j] = -1;
        if (ss_out)
            for (int t = tid; t < a.max_signal; t += nthr) ss_out[t] = -1;
        if (tid == 0) {
            a.score[b] = poisoned ? kSaBadRead : kSaNoAlignment;
            a.band_hits[b] = poisoned ? -1 : 0;
            if (poisoned && a.bad) atomicAdd(a.bad, 1);
        }
        return;
    }
    for (int j = N + tid; j <= a.max_events; j += nthr) st_out[j] = Tb;
    if (ss_out)
        for (int t = Tb + tid; t < a.max_signal; t += nthr) ss_out[t] = -1;

    int s_end = N - 1, hits = 0;
    for (int t0 = (Tb - 1) / kSaTrace * kSaTrace; t0 >= 0; t0 -= kSaTrace) {
        const int nf = min(kSaTrace, Tb - t0);
        const int g0 = max(s_end - (kSaTrace - 1), 0) >> 3;          // first byte of the window (s_end - 64, s_end]
        for (int i = tid; i < nf * kSaWinBytes; i += nthr) {
            const int f = i / kSaWinBytes, g = g0 + (i - f * kSaWinBytes);
            s_win[i] = bprow[(long long)(t0 + f) * nact + g % nact];
        }
        __syncthreads();                                             // window loaded; s_path of the previous chunk was read
        if (tid == 0) {
            int s = s_end;
            for (int f = nf - 1; f >= 0; --f) {
                s_path[f + 1] = s;
                const unsigned w = s_win[f * kSaWinBytes + ((s >> 3) - g0)];
                if (s > 0) s -= (int)((w >> (s & 7)) & 1u);          // row 0 holds zeros: the state of sample 0 stays
            }
            s_path[0] = t0 > 0 ? s : -1;
        }
        __syncthreads();
        for (int f = tid; f < nf; f += nthr) {
            const int before = s_path[f], pi = s_path[f + 1], t = t0 + f;
            if (ss_out) ss_out[t] = pi;
            if (before != pi) st_out[pi] = t;
            const int lt = sa_band_lo(t, N, Tb, W);
            if ((pi == lt && lt > 0) || (pi == lt + W - 1 && lt + W < N)) ++hits;
        }
        s_end = s_path[0];
    }
    if (hits) atomicAdd(&s_hits, hits);
    __syncthreads();
    if (tid == 0) {
        a.score[b] = fin;
        a.band_hits[b] = s_hits;
    }
}

static bool sa_sizes_ok(int batch, int max_signal, int band) {
    return batch >= 1 && batch <= 65535 && max_signal >= 1 && max_signal <= kSaMaxSignal && band >= kSaMinBand && band <= kSaMaxBand &&
           band % 64 == 0;
}

}  // namespace wn
using namespace wn;

// workspace: backpointers, 1 bit per (sample, band slot), [B][max_signal][band / 8] bytes
size_t wn_signal_align_workspace_bytes(int batch, int max_signal, int band) {
    if (!sa_sizes_ok(batch, max_signal, band)) return 0;
    return ((size_t)batch * (size_t)max_signal * (size_t)(band / 8) + 15) / 16 * 16;
}

int wn_signal_align(const void* signal, int signal_kind, long long signal_stride, const int* signal_lengths, const float* scale_shift,
                    const int* labels, long long labels_stride, const int* label_lengths, const int* model, int batch, int max_signal,
                    int max_labels, int max_events, int k, int first, int frac_bits, int weight_shift, int max_cost, int band,
                    int* starts, long long* score, int* band_hits, int* sample_state, void* workspace, size_t workspace_bytes,
                    int* bad, wn_stream_t stream) {
    if (batch < 1 || max_signal < 1 || max_labels < 1 || max_events < 1) return WN_ERR_BAD_SHAPE;
    if (signal_stride < 0 || labels_stride < 0 || signal_kind < 0 || signal_kind > 1) return WN_ERR_BAD_SHAPE;
    if (k < 1 || k > kSigMaxK || first < 0 || first > kSigMaxFirst || frac_bits < 0 || frac_bits > kSigMaxFrac) return WN_ERR_UNSUPPORTED;
    if (weight_shift < 16 || weight_shift > 63 || max_cost < 1) return WN_ERR_UNSUPPORTED;
    if (band < kSaMinBand || band > kSaMaxBand || band % 64 != 0) return WN_ERR_UNSUPPORTED;
    if (batch > 65535 || max_signal > kSaMaxSignal || max_events > kSaMaxEvents) return WN_ERR_UNSUPPORTED;
    if (!signal || !signal_lengths || !labels || !label_lengths || !model || !starts || !score || !band_hits || !workspace)
        return WN_ERR_NULL;
    if (workspace_bytes < wn_signal_align_workspace_bytes(batch, max_signal, band) || ((size_t)workspace & 15)) return WN_ERR_WORKSPACE;
    if (!signal_aligned(signal, signal_kind)) return WN_ERR_WORKSPACE;

    SigAlignArgs a = {};
    a.signal = signal; a.signal_lengths = signal_lengths; a.scale_shift = scale_shift; a.labels = labels;
    a.label_lengths = label_lengths; a.model = model; a.signal_stride = signal_stride; a.labels_stride = labels_stride;
    a.B = batch; a.max_signal = max_signal; a.max_labels = max_labels; a.max_events = max_events; a.k = k; a.first = first;
    a.weight_shift = weight_shift; a.max_cost = max_cost; a.band = band;
    a.two_f = (double)(1 << frac_bits);
    a.starts = starts; a.score = score; a.band_hits = band_hits; a.sample_state = sample_state;
    a.bp = (unsigned char*)workspace; a.bad = bad;

    hipStream_t st = (hipStream_t)stream;
    const int threads = (band / kSaPer + 63) / 64 * 64;              // one wave up to band 512, four at 2048
    const size_t lds = (size_t)(3 << (2 * k)) * sizeof(int);
    if (signal_kind)
        hipLaunchKernelGGL(signal_align_kernel<short>, dim3((unsigned)batch), dim3(threads), lds, st, a);
    else
        hipLaunchKernelGGL(signal_align_kernel<float>, dim3((unsigned)batch), dim3(threads), lds, st, a);
    WN_HIP(hipGetLastError(), "signal_align");
    return WN_OK;
}
