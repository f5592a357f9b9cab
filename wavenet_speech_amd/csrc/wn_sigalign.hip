// Signal-to-base alignment under the k-mer pore model: raw samples against the k-mers of KNOWN bases, the
// minimum-cost monotone path (every sample stays in its k-mer or steps to the next one, no skips) inside a band around the
// diagonal.  What nanopolish `eventalign` does before the reference's utils/dump_distributions.py reads its output, and the
// segmentation that wn_kmer_events (wn_events.hip, section 7j) takes.  Everything after the quantisation of a sample is integer.
//
//   signal_align_kernel<T>   one workgroup per read on the banded-path core of wn_band_dev.h (slots, band entry, closing, trace
//                            windows), two phases in one launch.  What is this kernel's own:
//
//     forward   cost_t(j) = min(cost_{t-1}(j), cost_{t-1}(j-1)) + sample_cost(q_t, model[kmer_j]) over the states of the band
//               [lo(t), lo(t) + W).  N <= T, so lo rises by at most one per sample: the state that enters takes the slot of the
//               one that left and its stay predecessor is +inf for this one step.  One value crosses threads per step: the last
//               slot of the left neighbour, cyclic over the band, through a double-buffered LDS row and ONE workgroup barrier per
//               step (with band <= 512 the workgroup is one wave).  The state at lo(t) has no step predecessor unless lo has just
//               risen (lo(t) - 1 was outside the band at t - 1).  The eight 1-bit backpointers of a thread are one byte store to
//               the workspace, bp[b][t][W / 8].  Samples are quantised 1024 at a time into LDS and validated there.
//     trace     the path moves at most one state per sample, so a chunk's window is 9 bytes per sample; one lane walks the 64
//               steps in LDS, then the threads write sample_state, the starts of the states that begin in the chunk and count
//               the samples on the band's edge.
//
// Ties (tests/signal_align_ref.py holds the same rule): the stay predecessor is taken first, the step predecessor replaces it
// only if strictly smaller.  No value of a length, a label or a sample is used as an index before it is checked; a read found
// bad anywhere in the forward phase gets its outputs from the fill at the end, never from the trace.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"
#include "wn_band_dev.h"

namespace wn {

constexpr int kSaSamples = 1024;              // samples quantised into LDS at a time
constexpr int kSaWinBytes = kBandWinBytes<1, 1>;                     // 1-bit backpointers, one state per sample at the most: 9
constexpr int kSaMaxSignal = 1 << 24;
constexpr int kSaMaxEvents = 1 << 20;         // a path's cost stays below 2^24 (2^31 + 2^30) < 2^56 < kPathInf

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

template <typename T>
__global__ __launch_bounds__(kBandMaxThreads) void signal_align_kernel(const SigAlignArgs a) {
    extern __shared__ __attribute__((aligned(16))) char sa_smem[];
    int* s_model = reinterpret_cast<int*>(sa_smem);                  // [4^k][3]
    __shared__ int s_q[kSaSamples];
    __shared__ int s_code[kBandCodes];
    __shared__ long long s_edge[2][kBandMaxThreads];                 // every thread's last slot, by step parity
    __shared__ unsigned char s_win[kBandTrace * kSaWinBytes];
    __shared__ int s_path[kBandTrace + 1];                           // [0] the state before the chunk, [1 + f]
    __shared__ long long s_fin;
    __shared__ int s_bad, s_hits;
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int W = a.band, nact = W / kBandPer, k = a.k, S = a.weight_shift, max_cost = a.max_cost;
    const int Tn = a.signal_lengths[b], Lb = a.label_lengths[b];
    const long long n64 = (long long)Lb - (k - 1) - 2 * a.first;
    const bool bad_len = Tn < 0 || Tn > a.max_signal || Lb < 0 || Lb > a.max_labels || n64 > a.max_events;
    const bool none = !bad_len && (n64 < 1 || Tn < n64);
    int* st_out = a.starts + (long long)b * (a.max_events + 1);
    int* ss_out = a.sample_state ? a.sample_state + (long long)b * a.max_signal : nullptr;
    if (bad_len || none) {                                           // workgroup-uniform: nothing else of the read is looked at
        band_refuse(bad_len, st_out, a.max_events + 1, ss_out, a.max_signal, a.score + b, a.band_hits + b, a.bad, tid, nthr);
        return;
    }
    const int N = (int)n64, Tb = Tn;                                 // 1 <= N <= Tb

    for (int i = tid; i < (3 << (2 * k)); i += nthr) s_model[i] = a.model[i];
    if (tid == 0) { s_bad = 0; s_hits = 0; s_fin = kPathInf; }
    __syncthreads();

    const int* lab = a.labels + (long long)b * a.labels_stride + a.first;        // state j is the window lab[j .. j + k)
    int lvl[kBandPer], wgt[kBandPer], off[kBandPer];
    long long d[kBandPer];
    unsigned alive;
    bool ok = true;
    band_arm(s_model, lab, k, N, W, tid, lvl, wgt, off, d, alive, ok);           // N + k - 1 = Lb - 2 first: inside the labels

    const T* sig = (const T*)a.signal + (long long)b * a.signal_stride;
    const auto [scaled, scale, shift] = read_scale(a.scale_shift, b);
    unsigned char* bprow = a.bp + (long long)b * a.max_signal * nact;
    BandCursor cur(N, Tb, W);
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
            const int r = cur.lo;
            rearm = cur.lo_slot;
            rose = cur.advance() > 0;                                // N <= Tb: lo rises by at most one
            if (rose) band_enter(r, rearm, s_model, s_code, lab, k, N, W, tid, nthr, lvl, wgt, off, ok);
        }
        const int lo_slot = cur.lo_slot;
        const int q = s_q[ks];
        long long prev = kPathInf;                                   // cost_{t-1} of the slot to the left
        if (t > 0) prev = s_edge[(t - 1) & 1][tid == 0 ? nact - 1 : tid - 1];
        unsigned bits = 0;
#pragma unroll
        for (int i = 0; i < kBandPer; ++i) {
            const int sl = kBandPer * tid + i;
            long long m = d[i];
            long long step = prev;
            prev = d[i];
            if (rose && sl == rearm) m = kPathInf;                   // the state that enters was outside the band at t - 1
            if (!rose && sl == lo_slot) step = kPathInf;             // and so was the state below lo
            unsigned bp = 0;
            if (step < m) { m = step; bp = 1; }
            if (t == 0) { m = sl == 0 ? 0 : kPathInf; bp = 0; }      // paths start in state 0
            long long n = kPathInf;
            if (((alive >> i) & 1u) && m < kPathInf) n = m + sa_sample_cost(q, lvl[i], wgt[i], off[i], S, max_cost);
            d[i] = n;
            bits |= bp << i;
        }
        s_edge[t & 1][tid] = d[kBandPer - 1];
        if (tid < nact) bprow[(long long)t * nact + tid] = (unsigned char)bits;
        __syncthreads();                                             // one barrier per step: the row of step t - 1 is free again
    }
    band_close(d, ok, N, W, tid, &s_fin, &s_bad);

    const long long fin = s_fin;
    const bool poisoned = s_bad != 0;
    if (poisoned || fin >= kPathInf) {
        band_refuse(poisoned, st_out, a.max_events + 1, ss_out, a.max_signal, a.score + b, a.band_hits + b, a.bad, tid, nthr);
        return;
    }
    for (int j = N + tid; j <= a.max_events; j += nthr) st_out[j] = Tb;
    if (ss_out)
        for (int t = Tb + tid; t < a.max_signal; t += nthr) ss_out[t] = -1;

    int s_end = N - 1, hits = 0;
    for (int t0 = (Tb - 1) / kBandTrace * kBandTrace; t0 >= 0; t0 -= kBandTrace) {
        const int nf = min(kBandTrace, Tb - t0);
        const int g0 = band_load_window<1, 1>(s_win, bprow, t0, nf, s_end, W, tid, nthr);       // (s_end - 64, s_end]
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
            if (band_on_edge(pi, band_lo(t, N, Tb, W), N, W)) ++hits;
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

}  // namespace wn
using namespace wn;

// workspace: backpointers, 1 bit per (sample, band slot), [B][max_signal][band / 8] bytes
size_t wn_signal_align_workspace_bytes(int batch, int max_signal, int band) {
    return band_sizes_ok(batch, max_signal, kSaMaxSignal, band) ? band_workspace_bytes(batch, max_signal, band, 1) : 0;
}

int wn_signal_align(const void* signal, int signal_kind, long long signal_stride, const int* signal_lengths, const float* scale_shift,
                    const int* labels, long long labels_stride, const int* label_lengths, const int* model, int batch, int max_signal,
                    int max_labels, int max_events, int k, int first, int frac_bits, int weight_shift, int max_cost, int band,
                    int* starts, long long* score, int* band_hits, int* sample_state, void* workspace, size_t workspace_bytes,
                    int* bad, wn_stream_t stream) {
    if (batch < 1 || max_signal < 1 || max_labels < 1 || max_events < 1) return WN_ERR_BAD_SHAPE;
    if (signal_stride < 0 || labels_stride < 0 || signal_kind < 0 || signal_kind > 1) return WN_ERR_BAD_SHAPE;
    if (const int e = band_check_params(k, first, frac_bits, weight_shift, max_cost, band)) return e;
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
    const size_t lds = (size_t)(3 << (2 * k)) * sizeof(int);
    if (signal_kind)
        hipLaunchKernelGGL(signal_align_kernel<short>, dim3((unsigned)batch), dim3(band_threads(band)), lds, st, a);
    else
        hipLaunchKernelGGL(signal_align_kernel<float>, dim3((unsigned)batch), dim3(band_threads(band)), lds, st, a);
    WN_HIP(hipGetLastError(), "signal_align");
    return WN_OK;
}
