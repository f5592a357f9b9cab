// Ragged synthetic reads on the device: what the reference's RawCTCNet workloads train on.  RawGaussianModelLoader
// (utils/gaussian_kmer_model.py, random_upsample=True) and RawSignalGenerator (utils/raw_signal_generator.py) draw reads of
// random length, hold every 5-mer for a random number of samples (its dwell), emit raw float picoamps zero-padded to the
// longest read of the batch, and hand the bases to CTC as targets.  wn_synth.hip restates the rectangular, fixed-dwell,
// quantised corner of the same generators; this file is the ragged one.  Two launches:
//
//   reads_plan_kernel     one workgroup per read.  Read length (Philox stream 2) -> bases 1..4, 0 past the length (stream 0) ->
//                         5-mer index of every k-mer -> dwell of every k-mer (stream 3: fixed, uniform integer, or
//                         max(1, (int)(Gamma * sample_rate))) -> starts = exclusive prefix sum of the dwell (a workgroup scan
//                         in chunks of 256: wave prefix by shuffles, wave totals through LDS, a running carry) -> signal length.
//                         Every drawn quantity can be given by the caller instead (the deterministic rest is then checked
//                         against fixtures of the reference).  The k-mer indices go to the workspace for the second launch.
//   reads_signal_kernel   grid (ceil(ld / 256), B), a tile of 256 samples per workgroup.  signal[b][t] = (float)(mean[k] +
//                         stdv[k] * z) in float64, k the 5-mer of the k-mer p with starts[p] <= t < starts[p + 1].  Every dwell
//                         is >= 1, so a tile touches at most 257 k-mers: the tile's first k-mer is found by ONE binary search
//                         of the read's starts that is uniform across the workgroup, 257 starts and 257 k-mer indices from
//                         there are staged in LDS, and each thread finds its own k-mer by an 8-step search in LDS (no
//                         per-sample dependent global loads, no LDS atomics).  Past the read: 0.0f / -1, every element of a
//                         row is written.
//
// The Gamma sampler is Marsaglia-Tsang (2000) with Box-Muller normals, shape < 1 through Gamma(shape + 1) * U^(1 / shape).  Its
// rejection loop is bounded: kGammaAttempts attempts, attempt i on sub-counter i of the k-mer's Philox counter.  An attempt is
// rejected with probability < 0.0485 for every shape >= 1 (the paper's table: acceptance 0.9516 at shape 1, rising with the
// shape), so all 16 fail with probability < 0.0485^16 < 1e-21; the fallback is then the mean of Gamma(a, 1), a itself, with
// U = 1/2.  No loop in either kernel has a data-dependent bound other than the read's own (host-limited) size.
// The uniform integer in [lo, hi) is lo + mulhi(word, hi - lo): its bias is at most (hi - lo) / 2^32 per value.
// All results leave through ordinary vector stores from plain C++.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"
#include "wn_philox.h"
#include "wn_wave_dev.h"

namespace wn {

constexpr int kRdTile = 256;             // threads of both kernels; k-mers per scan chunk; samples per signal tile
constexpr int kRdWin = kRdTile + 1;      // k-mers a tile of samples can touch (every dwell >= 1)
constexpr int kGammaAttempts = 16;
constexpr int kRdMaxBases = 65536;
constexpr int kRdSearchSteps = 17;       // halvings that empty any range below 2^17 > kRdMaxBases

struct ReadsPlanArgs {
    unsigned long long seed;
    int B, min_bases, max_bases, window, model, max_dwell;
    double p0, p1, p2;                   // FIXED: r | UNIFORM: r, w | GAMMA: shape, rate, sample_rate
    const int* base_lengths_in;          // [B] or nullptr
    const int* bases_in;                 // [B][max_bases] or nullptr
    const int* dwell_in;                 // [B][max_bases] or nullptr
    int* base_lengths;                   // [B]
    int* bases;                          // [B][max_bases]
    int* dwell;                          // [B][max_bases]
    int* starts;                         // [B][max_bases]
    int* signal_lengths;                 // [B]
    unsigned short* kmers;               // [B][kmer_stride]: the workspace
    long long kmer_stride;
    int* bad;
    int* clamped;
};

// Gamma(shape, scale 1 / rate) * srate, truncated towards zero, at least 1; anything above `cap` comes back as cap + 1
__device__ __forceinline__ int gamma_dwell(unsigned long long seed, unsigned long long index, double shape, double rate,
                                           double srate, int cap) {
    const double a = shape < 1.0 ? shape + 1.0 : shape;
    const double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    double g = a;                                                        // the fallback: the mean of Gamma(a, 1)
    unsigned uw = 0x80000000u;                                           // and U = 1/2
    for (int att = 0; att < kGammaAttempts; ++att) {
        unsigned w[4];
        draw_sub(seed, 3u, index, (unsigned)att, w);
        const double u1 = ((double)w[0] + 0.5) * (1.0 / 4294967296.0), u2 = ((double)w[1] + 0.5) * (1.0 / 4294967296.0);
        const double x = sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
        double v = 1.0 + c * x;
        if (v <= 0.0) continue;
        v = v * v * v;
        const double ua = ((double)w[2] + 0.5) * (1.0 / 4294967296.0);
        if (log(ua) < 0.5 * x * x + d - d * v + d * log(v)) {
            g = d * v;
            uw = w[3];
            break;
        }
    }
    if (shape < 1.0) g *= pow(((double)uw + 0.5) * (1.0 / 4294967296.0), 1.0 / shape);
    const double n = g / rate * srate;
    if (!(n < (double)cap + 1.0)) return cap + 1;
    return max(1, (int)n);
}

__global__ __launch_bounds__(kRdTile) void reads_plan_kernel(const ReadsPlanArgs a) {
    __shared__ int wave_total[kRdTile / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int mb = a.max_bases, trim = 2 * a.window;
    const long long row = (long long)b * mb;

    // read length
    int n;
    bool poisoned = false;
    if (a.base_lengths_in) {
        n = a.base_lengths_in[b];
        poisoned = n < 5 + trim || n >= mb;
    } else {
        unsigned w[4];
        draw(a.seed, 2u, (unsigned long long)b, w);
        n = a.min_bases + (int)__umulhi(w[0], (unsigned)(mb - a.min_bases));
    }
    if (poisoned) n = 0;                                                 // never used as an index
    int K = n > 0 ? n - 4 - trim : 0;

    // given bases must be nucleotides, given dwell positive: checked before anything is written
    if (a.bases_in || a.dwell_in) {
        int wrong = 0;
        if (a.bases_in)
            for (int i = tid; i < n; i += kRdTile) { const int v = a.bases_in[row + i]; wrong |= v < 1 || v > 4; }
        if (a.dwell_in)
            for (int p = tid; p < K; p += kRdTile) wrong |= a.dwell_in[row + p] < 1;
        if (__syncthreads_or(wrong)) { poisoned = true; n = 0; K = 0; }
    }

    // bases, zero past the length (the reference's batchify)
    for (int i = tid; i < mb; i += kRdTile) {
        int v = 0;
        if (i < n) {
            if (a.bases_in) v = a.bases_in[row + i];
            else {
                unsigned w[4];
                draw(a.seed, 0u, ((unsigned long long)b << 32) | (unsigned)i, w);
                v = 1 + (int)(w[0] & 3u);
            }
        }
        a.bases[row + i] = v;
    }
    __syncthreads();                                                     // this workgroup's bases, through global memory

    // k-mers, dwell and its exclusive prefix sum, 256 k-mers per pass
    unsigned short* km = a.kmers + (long long)b * a.kmer_stride;
    int carry = 0, nclamped = 0;
    for (int p0 = 0; p0 < K; p0 += kRdTile) {
        const int p = p0 + tid;
        int d = 0;
        if (p < K) {
            const int* wb = a.bases + row + p + a.window;                // k-mer p = bases[p + window .. p + window + 4]
            int k = 0;
#pragma unroll
            for (int j = 0; j < 5; ++j) k = k * 4 + ((wb[j] - 1) & 3);
            km[p] = (unsigned short)k;
            const unsigned long long index = ((unsigned long long)b << 32) | (unsigned)p;
            if (a.dwell_in) d = a.dwell_in[row + p];
            else if (a.model == WN_DWELL_FIXED) d = (int)a.p0;
            else if (a.model == WN_DWELL_UNIFORM) {
                const int r = (int)a.p0, w = (int)a.p1, lo = max(r - w, 1);
                unsigned c[4];
                draw(a.seed, 3u, index, c);
                d = lo + (int)__umulhi(c[0], (unsigned)(r + w - lo));
            } else d = gamma_dwell(a.seed, index, a.p0, a.p1, a.p2, a.max_dwell);
            if (d > a.max_dwell) { d = a.max_dwell; ++nclamped; }
            a.dwell[row + p] = d;
        }
        int chunk, incl;
        block_scan<kRdTile / 64>(d, tid, wave_total, &chunk, OpAdd(), 0, &incl);
        if (p < K) a.starts[row + p] = carry + incl - d;                 // in this order the code is what it was before block_scan
        carry += chunk;
        __syncthreads();                                                 // wave_total is free again
    }
    // past the last k-mer: dwell 0, starts = the signal length
    for (int p = K + tid; p < mb; p += kRdTile) { a.dwell[row + p] = 0; a.starts[row + p] = carry; }
    if (tid == 0) {
        a.base_lengths[b] = n;
        a.signal_lengths[b] = carry;
        if (poisoned && a.bad) atomicAdd(a.bad, 1);
    }
    if (nclamped && a.clamped) atomicAdd(a.clamped, nclamped);
}

__global__ __launch_bounds__(kRdTile) void reads_signal_kernel(const int* __restrict__ base_lengths, const int* __restrict__ starts,
                                                               const int* __restrict__ signal_lengths,
                                                               const unsigned short* __restrict__ kmers, long long kmer_stride,
                                                               int max_bases, int window, int ld, const double* __restrict__ means,
                                                               const double* __restrict__ stdvs, unsigned long long seed,
                                                               const double* __restrict__ noise, float* __restrict__ signal,
                                                               int* __restrict__ sample_kmer, int* __restrict__ clipped_lengths,
                                                               int* __restrict__ bad) {
    __shared__ int sst[kRdWin];
    __shared__ unsigned short skm[kRdWin];
    const int b = blockIdx.y, tid = threadIdx.x, t0 = blockIdx.x * kRdTile, t = t0 + tid;
    const int n = base_lengths[b];
    const int K = min(max(n - 4 - 2 * window, 0), max_bases - 1);        // 0 for a poisoned read
    const int* st = starts + (long long)b * max_bases;
    const int len = K > 0 ? max(signal_lengths[b], 0) : 0;
    const int eff = min(len, ld);                                        // a read longer than the row is truncated
    if (blockIdx.x == 0 && tid == 0) {
        if (clipped_lengths) clipped_lengths[b] = eff;
        if (len > ld && bad) atomicAdd(bad, 1);
    }
    float* srow = signal + (long long)b * ld;
    int* krow = sample_kmer ? sample_kmer + (long long)b * ld : nullptr;
    if (t0 >= eff) {                                                     // a tile wholly past the read
        if (t < ld) { srow[t] = 0.0f; if (krow) krow[t] = -1; }
        return;
    }
    // the tile's first k-mer: the last p in [0, K) with starts[p] <= t0 (starts[0] = 0); the same search in every thread
    int lo = 0, hi = K - 1;
    for (int it = 0; it < kRdSearchSteps && lo < hi; ++it) {
        const int mid = (lo + hi + 1) >> 1;
        if (st[mid] <= t0) lo = mid; else hi = mid - 1;
    }
    const int pfirst = lo;
    const unsigned short* km = kmers + (long long)b * kmer_stride;
    for (int i = tid; i < kRdWin; i += kRdTile) {
        const int p = pfirst + i;
        sst[i] = p < K ? st[p] : len;                                    // starts[K] and everything after it: the length
        skm[i] = km[min(p, K - 1)];
    }
    __syncthreads();
    if (t >= ld) return;
    if (t >= eff) { srow[t] = 0.0f; if (krow) krow[t] = -1; return; }
    // the last j in [0, 256] with sst[j] <= t
    int j = 0;
    if (sst[kRdTile] <= t) j = kRdTile;
    else {
#pragma unroll
        for (int s = kRdTile / 2; s > 0; s >>= 1)
            if (sst[j + s] <= t) j += s;
    }
    const int k = skm[j] & 1023;
    double z;
    if (noise) z = noise[(long long)b * ld + t];
    else {
        unsigned c[4];
        draw(seed, 1u, ((unsigned long long)b << 32) | (unsigned)t, c);
        z = philox_normal(c);
    }
    srow[t] = (float)(means[k] + stdvs[k] * z);                          // float64, rounded once: the reference's .float()
    if (krow) krow[t] = pfirst + j;
}

}  // namespace wn

using namespace wn;

static int check_reads(int batch, int max_bases) {
    if (batch <= 0 || max_bases <= 0) return WN_ERR_BAD_SHAPE;
    if (batch > 65535 || max_bases > kRdMaxBases) return WN_ERR_UNSUPPORTED;
    return WN_OK;
}
static size_t reads_kmer_stride(int max_bases) { return ((size_t)max_bases + 7) / 8 * 8; }

// workspace: the 5-mer index of every k-mer, [B][round_up(max_bases, 8)] 16-bit
size_t wn_reads_workspace_bytes(int batch, int max_bases) {
    if (check_reads(batch, max_bases) != WN_OK) return 0;
    return (size_t)batch * reads_kmer_stride(max_bases) * sizeof(unsigned short);
}

int wn_reads_plan(unsigned long long seed, int batch, int min_bases, int max_bases, int window, int dwell_model, double dwell_p0,
                  double dwell_p1, double dwell_p2, int max_dwell, const int* base_lengths_in, const int* bases_in,
                  const int* dwell_in, int* base_lengths, int* bases, int* dwell, int* starts, int* signal_lengths, void* workspace,
                  size_t workspace_bytes, int* bad, int* clamped, wn_stream_t stream) {
    // shape
    if (batch <= 0 || max_bases <= 0 || max_dwell < 1) return WN_ERR_BAD_SHAPE;
    if (window != 0 && window != 2) return WN_ERR_BAD_SHAPE;
    if (min_bases < 5 + 2 * window || min_bases >= max_bases) return WN_ERR_BAD_SHAPE;
    switch (dwell_model) {
        case WN_DWELL_FIXED:
            if (!(dwell_p0 >= 1.0 && dwell_p0 < 2147483648.0)) return WN_ERR_BAD_SHAPE;
            break;
        case WN_DWELL_UNIFORM: {
            if (!(dwell_p0 >= 1.0 && dwell_p0 < 1073741824.0 && dwell_p1 >= 0.0 && dwell_p1 < 1073741824.0)) return WN_ERR_BAD_SHAPE;
            const long long r = (long long)dwell_p0, w = (long long)dwell_p1, lo = r - w > 1 ? r - w : 1;
            if (r + w <= lo) return WN_ERR_BAD_SHAPE;                    // an empty interval
            break;
        }
        case WN_DWELL_GAMMA:
            if (!(dwell_p0 > 0.0 && dwell_p1 > 0.0 && dwell_p2 > 0.0) || !(dwell_p0 < 1e300 && dwell_p1 < 1e300 && dwell_p2 < 1e300))
                return WN_ERR_BAD_SHAPE;
            break;
        default: return WN_ERR_BAD_SHAPE;
    }
    // limits
    const int rc = check_reads(batch, max_bases);
    if (rc != WN_OK) return rc;
    if ((long long)(max_bases - 5) * max_dwell >= 2147483648ll) return WN_ERR_UNSUPPORTED;    // a signal length is an int32
    if (!base_lengths || !bases || !dwell || !starts || !signal_lengths || !workspace) return WN_ERR_NULL;
    if (workspace_bytes < wn_reads_workspace_bytes(batch, max_bases)) return WN_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return WN_ERR_WORKSPACE;
    ReadsPlanArgs a = {};
    a.seed = seed; a.B = batch; a.min_bases = min_bases; a.max_bases = max_bases; a.window = window; a.model = dwell_model;
    a.max_dwell = max_dwell; a.p0 = dwell_p0; a.p1 = dwell_p1; a.p2 = dwell_p2;
    a.base_lengths_in = base_lengths_in; a.bases_in = bases_in; a.dwell_in = dwell_in;
    a.base_lengths = base_lengths; a.bases = bases; a.dwell = dwell; a.starts = starts; a.signal_lengths = signal_lengths;
    a.kmers = reinterpret_cast<unsigned short*>(workspace); a.kmer_stride = (long long)reads_kmer_stride(max_bases);
    a.bad = bad; a.clamped = clamped;
    hipLaunchKernelGGL(reads_plan_kernel, dim3(batch), dim3(kRdTile), 0, (hipStream_t)stream, a);
    WN_HIP(hipGetLastError(), "reads_plan");
    return WN_OK;
}

int wn_reads_signal(const int* base_lengths, const int* starts, const int* signal_lengths, const void* workspace,
                    size_t workspace_bytes, int batch, int max_bases, int window, int ld, const double* means, const double* stdvs,
                    unsigned long long seed, const double* noise, float* signal, int* sample_kmer, int* clipped_lengths, int* bad,
                    wn_stream_t stream) {
    if (batch <= 0 || max_bases <= 0 || ld <= 0) return WN_ERR_BAD_SHAPE;
    if (window != 0 && window != 2) return WN_ERR_BAD_SHAPE;
    const int rc = check_reads(batch, max_bases);
    if (rc != WN_OK) return rc;
    if (ld > 2147483647 - kRdTile) return WN_ERR_UNSUPPORTED;            // t0 + tid stays an int32
    if (!base_lengths || !starts || !signal_lengths || !workspace || !means || !stdvs || !signal) return WN_ERR_NULL;
    if (workspace_bytes < wn_reads_workspace_bytes(batch, max_bases)) return WN_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return WN_ERR_WORKSPACE;
    hipLaunchKernelGGL(reads_signal_kernel, dim3((unsigned)((ld + kRdTile - 1) / kRdTile), batch), dim3(kRdTile), 0, (hipStream_t)stream,
                       base_lengths, starts, signal_lengths, reinterpret_cast<const unsigned short*>(workspace),
                       (long long)reads_kmer_stride(max_bases), max_bases, window, ld, means, stdvs, seed, noise, signal, sample_kmer,
                       clipped_lengths, bad);
    WN_HIP(hipGetLastError(), "reads_signal");
    return WN_OK;
}
