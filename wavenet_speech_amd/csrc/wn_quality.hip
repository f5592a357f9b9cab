// Per-base quality of a decoded read: for every label a decoder emitted, the mean (or the least) frame
// error over the label's run of frames, its Phred quality and its dwell; per read the mean error of its bases.  The input is
// read in place through (batch, class, time) element strides, as the decoders read it; labels / frames are int32 rows with a
// row stride, so the best beam of wn_ctc_beam_decode goes in as it lies.
//
//   base_quality_kernel   grid (ceil(max_labels / 256), batch), 256 threads, ONE THREAD PER BASE j.  It walks from frame f_j
//                         while the run lasts: the run is {f_j} and then every following frame below the next base's frame
//                         (the utterance's end for the last base) whose argmax (ties to the lowest class, strict >, the greedy
//                         decoder's rule) is the base's label.  Per frame two passes over the C classes: max and argmax, then
//                         w_c = expf(x_c - max) (w_c = x_c for probabilities), sum of all w and sum of the w of the other
//                         classes, both in fp32 in class order, one division: never 1 - p.  The second pass re-reads the
//                         frame (it hits the L1 the first pass filled) rather than keep up to 64 values in an indexed array,
//                         which would live in scratch.  The frame errors of a run are summed in frame order in float64 (or
//                         their minimum is taken).  Neighbouring bases sit a few frames apart, so the loads of a wave along t
//                         stay close to coalesced in the [B][C][T] layout.  Work per base is its own run, never T; a single
//                         run of thousands of frames is walked by one thread.
//   read_error_kernel     one workgroup per read, 256 threads: thread i sums e_j for j = i, i + 256, ... in that order in
//                         float64, then a fixed LDS tree (128, 64, ... 1): bitwise the same from run to run.  It reads the
//                         errors the first launch stored, or -- when the caller asked for no per-base errors -- evaluates the
//                         same device function itself.
//
// No value of a label, frame or length is used as an index before it is checked.  No atomics on floating point, no workspace,
// no scratch, plain vector stores; expf and log10 are the device library's.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"
#include <float.h>

namespace wn {

constexpr int kQThreads = 256;
constexpr int kQMaxClasses = 64;
constexpr int kQMaxLength = 1 << 24;
constexpr long long kQMaxGridThreads = 4294967296ll;     // threads of one launch stay below 2^32

struct QualityArgs {
    const float* x;                     // element (b, c, t) at x[b * sb + c * sc + t * st]
    long long sb, sc, st;
    const long long* input_len;         // [B] or nullptr (= T)
    const int* labels;                  // row b at labels + b * labels_stride
    const int* frames;
    long long labels_stride, frames_stride;
    const int* lengths;                 // [B]
    float* error;                       // [B][Lmax] or nullptr
    unsigned char* qual;                // [B][Lmax] or nullptr
    int* dwell;                         // [B][Lmax] or nullptr
    float* read_error;                  // [B] or nullptr
    int* bad;
    int B, C, T, Lmax, blank, kind, stat;
    float qscale, qbias;
};

// the read's frame count and label count, or false when either is out of range (then neither is used)
__device__ __forceinline__ bool read_extent(const QualityArgs& a, int b, int* Tb, int* len) {
    const long long tb = a.input_len ? a.input_len[b] : (long long)a.T;
    const int n = a.lengths[b];
    if (tb < 0 || tb > a.T || n < 0 || n > a.Lmax) return false;
    *Tb = (int)tb;
    *len = n;
    return true;
}

// argmax of frame p (ties to the lowest class) and its maximum
__device__ __forceinline__ int frame_argmax(const float* p, long long sc, int C, float* mx) {
    float m = p[0];
    int best = 0;
    for (int c = 1; c < C; ++c) {
        const float v = p[(long long)c * sc];
        if (v > m) { m = v; best = c; }
    }
    *mx = m;
    return best;
}

// eps_t(l): the weight of every class but l over the weight of all classes
__device__ __forceinline__ float frame_error(const float* p, long long sc, int C, int l, float m, bool exponent) {
    float all = 0.0f, others = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float v = p[(long long)c * sc];
        const float w = exponent ? expf(v - m) : v;
        all += w;
        others += c != l ? w : 0.0f;
    }
    return others / all;
}

// base j of read b (j < len, the read's extent in range): its error e_j as the fp32 value that is published, NaN for a bad
// base; *n_frames = its dwell (0 for a bad base)
__device__ float base_error(const QualityArgs& a, int b, int j, int len, int Tb, int* n_frames) {
    *n_frames = 0;
    const int* lab = a.labels + (long long)b * a.labels_stride;
    const int* frm = a.frames + (long long)b * a.frames_stride;
    const int l = lab[j], f = frm[j];
    if (l < 0 || l >= a.C || l == a.blank || f < 0 || f >= Tb) return __builtin_nanf("");
    if (j > 0 && f <= frm[j - 1]) return __builtin_nanf("");
    int lim = Tb;
    if (j + 1 < len) {
        const int next = frm[j + 1];                                 // a bad successor bounds nothing beyond the utterance
        lim = next < Tb ? next : Tb;
    }
    const bool exponent = a.kind != 1;
    const float* p = a.x + (long long)b * a.sb + (long long)f * a.st;
    float m = 0.0f;
    if (exponent) frame_argmax(p, a.sc, a.C, &m);
    float eps = frame_error(p, a.sc, a.C, l, m, exponent);
    double sum = (double)eps;
    float least = eps;
    int n = 1;
    for (int t = f + 1; t < lim; ++t) {
        p += a.st;
        if (frame_argmax(p, a.sc, a.C, &m) != l) break;
        eps = frame_error(p, a.sc, a.C, l, m, exponent);
        sum += (double)eps;
        least = eps < least ? eps : least;
        ++n;
    }
    *n_frames = n;
    return a.stat == 0 ? (float)(sum / (double)n) : least;
}

// Q = qscale (-10 log10 e) + qbias in float64, rounded half up, clamped to [0, 93]; NaN -> 0
__device__ __forceinline__ unsigned char phred(float e, float qscale, float qbias) {
    const double q = (double)qscale * (-10.0 * log10((double)e)) + (double)qbias;
    const double r = floor(q + 0.5);
    if (!(r > 0.0)) return 0;                                        // NaN, -inf and everything that rounds to 0 or below
    return (unsigned char)(r < 93.0 ? (int)r : 93);
}

__global__ __launch_bounds__(kQThreads) void base_quality_kernel(const QualityArgs a) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * kQThreads + threadIdx.x;
    if (j >= a.Lmax) return;
    int Tb = 0, len = 0;
    const bool read_ok = read_extent(a, b, &Tb, &len);
    if (!read_ok && j == 0 && a.bad) atomicAdd(a.bad, 1);            // a read out of range counts once
    float e = __builtin_nanf("");
    int n = 0;
    if (read_ok && j < len) {
        e = base_error(a, b, j, len, Tb, &n);
        if (n == 0 && a.bad) atomicAdd(a.bad, 1);                    // a bad base counts once
    }
    const long long o = (long long)b * a.Lmax + j;
    if (a.error) a.error[o] = e;
    if (a.qual) a.qual[o] = n > 0 ? phred(e, a.qscale, a.qbias) : (unsigned char)0;
    if (a.dwell) a.dwell[o] = n;
}

template <bool kStored>
__global__ __launch_bounds__(kQThreads) void read_error_kernel(const QualityArgs a) {
    __shared__ double part[kQThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    int Tb = 0, len = 0;
    const bool read_ok = read_extent(a, b, &Tb, &len);
    double sum = 0.0;
    if (read_ok) {
        for (int j = tid; j < len; j += kQThreads) {
            int n;
            sum += (double)(kStored ? a.error[(long long)b * a.Lmax + j] : base_error(a, b, j, len, Tb, &n));
        }
    }
    part[tid] = sum;
    __syncthreads();
    for (int s = kQThreads / 2; s > 0; s >>= 1) {
        if (tid < s) part[tid] += part[tid + s];
        __syncthreads();
    }
    if (tid == 0) a.read_error[b] = read_ok && len > 0 ? (float)(part[0] / (double)len) : __builtin_nanf("");
}

}  // namespace wn
using namespace wn;

int wn_ctc_base_quality(const float* x, long long sb, long long sc, long long st, int input_kind, const long long* input_lengths,
                        const int* labels, long long labels_stride, const int* frames, long long frames_stride, const int* lengths,
                        int batch, int classes, int length, int max_labels, int blank, int stat, float qscale, float qbias,
                        float* error, unsigned char* qual, int* dwell, float* read_error, int* bad, wn_stream_t stream) {
    if (batch < 1 || length < 1 || max_labels < 1 || classes < 2 || labels_stride < 0 || frames_stride < 0) return WN_ERR_BAD_SHAPE;
    if (input_kind < 0 || input_kind > 2 || stat < 0 || stat > 1) return WN_ERR_BAD_SHAPE;
    if (!(qscale > 0.0f && qscale <= FLT_MAX) || !(qbias >= -FLT_MAX && qbias <= FLT_MAX)) return WN_ERR_BAD_SHAPE;   // NaN fails both
    if (classes > kQMaxClasses || length > kQMaxLength || max_labels > length || batch > 65535) return WN_ERR_UNSUPPORTED;
    const long long tiles = ((long long)max_labels + kQThreads - 1) / kQThreads;
    if (tiles * kQThreads * batch >= kQMaxGridThreads) return WN_ERR_UNSUPPORTED;
    if (!x || !labels || !frames || !lengths || (!error && !qual && !dwell && !read_error)) return WN_ERR_NULL;
    QualityArgs a = {};
    a.x = x; a.sb = sb; a.sc = sc; a.st = st; a.input_len = input_lengths;
    a.labels = labels; a.frames = frames; a.labels_stride = labels_stride; a.frames_stride = frames_stride; a.lengths = lengths;
    a.error = error; a.qual = qual; a.dwell = dwell; a.read_error = read_error; a.bad = bad;
    a.B = batch; a.C = classes; a.T = length; a.Lmax = max_labels; a.blank = blank; a.kind = input_kind; a.stat = stat;
    a.qscale = qscale; a.qbias = qbias;
    hipStream_t s = (hipStream_t)stream;
    if (error || qual || dwell || bad) {                             // the per-base launch also owns the bad count
        hipLaunchKernelGGL(base_quality_kernel, dim3((unsigned)tiles, (unsigned)batch), dim3(kQThreads), 0, s, a);
        WN_HIP(hipGetLastError(), "base_quality");
    }
    if (read_error) {
        if (error)
            hipLaunchKernelGGL(read_error_kernel<true>, dim3(batch), dim3(kQThreads), 0, s, a);
        else
            hipLaunchKernelGGL(read_error_kernel<false>, dim3(batch), dim3(kQThreads), 0, s, a);
        WN_HIP(hipGetLastError(), "read_error");
    }
    return WN_OK;
}
