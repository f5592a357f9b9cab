// Chunked whole-read inference (wavenet_speech_amd/basecalling.py): the two streaming kernels around the fixed-shape forward.
// A read of any length is cut into chunks of `chunk` samples that overlap by the network's receptive field; every chunk keeps
// only the output frames whose receptive field lay inside it, and the kept frames of a read tile its frames exactly.  The
// plan is made on the host: one row of five ints per chunk,
//
//   plan[n] = (read, s0, u_lo, t0, count)    chunk n holds samples [s0, s0 + chunk) of `read`; its frames [u_lo, u_lo + count)
//                                            are frames [t0, t0 + count) of the read.  count = 0: a dead chunk (padding of the
//                                            last micro-batch), its other fields are not looked at.
//
//   chunk_gather_kernel   grid (ceil(chunk / 1024), n_chunks), 256 threads, 4 consecutive samples per thread written with one
//                         16-byte store (rows are 16-byte aligned: chunk % 4 == 0, out aligned).  The source offset s0 is
//                         arbitrary, so the loads are per element (a wave still reads one contiguous span).  int16 DAC counts
//                         or fp32; x = (float(raw) + shift[read]) * scale[read] as two separately rounded fp32 operations (no
//                         FMA: bit-equal to the same expression in torch).  Samples at or past the read's length are 0.0f, not
//                         the affine image of 0.
//   chunk_stitch_kernel   grid (ceil(y_frames / 256), classes, n_chunks), 256 threads, one element per thread:
//                         out[read][c][t0 + i] = y[n][c][u_lo + i], i < count.  y is addressed through its strides.
//
// No value of a plan row or of a length is used as an index before it is checked: a row that would read or write outside its
// tensors is counted in *bad and gathers zeros / stitches nothing.  No LDS, no scratch, no loops with a data-dependent bound.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"

namespace wn {

constexpr int kChThreads = 256;
constexpr int kChPerThread = 4;
constexpr int kChPlanInts = 5;
constexpr long long kChMaxGridThreads = 4294967296ll;    // threads of one launch stay below 2^32
constexpr int kChMaxDim = 2147482624;            // 2^31 - 1024; ld, chunk, frames stay below it: index + tile is an int32

template <typename T>
__global__ __launch_bounds__(kChThreads) void chunk_gather_kernel(const T* __restrict__ signal, int batch, int ld,
                                                                  const int* __restrict__ signal_lengths,
                                                                  const float* __restrict__ scale, const float* __restrict__ shift,
                                                                  const int* __restrict__ plan, int chunk, float* __restrict__ out,
                                                                  int* __restrict__ bad) {
    const int n = blockIdx.y;
    const int i0 = (blockIdx.x * kChThreads + threadIdx.x) * kChPerThread;
    if (i0 >= chunk) return;                                             // chunk % 4 == 0: i0 + 3 < chunk below
    const int* row = plan + (long long)n * kChPlanInts;
    const int read = row[0], s0 = row[1], count = row[4];
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool live = count != 0;
    int len = 0;
    if (live) {
        bool wrong = read < 0 || read >= batch || s0 < 0 || s0 >= ld || count < 0;
        if (!wrong) {
            len = signal_lengths[read];
            wrong = len < 0 || len > ld;
        }
        if (wrong) {
            live = false;
            if (bad && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(bad, 1);
        }
    }
    if (live) {
        const T* src = signal + (long long)read * ld;
        const long long s = (long long)s0 + i0;                          // < 2^32: compared before it is narrowed
        const float sh = shift ? shift[read] : 0.0f, sc = scale ? scale[read] : 1.0f;
        float x[kChPerThread];
#pragma unroll
        for (int i = 0; i < kChPerThread; ++i) {
            float r = 0.0f;
            if (s + i < (long long)len) {
                r = (float)src[s + i];
                if (shift) r = __fadd_rn(r, sh);
                if (scale) r = __fmul_rn(r, sc);
            }
            x[i] = r;
        }
        v = make_float4(x[0], x[1], x[2], x[3]);
    }
    *reinterpret_cast<float4*>(out + (long long)n * chunk + i0) = v;
}

__global__ __launch_bounds__(kChThreads) void chunk_stitch_kernel(const float* __restrict__ y, long long stride_n, long long stride_c,
                                                                  long long stride_t, int y_frames, const int* __restrict__ plan,
                                                                  int batch, float* __restrict__ out, long long out_stride_b,
                                                                  long long out_stride_c, int out_frames,
                                                                  const int* __restrict__ frame_lengths, int* __restrict__ bad) {
    const int n = blockIdx.z, c = blockIdx.y;
    const int i = blockIdx.x * kChThreads + threadIdx.x;
    const int* row = plan + (long long)n * kChPlanInts;
    const int read = row[0], u_lo = row[2], t0 = row[3], count = row[4];
    if (count == 0) return;                                              // a dead chunk
    bool wrong = read < 0 || read >= batch || u_lo < 0 || t0 < 0 || count < 0 || (long long)u_lo + count > y_frames;
    if (!wrong) {
        const int T = frame_lengths[read];
        wrong = T > out_frames || (long long)t0 + count > T;
    }
    if (wrong) {
        if (bad && blockIdx.x == 0 && c == 0 && threadIdx.x == 0) atomicAdd(bad, 1);
        return;
    }
    if (i >= count) return;
    out[(long long)read * out_stride_b + (long long)c * out_stride_c + t0 + i] =
        y[(long long)n * stride_n + (long long)c * stride_c + (long long)(u_lo + i) * stride_t];
}

}  // namespace wn
using namespace wn;

int wn_chunk_gather(const void* signal, int signal_is_int16, int batch, int ld, const int* signal_lengths, const float* scale,
                    const float* shift, const int* plan, int n_chunks, int chunk, float* out, int* bad, wn_stream_t stream) {
    if (batch <= 0 || ld <= 0 || n_chunks <= 0 || chunk <= 0 || chunk % kChPerThread != 0) return WN_ERR_BAD_SHAPE;
    if (n_chunks > 65535 || ld >= kChMaxDim || chunk >= kChMaxDim) return WN_ERR_UNSUPPORTED;
    if (((long long)chunk + kChThreads * kChPerThread - 1) / (kChThreads * kChPerThread) * n_chunks * kChThreads >= kChMaxGridThreads)
        return WN_ERR_UNSUPPORTED;
    if (!signal || !signal_lengths || !plan || !out) return WN_ERR_NULL;
    if (reinterpret_cast<uintptr_t>(out) & 15) return WN_ERR_WORKSPACE;
    const int tile = kChThreads * kChPerThread;
    const dim3 grid((unsigned)((chunk + tile - 1) / tile), (unsigned)n_chunks);
    if (signal_is_int16)
        hipLaunchKernelGGL(chunk_gather_kernel<short>, grid, dim3(kChThreads), 0, (hipStream_t)stream,
                           reinterpret_cast<const short*>(signal), batch, ld, signal_lengths, scale, shift, plan, chunk, out, bad);
    else
        hipLaunchKernelGGL(chunk_gather_kernel<float>, grid, dim3(kChThreads), 0, (hipStream_t)stream,
                           reinterpret_cast<const float*>(signal), batch, ld, signal_lengths, scale, shift, plan, chunk, out, bad);
    WN_HIP(hipGetLastError(), "chunk_gather");
    return WN_OK;
}

int wn_chunk_stitch(const float* y, long long stride_n, long long stride_c, long long stride_t, int y_frames, const int* plan,
                    int n_chunks, int classes, int batch, float* out, long long out_stride_b, long long out_stride_c, int out_frames,
                    const int* frame_lengths, int* bad, wn_stream_t stream) {
    if (batch <= 0 || n_chunks <= 0 || classes <= 0 || y_frames <= 0 || out_frames <= 0) return WN_ERR_BAD_SHAPE;
    if (stride_n < 0 || stride_c < 0 || stride_t < 0 || out_stride_b < 0 || out_stride_c < 0) return WN_ERR_BAD_SHAPE;
    if (n_chunks > 65535 || classes > 65535 || y_frames >= kChMaxDim || out_frames >= kChMaxDim) return WN_ERR_UNSUPPORTED;
    if (((long long)y_frames + kChThreads - 1) / kChThreads * classes * n_chunks * kChThreads >= kChMaxGridThreads) return WN_ERR_UNSUPPORTED;
    if (!y || !plan || !out || !frame_lengths) return WN_ERR_NULL;
    const dim3 grid((unsigned)((y_frames + kChThreads - 1) / kChThreads), (unsigned)classes, (unsigned)n_chunks);
    hipLaunchKernelGGL(chunk_stitch_kernel, grid, dim3(kChThreads), 0, (hipStream_t)stream, y, stride_n, stride_c, stride_t, y_frames,
                       plan, batch, out, out_stride_b, out_stride_c, out_frames, frame_lengths, bad);
    WN_HIP(hipGetLastError(), "chunk_stitch");
    return WN_OK;
}
