// Fused next-sample NLL head: sum over time of the batch-averaged cross entropy of logits [B][C][L] against integer
// targets [B][L] -- the reference computes it with an L-iteration Python loop of CrossEntropyLoss calls
// (Loss.py:38-43, legacy_code/train.py:37-39).
//
// Memory-bound elementwise/reduction work (HBM roofline): time is the contiguous axis, so each thread owns four
// consecutive time steps and walks the C channel rows with 16-byte loads (a wave reads 1 KB contiguous per row);
// an online max/sum gives log-sum-exp in ONE pass over the logits.  Forward writes lse[2][B][L] (kept for backward) and
// one partial loss per workgroup (summed in a fixed order by the caller: deterministic).  Backward is one more pass:
// dlogits = (softmax - onehot) * scale.
//
// lse is kept as its two terms, the maximum m (plane 0) and log sum exp(v - m) (plane 1), and never added up: the sum m + log s is
// rounded to an ulp of |m|, and exp(v - (m + log s)) inherits that as a RELATIVE error of the whole softmax (4e-6 at |m| = 80,
// tests/test_gpu_nll.py), while (v - m) - log s is a difference of nearby numbers minus a small one.  The loss is formed the same way.
#include "wn_kernels.h"

namespace wn {

// Online log-sum-exp, G class rows at a time, of the thread's four time steps: the group's maximum joins the running one first, so
// that every term is exp(v - max) <= 1 with ONE exponential and no select; the running sum is rescaled once per group (one more
// exponential per G elements).  A masked class (v = -inf) contributes exp(-inf) = 0 wherever it stands; while every class so far
// is masked the maximum is still -inf and 0 stands in for it (-inf - (-inf) would be NaN).
// The G terms are summed in fp32 (each <= 1, G of them); the running sum that carries them across the C / G groups is fp64: C
// sequential fp32 additions leave it up to 2e-6 (relative) from the exact sum at C = 256, and the whole softmax of the frame with it
// (tests/test_gpu_nll.py).
template <int G>
__device__ __forceinline__ void lse_group(const float* __restrict__ p, int L, bool vec, int t0, float (&m)[4], double (&s)[4]) {
    float v[G][4];
#pragma unroll
    for (int i = 0; i < G; ++i) {
        if (vec) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(p + (long long)i * L);
            v[i][0] = q[0]; v[i][1] = q[1]; v[i][2] = q[2]; v[i][3] = q[3];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) v[i][j] = t0 + j < L ? p[(long long)i * L + j] : 0.0f;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float gm = m[j];
#pragma unroll
        for (int i = 0; i < G; ++i) gm = fmaxf(gm, v[i][j]);
        const float base = gm == -INFINITY ? 0.0f : gm;
        float g = 0.0f;
#pragma unroll
        for (int i = 0; i < G; ++i) g += __builtin_amdgcn_exp2f(1.44269504088896341f * (v[i][j] - base));
        const float r = __builtin_amdgcn_exp2f(1.44269504088896341f * (m[j] - base));   // 1 while the maximum stands, 0 on the first group
        s[j] = s[j] * (double)r + (double)g;
        m[j] = gm;
    }
}

__global__ __launch_bounds__(256) void nll_forward_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                                          float* __restrict__ lse, float* __restrict__ partial,
                                                          int* __restrict__ bad_targets, int B, int C, int L) {
    const int L4 = (L + 3) / 4;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    float loss = 0.0f;
    if (gid < (long long)B * L4) {
        const int b = (int)(gid / L4), t0 = (int)(gid - (long long)b * L4) * 4;
        const float* p = logits + (long long)b * C * L + t0;
        const bool vec = (L % 4 == 0);               // rows are 16-byte aligned only then
        float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        int c = 0;
        for (; c + 8 <= C; c += 8) lse_group<8>(p + (long long)c * L, L, vec, t0, m, s);
        for (; c < C; ++c) lse_group<1>(p + (long long)c * L, L, vec, t0, m, s);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (t0 + j < L) {
                const float ls = __logf((float)s[j]);
                lse[(long long)b * L + t0 + j] = m[j];
                lse[((long long)B + b) * L + t0 + j] = ls;
                long long tg = target[(long long)b * L + t0 + j];
                if (tg < 0 || tg >= C) {   // never index the logits with an unchecked label: count it, read class 0, poison the loss
                    if (bad_targets) atomicAdd(bad_targets, 1);
                    tg = 0;
                    loss = __builtin_nanf("");
                }
                loss += (m[j] - logits[((long long)b * C + tg) * L + t0 + j]) + ls;
            }
        }
    }
    // workgroup sum in a fixed order: wave shuffles, then 4 partials through LDS
    __shared__ float red[4];
    for (int o = 32; o > 0; o >>= 1) loss += __shfl_down(loss, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = loss;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void nll_backward_kernel(const float* __restrict__ logits, const long long* __restrict__ target,
                                                           const float* __restrict__ lse, const float* __restrict__ gscale,
                                                           float* __restrict__ dlogits, int B, int C, int L) {
    const int L4 = (L + 3) / 4;
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long long)B * L4) return;
    const int b = (int)(gid / L4), t0 = (int)(gid - (long long)b * L4) * 4;
    const float g = gscale[0];
    const bool vec = (L % 4 == 0);
    float m[4], l[4];
    long long tg[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool ok = t0 + j < L;
        m[j] = ok ? lse[(long long)b * L + t0 + j] : 0.0f;
        l[j] = ok ? lse[((long long)B + b) * L + t0 + j] : 0.0f;
        tg[j] = ok ? target[(long long)b * L + t0 + j] : -1;
    }
    const float* p = logits + (long long)b * C * L + t0;
    float* d = dlogits + (long long)b * C * L + t0;
#pragma unroll 8
    for (int c = 0; c < C; ++c) {
        if (vec) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(p + (long long)c * L);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = (__expf((q[j] - m[j]) - l[j]) - (tg[j] == c ? 1.0f : 0.0f)) * g;
            *reinterpret_cast<f32x4*>(d + (long long)c * L) = o;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (t0 + j < L) d[(long long)c * L + j] = (__expf((p[(long long)c * L + j] - m[j]) - l[j]) - (tg[j] == c ? 1.0f : 0.0f)) * g;
        }
    }
}

hipError_t launch_nll_forward(const float* logits, const long long* target, float* lse, float* partial, int* bad_targets, int B, int C,
                              int L, hipStream_t st) {
    const long long n = (long long)B * ((L + 3) / 4);
    hipLaunchKernelGGL(nll_forward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, logits, target, lse, partial,
                       bad_targets, B, C, L);
    return hipGetLastError();
}

hipError_t launch_nll_backward(const float* logits, const long long* target, const float* lse, const float* gscale, float* dlogits,
                               int B, int C, int L, hipStream_t st) {
    const long long n = (long long)B * ((L + 3) / 4);
    hipLaunchKernelGGL(nll_backward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, logits, target, lse, gscale, dlogits, B, C, L);
    return hipGetLastError();
}

}  // namespace wn
