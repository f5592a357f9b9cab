// Weight repacking: PyTorch-layout parameters -> MFMA-fragment order for series_gemm_kernel.
//
// Packed layout of one slab:  [k-block g][row-tile m (MT)][lane (64)][q (4)]  floats, where
//   lane = 32*h + i  holds  W[row = 32*m + i][k = 8*g + 4*h + q]
// i.e. exactly the A operand of v_mfma_f32_32x32x2_f32 (lane l: A[i = l&31][k = l>>5]) for the
// four k-steps q of k-block g, so one coalesced global_load_dwordx4 per lane feeds four MFMAs.
// Runs once per optimizer step per block (a few MB), so one thread per output float is plenty.
#include "wn_kernels.h"

namespace wn {

// One output float (and one packed bias) per thread.  `src(set, seg)`, `bias0(set)`, `bias1(set)` resolve the job's source
// pointers: as stored for pack_kernel, relative to the launch's dynamic bases for pack_table_kernel.
template <class SrcFn, class Bias0Fn, class Bias1Fn>
__device__ __forceinline__ void pack_element(const PackArgs& a, long long idx, float* wpacked, float* bias, SrcFn src,
                                             Bias0Fn bias0, Bias1Fn bias1) {
    if (idx < a.total) {
        // locate the slab
        int slab = 0;
        while (slab + 1 < a.nslab && idx >= a.slab_woff[slab + 1]) ++slab;
        const long long rel = idx - a.slab_woff[slab];
        const int q = (int)(rel & 3);
        const int lane = (int)((rel >> 2) & 63);
        const long long gm = rel >> 8;  // g*MT + m
        const int m = (int)(gm % a.MT);
        int g = (int)(gm / a.MT);
        int s = 0;
        while (g >= a.seg_nkb[s]) { g -= a.seg_nkb[s]; ++s; }
        const int c = 8 * g + 4 * (lane >> 5) + q;
        const PackTile t = a.tile[slab * a.MT + m];
        float v = 0.0f;
        if (t.row0 >= 0) {
            const PackSrc& ps = a.set[t.set].seg[s];
            const float* ptr = src(t.set, s);
            const int r = t.row0 + (lane & 31);
            if (ptr && r < ps.rows && c < ps.cols) v = ptr[(long long)r * ps.stride_r + (long long)c * ps.stride_c];
        }
        wpacked[idx] = v;
    }
    // bias: [slab][MT*32]
    const long long nb = (long long)a.nslab * a.MT * 32;
    if (idx < nb && bias) {
        const int slab = (int)(idx / (a.MT * 32));
        const int rr = (int)(idx % (a.MT * 32));
        const PackTile t = a.tile[slab * a.MT + rr / 32];
        float v = 0.0f;
        if (t.row0 >= 0) {
            const int r = t.row0 + (rr & 31);
            if (r < a.set[t.set].bias_rows) {
                const float* p0 = bias0(t.set);
                const float* p1 = bias1(t.set);
                if (p0) v += p0[r];
                if (p1) v += p1[r];
            }
        }
        bias[a.slab_boff[slab] + rr] = v;
    }
}

__global__ __launch_bounds__(256) void pack_kernel(const PackArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    pack_element(a, idx, a.wpacked, a.bias,
                 [&](int set, int seg) { return a.set[set].seg[seg].ptr; },
                 [&](int set) { return a.set[set].bias0; }, [&](int set) { return a.set[set].bias1; });
}

// every job of a table in one launch: workgroups [first_block, first_block of the next job) belong to one job
__global__ __launch_bounds__(256) void pack_table_kernel(const PackJob* __restrict__ jobs, int njobs, const PackBases bases,
                                                         char* packed) {
    int lo = 0, hi = njobs - 1;   // the last job whose first_block <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const PackJob& j = jobs[lo];
    const PackArgs& a = j.a;
    const long long idx = (long long)((int)blockIdx.x - j.first_block) * 256 + threadIdx.x;
    // a dynamic source is never NULL (only existing sources are marked): its pointer field holds the offset from its base
    auto dynp = [&](const float* p, int dyn) -> const float* {
        return dyn < 0 ? p : reinterpret_cast<const float*>(bases.b[dyn] + reinterpret_cast<size_t>(p));
    };
    pack_element(a, idx, reinterpret_cast<float*>(packed + reinterpret_cast<size_t>(a.wpacked)),
                 reinterpret_cast<float*>(packed + reinterpret_cast<size_t>(a.bias)),
                 [&](int set, int seg) { return dynp(a.set[set].seg[seg].ptr, j.seg_dyn[set][seg]); },
                 [&](int set) { return dynp(a.set[set].bias0, j.bias_dyn[set][0]); },
                 [&](int set) { return dynp(a.set[set].bias1, j.bias_dyn[set][1]); });
}

long long pack_job_blocks(const PackArgs& a) {
    long long n = a.total;
    const long long nb = (long long)a.nslab * a.MT * 32;
    if (nb > n) n = nb;
    return n <= 0 ? 0 : (n + 255) / 256;
}

hipError_t launch_pack(const PackArgs& a, hipStream_t st) {
    const long long nblk = pack_job_blocks(a);
    if (nblk <= 0) return hipSuccess;
    hipLaunchKernelGGL(pack_kernel, dim3((unsigned)nblk), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_pack_table(const PackJob* jobs_dev, int njobs, int launch_blocks, const PackBases& bases, void* packed,
                             hipStream_t st) {
    if (njobs <= 0 || launch_blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(pack_table_kernel, dim3((unsigned)launch_blocks), dim3(256), 0, st, jobs_dev, njobs, bases,
                       reinterpret_cast<char*>(packed));
    return hipGetLastError();
}

}  // namespace wn
