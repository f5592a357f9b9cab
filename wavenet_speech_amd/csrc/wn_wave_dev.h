// The cross-lane and cross-wave steps the read tools share, each written once.  Device code only; a wave is
// 64 lanes, lane = tid & 63, wave = tid >> 6.  What each returns in which lanes, its LDS, and ITS BARRIERS:
//   wave_scan<n>(v, lane, op)   inclusive scan by __shfl_up over the first n lanes (a power of two, 64 by default); lanes from n up
//                               hold no result.  No LDS, no barrier.
//   wave_offsets<kWaves>(slot, wave, &before, &total)   from kWaves per-wave totals in LDS: the sum of the slots below `wave` and of
//                               all.  Reads only, no barrier: the caller has one between the writes of the slots and this call.
//   block_scan<kWaves>(v, tid, slot, &total, op = OpAdd, identity = 0, &inclusive = nullptr)   every thread of a workgroup of kWaves
//                               waves calls it; returns the EXCLUSIVE scan of v in thread order, *total in every thread and, if
//                               asked, the inclusive value.  slot: kWaves elements of LDS.  kWaves <= 4: sums; lane 63 writes its
//                               wave's total, ONE barrier, wave_offsets.  Above (up to 64): any op with its identity; a barrier, wave
//                               0 scans the slots in place, a second barrier: TWO.  There is NO barrier after its last read of `slot`:
//                               a caller that writes the slot again puts a __syncthreads() before that, or alternates slots.
//   wave_reduce(v, op)          butterfly by __shfl_xor: op over all 64 lanes, in every lane; wave_reduce_each(op, a, b, ...) does
//                               several values in place, their shuffles interleaved.  No LDS, no barrier.
//   wave_max_dpp(v)             the maximum of an int over the wave by DPP row operations and a readlane: a scalar.
//   wave_shr1(v, fill)          lane l gets lane l - 1's v, lane 0 gets fill (DPP wave_shr:1).  int and double.
//   wave_shl1(v, fill)          lane l gets lane l + 1's v, lane 63 gets fill (DPP wave_shl:1).  int.
//   edge_publish(edge, k, lane, wave, v) / edge_left(edge, k, wave)   the neighbour hand-off of a systolic step over a caller-declared
//                               __shared__ T edge[2][kWaves]: lane 63 stores its wave's last value of step k; lane 0 of a wave > 0
//                               takes what wave - 1 published in step k - 1.  NO barrier in either: the kernel has one __syncthreads()
//                               per step after the publish; it orders step k's stores before step k + 1's loads and frees slot k - 1.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace wn {

struct OpAdd { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct OpMax { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; } };
struct OpOr  { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a | b; } };

template <int kLanes = 64, typename T, typename Op>
__device__ __forceinline__ T wave_scan(T v, int lane, Op op) {
#pragma unroll
    for (int d = 1; d < kLanes; d <<= 1) {
        const T up = __shfl_up(v, d);
        if (lane >= d) v = op(v, up);
    }
    return v;
}

template <int kWaves, typename T>
__device__ __forceinline__ void wave_offsets(const T* slot, int wave, T* before, T* total) {
    T off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const T t = slot[w];
        off += w < wave ? t : 0;
        tot += t;
    }
    *before = off, *total = tot;
}

template <int kWaves, typename T, typename Op = OpAdd>
__device__ __forceinline__ T block_scan(T v, int tid, T* slot, T* total, Op op = Op(), T identity = 0, T* inclusive = nullptr) {
    const int lane = tid & 63, wave = tid >> 6;
    const T inc = wave_scan(v, lane, op);
    T ex = inc - v, before;                                              // of a sum; of any op: the lane to the left
    if constexpr (kWaves > 4) {
        ex = __shfl_up(inc, 1);
        if (lane == 0) ex = identity;
    }
    if (lane == 63) slot[wave] = inc;
    __syncthreads();
    if constexpr (kWaves <= 4) {
        static_assert(std::is_same_v<Op, OpAdd>, "the slot loop sums");
        wave_offsets<kWaves>(slot, wave, &before, total);
    } else {
        if (wave == 0) {
            const T x = wave_scan<kWaves>(lane < kWaves ? slot[lane] : identity, lane, op);
            if (lane < kWaves) slot[lane] = x;
        }
        __syncthreads();
        before = wave > 0 ? slot[wave - 1] : identity;
        *total = slot[kWaves - 1];
    }
    if (inclusive) *inclusive = op(before, inc);
    return op(before, ex);
}

template <typename Op, typename... T>
__device__ __forceinline__ void wave_reduce_each(Op op, T&... v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ((v = op(v, __shfl_xor(v, m))), ...);
}
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) { return wave_reduce_each(op, v), v; }

// quads, half rows and rows by DPP swaps, then the two row broadcasts; lane 63 holds the maximum
__device__ __forceinline__ int wave_max_dpp(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));    // quad_perm [1, 0, 3, 2]
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));    // quad_perm [2, 3, 0, 1]
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));   // row_half_mirror
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));   // row_mirror
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xA, 0xF, false));   // row_bcast15 into rows 1 and 3
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xC, 0xF, false));   // row_bcast31 into rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);
}

constexpr int kDppWaveShr1 = 0x138;      // DPP control word wave_shr:1
__device__ __forceinline__ int wave_shr1(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, kDppWaveShr1, 0xf, 0xf, false); }
__device__ __forceinline__ double wave_shr1(double v, double fill) {
    const int lo = wave_shr1(__double2loint(v), __double2loint(fill)), hi = wave_shr1(__double2hiint(v), __double2hiint(fill));
    return __hiloint2double(hi, lo);
}

constexpr int kDppWaveShl1 = 0x130;      // DPP control word wave_shl:1
__device__ __forceinline__ int wave_shl1(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, kDppWaveShl1, 0xf, 0xf, false); }

template <typename T, int kWaves>
__device__ __forceinline__ void edge_publish(T (*edge)[kWaves], int step, int lane, int wave, T v) { if (lane == 63) edge[step & 1][wave] = v; }
template <typename T, int kWaves>
__device__ __forceinline__ T edge_left(T (*edge)[kWaves], int step, int wave) { return edge[(step - 1) & 1][wave - 1]; }

}  // namespace wn
