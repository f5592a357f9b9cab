// What the kernels that walk an op string of wn_pair_align share (wn_profile.hip, wn_pileup.hip): one workgroup of 256 threads per
// pair, the ops in tiles of 256 columns, and the reference / query index of every column as a ballot prefix sum.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace wn
