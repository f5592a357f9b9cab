// Signal-to-reference mapping under the k-mer pore model: the first samples of a read against EVERY state
// of a reference's k-mer sequence, start free and end free -- the subsequence form of wn_sigalign.hip's dynamic program (section
// 7k), with the same cost of a sample in a state (wn_signal_dev.h), the same stay / step moves and the same tie rule.  No
// backpointers: a cell carries the state its path started in (the origin) beside its cost.  Integer only after the quantisation.
//
//   signal_map_reference_kernel   bases + model -> the prepared buffer: one int32 per state (its k-mer code, -1 for a wall)
//                                 followed by a copy of the model.  One launch; labels and model rows are validated here.
//   signal_map_kernel<T>          grid (ceil(M / strip), B), 256 threads.  A workgroup owns the END states [a, a + strip) of one
//                                 read.  D(T - 1, j) depends on the columns [j - (T - 1), j] only, so the workgroup starts at
//                                 a - round_up(T - 1, 64) (or 0) with +inf to its left: its owned columns are exact, the halo
//                                 columns are computed and thrown away.  It sweeps its columns left to right in TILES of 1024
//                                 states, 4 consecutive states per thread with their running costs (int64), origins (int32) and
//                                 model rows in registers, T steps per tile, one workgroup barrier per step.  What crosses lanes
//                                 per step is the left neighbour's last slot (cost, origin): a wave shuffle inside a wave, a
//                                 double-buffered LDS pair across waves.  What crosses tiles is the previous tile's rightmost
//                                 column for every t: a [T] array of (int64, int32) in LDS that thread 0 reads TWO steps ahead of
//                                 its use (so that the read of entry t + 1 and the last thread's write of entry t in the same
//                                 step never meet) while the last thread overwrites it in place.  The read's quantised samples
//                                 sit beside it: 16 bytes of dynamic LDS per sample, 64 KiB at T = 4096.  After the last step the
//                                 owned threads write end_cost and reduce their 64-state blocks (16 lanes of 4 states: tiles
//                                 and strips start on multiples of 64) with wave shuffles into block_cost / block_end and the
//                                 block's origin in the workspace.  A bad or empty read gets its fill here, strip by strip.
//   signal_map_pick_kernel        one workgroup per read: the block table to score / end / start / runner_up, and *bad.
//
// Nothing depends on strip: every owned column is the exact recurrence, and the block granule (64) is the ABI's, not the tile's.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"
#include "wn_signal_dev.h"

namespace wn {

constexpr int kSmPer = 4;                     // consecutive states per thread
constexpr int kSmThreads = 256;
constexpr int kSmWaves = kSmThreads / 64;
constexpr int kSmTile = kSmPer * kSmThreads;  // states per tile
constexpr int kSmBlockLanes = WN_MAP_GRANULE / kSmPer;    // the lanes of one 64-state block
constexpr int kSmMaxSignal = 4096;
constexpr int kSmMaxRef = 1 << 26;
constexpr int kSmMaxStrip = 1 << 20;
constexpr int kSmFullChip = 512;              // two workgroups for each of the MI355X's 256 CUs
// a finite cost stays below 2^12 (2^31 + 2^30) in magnitude, far below kPathInf (wn_signal_dev.h)

static_assert(kSmBlockLanes * kSmPer == WN_MAP_GRANULE && kSmTile % WN_MAP_GRANULE == 0 && 64 % kSmBlockLanes == 0, "blocks within waves");

// the prepared buffer: int32 code[round_up(M, 4)], then int32 model[4^k][3]
static inline size_t sm_table_offset(int M) { return ((size_t)M + 3) / 4 * 4; }

__global__ __launch_bounds__(256) void signal_map_reference_kernel(const int* ref, int R, const int* model, int k, int* prepared,
                                                                   long long table_offset, int* bad) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    const int M = R - k + 1, rows3 = 3 << (2 * k);
    if (j < rows3) prepared[table_offset + j] = model[j];
    if (j >= R) return;
    const int v = ref[j];
    int faults = (v < 0 || v > 4) ? 1 : 0;                           // a label outside 0..4 counts once, where it stands
    if (j < M) {
        bool open = true;                                            // every base of the window is in 1..4
        int code = 0;
        for (int i = 0; i < k; ++i) {
            const int w = ref[j + i];
            if (w < 1 || w > 4) open = false;
            code = code * 4 + ((w - 1) & 3);
        }
        if (open) {
            int l, w, o;
            bool ok = true;
            sa_model_row(model, code, &l, &w, &o, &ok);
            if (!ok) { ++faults; open = false; }                     // a state whose model row is out of range: counted, a wall
        }
        prepared[j] = open ? code : -1;
    }
    if (faults && bad) atomicAdd(bad, faults);
}

struct SigMapArgs {
    const void* signal;
    const int* signal_lengths;
    const float* scale_shift;           // [B][2] or nullptr
    const int* codes;                   // prepared: [M]
    const int* model;                   // prepared: [4^k][3]
    long long signal_stride;
    int B, max_signal, M, G, k, weight_shift, max_cost, strip;
    double two_f;
    long long* score;                   // [B]
    int* end;                           // [B]
    int* start;                         // [B]
    long long* runner_up;               // [B]
    long long* block_cost;              // [B][G]
    int* block_end;                     // [B][G]
    long long* end_cost;                // [B][M] or nullptr
    int* block_origin;                  // workspace: [B][G]
    int* bad;
};

template <typename T>
__global__ __launch_bounds__(kSmThreads) void signal_map_kernel(const SigMapArgs a) {
    extern __shared__ __attribute__((aligned(16))) char sm_smem[];
    long long* s_bc = reinterpret_cast<long long*>(sm_smem);         // [max_signal] the previous tile's rightmost column: cost
    int* s_bo = reinterpret_cast<int*>(s_bc + a.max_signal);         // [max_signal] and origin
    int* s_q = s_bo + a.max_signal;                                  // [max_signal] the quantised samples
    __shared__ long long s_ec[2][kSmWaves];                          // every wave's last slot, by step parity
    __shared__ int s_eo[2][kSmWaves];
    __shared__ int s_bad;
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = a.M, S = a.weight_shift, max_cost = a.max_cost;
    const int own0 = (int)blockIdx.x * a.strip;                      // below M <= 2^26
    const int own1 = min(own0 + a.strip, M);
    const int Tn = a.signal_lengths[b];
    long long* bc_out = a.block_cost + (long long)b * a.G;
    int* be_out = a.block_end + (long long)b * a.G;
    int* bo_out = a.block_origin + (long long)b * a.G;
    long long* ec_out = a.end_cost ? a.end_cost + (long long)b * M : nullptr;

    long long fill = 0;                                              // workgroup-uniform
    if (Tn < 0 || Tn > a.max_signal) {
        fill = kPathBadRead;                                         // nothing else of the read is looked at
    } else if (Tn == 0) {
        fill = kPathNone;
    } else {
        if (tid == 0) s_bad = 0;
        __syncthreads();
        const T* sig = (const T*)a.signal + (long long)b * a.signal_stride;
        const auto [scaled, scale, shift] = read_scale(a.scale_shift, b);
        bool ok = true;
        for (int t = tid; t < Tn; t += kSmThreads) {
            int q = 0;
            if (!quantise(sig[t], scaled, scale, shift, a.two_f, &q)) { ok = false; q = 0; }
            s_q[t] = q;
        }
        if (!ok) atomicOr(&s_bad, 1);
        __syncthreads();
        if (s_bad) fill = kPathBadRead;                              // every workgroup of the read finds the same
    }
    if (fill) {
        for (int g = own0 / WN_MAP_GRANULE + tid; g < (own1 + WN_MAP_GRANULE - 1) / WN_MAP_GRANULE; g += kSmThreads) {
            bc_out[g] = fill;
            be_out[g] = -1;
            bo_out[g] = -1;
        }
        if (ec_out)
            for (int j = own0 + tid; j < own1; j += kSmThreads) ec_out[j] = fill;
        return;
    }

    const int halo = (Tn - 1 + 63) / 64 * 64;
    const int first = max(own0 - halo, 0);                           // a multiple of 64, as own0 and the tile are
    const int ncodes = 1 << (2 * a.k);
    for (int c0 = first; c0 < own1; c0 += kSmTile) {
        const bool leftmost = c0 == first;                           // +inf to its left
        int lvl[kSmPer], wgt[kSmPer], off[kSmPer], o[kSmPer];
        long long d[kSmPer];
        unsigned alive = 0;
#pragma unroll
        for (int i = 0; i < kSmPer; ++i) {
            const int col = c0 + kSmPer * tid + i;
            const int code = col < M ? a.codes[col] : -1;
            const bool open = code >= 0 && code < ncodes;
            const int r = open ? code : 0;
            lvl[i] = a.model[3 * r];
            wgt[i] = a.model[3 * r + 1];
            off[i] = a.model[3 * r + 2];
            if (open) alive |= 1u << i;
            d[i] = open ? 0 : kPathInf;                              // before sample 0: the start is free, a wall never opens
            o[i] = col;
        }
        // thread 0's view of the previous tile's rightmost column: la = its cell at t - 1 (used now), lb = at t (used next step)
        long long la = kPathInf, lb = kPathInf;
        int oa = -1, ob = -1;
        if (tid == 0 && !leftmost) { lb = s_bc[0]; ob = s_bo[0]; }
        __syncthreads();                                             // entry 0 is read before the last thread overwrites it

        for (int t = 0; t < Tn; ++t) {
            const int q = s_q[t];
            long long lc = kPathInf;
            int oc = -1;
            if (tid == 0 && !leftmost && t + 1 < Tn) { lc = s_bc[t + 1]; oc = s_bo[t + 1]; }
            long long prev = __shfl_up(d[kSmPer - 1], 1);            // cost_{t-1} and origin of the state to the left
            int prevo = __shfl_up(o[kSmPer - 1], 1);
            if (lane == 0) {
                if (wave == 0) {
                    prev = la;
                    prevo = oa;
                } else if (t > 0) {
                    prev = s_ec[(t - 1) & 1][wave - 1];
                    prevo = s_eo[(t - 1) & 1][wave - 1];
                } else {
                    prev = kPathInf;                                 // at t = 0 nothing steps
                }
            }
#pragma unroll
            for (int i = 0; i < kSmPer; ++i) {
                long long m = d[i];
                int mo = o[i];
                const long long step = prev;
                const int stepo = prevo;
                prev = d[i];
                prevo = o[i];
                if (step < m) { m = step; mo = stepo; }              // the stay first; the step only if strictly smaller
                long long n = kPathInf;
                if (((alive >> i) & 1u) && m < kPathInf) n = m + sa_sample_cost(q, lvl[i], wgt[i], off[i], S, max_cost);
                d[i] = n;
                o[i] = mo;
            }
            if (lane == 63) {
                s_ec[t & 1][wave] = d[kSmPer - 1];
                s_eo[t & 1][wave] = o[kSmPer - 1];
                if (wave == kSmWaves - 1) { s_bc[t] = d[kSmPer - 1]; s_bo[t] = o[kSmPer - 1]; }
            }
            la = lb; oa = ob;
            lb = lc; ob = oc;
            __syncthreads();                                         // one barrier per step
        }

        // the last row of this tile: end_cost, and the 64-state blocks of the owned columns
        long long best = kPathNone;
        int best_end = 0x7fffffff, best_origin = -1;
#pragma unroll
        for (int i = 0; i < kSmPer; ++i) {
            const int col = c0 + kSmPer * tid + i;
            const bool finite = d[i] < kPathInf;                     // only a state below M is ever finite
            if (ec_out && col >= own0 && col < own1) ec_out[col] = finite ? d[i] : kPathNone;
            if (finite && d[i] < best) { best = d[i]; best_end = col; best_origin = o[i]; }
        }
#pragma unroll
        for (int s = 1; s < kSmBlockLanes; s *= 2) {
            const long long oc = __shfl_xor(best, s);
            const int oe = __shfl_xor(best_end, s), oo = __shfl_xor(best_origin, s);
            if (oc < best || (oc == best && oe < best_end)) { best = oc; best_end = oe; best_origin = oo; }
        }
        const int block0 = c0 + kSmPer * tid;                        // of this thread's states
        if ((lane & (kSmBlockLanes - 1)) == 0 && block0 >= own0 && block0 < own1) {
            const int g = block0 / WN_MAP_GRANULE;
            const bool any = best < kPathNone;
            bc_out[g] = best;
            be_out[g] = any ? best_end : -1;
            bo_out[g] = any ? best_origin : -1;
        }
    }
}

__global__ __launch_bounds__(kSmThreads) void signal_map_pick_kernel(const SigMapArgs a) {
    __shared__ long long s_c[kSmThreads];
    __shared__ int s_g[kSmThreads];
    const int b = blockIdx.x, tid = threadIdx.x, G = a.G;
    const int Tn = a.signal_lengths[b];
    const long long* bc = a.block_cost + (long long)b * G;
    const bool bad_len = Tn < 0 || Tn > a.max_signal;
    if (bad_len || Tn == 0 || bc[0] == kPathBadRead) {               // workgroup-uniform; the strips have filled the tables
        if (tid == 0) {
            const bool is_bad = bad_len || Tn != 0;
            a.score[b] = a.runner_up[b] = is_bad ? kPathBadRead : kPathNone;
            a.end[b] = a.start[b] = -1;
            if (is_bad && a.bad) atomicAdd(a.bad, 1);
        }
        return;
    }
    long long best = kPathNone;
    int best_g = 0x7fffffff;
    for (int g = tid; g < G; g += kSmThreads) {
        const long long c = bc[g];
        if (c < best) { best = c; best_g = g; }                      // ascending g: the smallest block of a tie stays
    }
    s_c[tid] = best;
    s_g[tid] = best_g;
    __syncthreads();
    for (int s = kSmThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const long long oc = s_c[tid + s];
            const int og = s_g[tid + s];
            if (oc < s_c[tid] || (oc == s_c[tid] && og < s_g[tid])) { s_c[tid] = oc; s_g[tid] = og; }
        }
        __syncthreads();
    }
    best = s_c[0];
    best_g = s_g[0];
    __syncthreads();                                                 // s_c is reused below
    if (best == kPathNone) {                                         // no finite cell in the last row
        if (tid == 0) {
            a.score[b] = a.runner_up[b] = kPathNone;
            a.end[b] = a.start[b] = -1;
        }
        return;
    }
    const int end = a.block_end[(long long)b * G + best_g];
    // the best block whose states all lie T_b or more from `end`: two such paths share no state
    const long long left = (long long)end - Tn, right = (long long)end + Tn;
    long long other = kPathNone;
    for (int g = tid; g < G; g += kSmThreads) {
        const long long g0 = (long long)g * WN_MAP_GRANULE;
        if (g0 + WN_MAP_GRANULE - 1 <= left || g0 >= right) {
            const long long c = bc[g];
            other = c < other ? c : other;
        }
    }
    s_c[tid] = other;
    __syncthreads();
    for (int s = kSmThreads / 2; s > 0; s >>= 1) {
        if (tid < s) s_c[tid] = s_c[tid + s] < s_c[tid] ? s_c[tid + s] : s_c[tid];
        __syncthreads();
    }
    if (tid == 0) {
        a.score[b] = best;
        a.end[b] = end;
        a.start[b] = a.block_origin[(long long)b * G + best_g];
        a.runner_up[b] = s_c[0];
    }
}

static bool sm_ref_ok(int ref_len, int k) { return k >= 1 && k <= kSigMaxK && ref_len >= k && ref_len <= kSmMaxRef; }

static bool sm_strip_ok(int strip_states) {
    return strip_states == 0 || (strip_states >= WN_MAP_GRANULE && strip_states <= kSmMaxStrip && strip_states % WN_MAP_GRANULE == 0);
}

// the automatic strip: about 8 max_signal end states, so that the halo (below max_signal + 64 columns) is near an eighth of a
// workgroup's work; halved while the grid is short of two workgroups per CU, but never below max_signal (halo above a half)
static int sm_auto_strip(int batch, int max_signal, int M) {
    auto up64 = [](long long v) { return (v + 63) / 64 * 64; };
    long long strip = up64(8ll * max_signal);
    const long long floor_strip = up64(max_signal);
    while (strip / 2 >= floor_strip && (long long)batch * ((M + strip - 1) / strip) < kSmFullChip) strip = up64(strip / 2);
    return (int)(strip > kSmMaxStrip ? kSmMaxStrip : strip);
}

}  // namespace wn
using namespace wn;

size_t wn_signal_map_reference_bytes(int ref_len, int k) {
    if (!sm_ref_ok(ref_len, k)) return 0;
    return ((sm_table_offset(ref_len - k + 1) + (size_t)(3 << (2 * k))) * sizeof(int) + 15) / 16 * 16;
}

int wn_signal_map_reference(const int* ref, int ref_len, const int* model, int k, void* prepared, size_t prepared_bytes, int* bad,
                            wn_stream_t stream) {
    if (ref_len < 1 || ref_len < k) return WN_ERR_BAD_SHAPE;
    if (k < 1 || k > kSigMaxK || ref_len > kSmMaxRef) return WN_ERR_UNSUPPORTED;
    if (!ref || !model || !prepared) return WN_ERR_NULL;
    if (prepared_bytes < wn_signal_map_reference_bytes(ref_len, k) || ((size_t)prepared & 15)) return WN_ERR_WORKSPACE;
    const int M = ref_len - k + 1, rows3 = 3 << (2 * k);
    const int n = ref_len > rows3 ? ref_len : rows3;
    hipLaunchKernelGGL(signal_map_reference_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, ref, ref_len, model, k,
                       (int*)prepared, (long long)sm_table_offset(M), bad);
    WN_HIP(hipGetLastError(), "signal_map_reference");
    return WN_OK;
}

// workspace: the origin of every block minimum, [B][ceil(M / 64)] int32
size_t wn_signal_map_workspace_bytes(int batch, int max_signal, int ref_len, int k, int strip_states) {
    if (batch < 1 || batch > 65535 || max_signal < 1 || max_signal > kSmMaxSignal || !sm_ref_ok(ref_len, k) || !sm_strip_ok(strip_states))
        return 0;
    const size_t G = (size_t)cdiv(ref_len - k + 1, WN_MAP_GRANULE);
    return ((size_t)batch * G * sizeof(int) + 15) / 16 * 16;
}

int wn_signal_map(const void* signal, int signal_kind, long long signal_stride, const int* signal_lengths, const float* scale_shift,
                  const void* prepared, int ref_len, int k, int batch, int max_signal, int frac_bits, int weight_shift, int max_cost,
                  int strip_states, long long* score, int* end, int* start, long long* runner_up, long long* block_cost, int* block_end,
                  long long* end_cost, void* workspace, size_t workspace_bytes, int* bad, wn_stream_t stream) {
    if (batch < 1 || max_signal < 1 || ref_len < 1 || ref_len < k) return WN_ERR_BAD_SHAPE;
    if (signal_stride < 0 || signal_kind < 0 || signal_kind > 1) return WN_ERR_BAD_SHAPE;
    if (k < 1 || k > kSigMaxK || frac_bits < 0 || frac_bits > kSigMaxFrac) return WN_ERR_UNSUPPORTED;
    if (weight_shift < 16 || weight_shift > 63 || max_cost < 1) return WN_ERR_UNSUPPORTED;
    if (max_signal > kSmMaxSignal || ref_len > kSmMaxRef || batch > 65535 || !sm_strip_ok(strip_states)) return WN_ERR_UNSUPPORTED;
    const int M = ref_len - k + 1;
    const int strip = strip_states ? strip_states : sm_auto_strip(batch, max_signal, M);
    const long long nstrips = ((long long)M + strip - 1) / strip;
    if (nstrips * batch >= (1ll << 31)) return WN_ERR_UNSUPPORTED;
    if (!signal || !signal_lengths || !prepared || !score || !end || !start || !runner_up || !block_cost || !block_end || !workspace)
        return WN_ERR_NULL;
    if (workspace_bytes < wn_signal_map_workspace_bytes(batch, max_signal, ref_len, k, strip_states) || ((size_t)workspace & 15))
        return WN_ERR_WORKSPACE;
    if (!signal_aligned(signal, signal_kind)) return WN_ERR_WORKSPACE;

    SigMapArgs a = {};
    a.signal = signal; a.signal_lengths = signal_lengths; a.scale_shift = scale_shift;
    a.codes = (const int*)prepared; a.model = (const int*)prepared + sm_table_offset(M);
    a.signal_stride = signal_stride;
    a.B = batch; a.max_signal = max_signal; a.M = M; a.G = cdiv(M, WN_MAP_GRANULE); a.k = k;
    a.weight_shift = weight_shift; a.max_cost = max_cost; a.strip = strip;
    a.two_f = (double)(1 << frac_bits);
    a.score = score; a.end = end; a.start = start; a.runner_up = runner_up; a.block_cost = block_cost; a.block_end = block_end;
    a.end_cost = end_cost; a.block_origin = (int*)workspace; a.bad = bad;

    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)max_signal * (sizeof(long long) + 2 * sizeof(int));       // at most 64 KiB
    const dim3 grid((unsigned)nstrips, (unsigned)batch);
    if (signal_kind)
        hipLaunchKernelGGL(signal_map_kernel<short>, grid, dim3(kSmThreads), lds, st, a);
    else
        hipLaunchKernelGGL(signal_map_kernel<float>, grid, dim3(kSmThreads), lds, st, a);
    WN_HIP(hipGetLastError(), "signal_map");
    hipLaunchKernelGGL(signal_map_pick_kernel, dim3((unsigned)batch), dim3(kSmThreads), 0, st, a);
    WN_HIP(hipGetLastError(), "signal_map_pick");
    return WN_OK;
}
