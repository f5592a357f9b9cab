// Event tables and k-mer model tables from a segmentation: signal + event boundaries + bases give, per
// event, its k-mer, its clipped sample range and the integer sum and sum of squares of its quantised samples; the used events
// of good reads are then added into per-k-mer tables (events, samples, level sums, dwell histogram).  All sums are integers:
// every reduction order and every atomic order gives the same bits, so nothing below fixes an order.
//
//   kmer_events_kernel<T>   grid (ceil(max_events / 256), batch), 256 threads = 4 waves; a wave takes 64 CONSECUTIVE events, one
//                           lane each.  Consecutive events are contiguous in the signal, so while every event is short (<= 32
//                           samples: one lane sums it serially) the 64 loads of a wave fall in one contiguous region and are
//                           served from cache.  An event above 32 samples is summed by the whole wave, lanes striding its
//                           samples, with an integer butterfly reduction; the wave walks the ballot of such events.  Each
//                           lane validates its own boundaries (against its predecessor's end), its label window and its
//                           samples; anything bad raises the read's flag in the workspace.  Per-read counts go to the workspace
//                           with one integer atomic per wave and counter.
//   kmer_tables_kernel      after the first launch the flags are final.  grid (<= 256) over the flattened [batch][max_events]
//                           rows in contiguous chunks of >= 4096 events.  Bad reads: rows rewritten to -4 / 0, read_counts -1,
//                           *bad + 1, nothing added.  Good reads: events with a k-mer >= 0 add into kmer_stats -- for k <= 5
//                           privatised in LDS (4^k x 5 x 8 B, at most 40 KiB, 64-bit LDS adds; non-zero entries flushed with 64-bit
//                           global atomic adds), for k = 6 straight to global memory -- and into dwell_hist (global adds).
//
// No value of a length, a boundary, a label or a sample is used as an index before it is checked.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"
#include "wn_signal_dev.h"
#include "wn_wave_dev.h"

namespace wn {

constexpr int kEvThreads = 256;
constexpr int kEvShort = 32;                  // up to here one lane sums the event; above, the whole wave
constexpr int kEvMaxLen = 65536;              // samples per event: sum of q^2 < 2^16 * 2^46 = 2^62
constexpr int kEvMaxDwell = 65536;
constexpr int kEvLdsK = 5;                    // kmer_stats lives in LDS up to this k
constexpr long long kEvTableChunk = 4096;     // events per workgroup of the second launch, at least
constexpr int kEvTableBlocks = 256;           // workgroups of the second launch, at most

struct EventArgs {
    const void* signal;
    const int* signal_lengths;
    const float* scale_shift;           // [B][2] or nullptr
    const int* seg_begin;
    const int* seg_end;
    const int* labels;
    const int* label_lengths;
    const int* events;
    long long signal_stride, seg_row_stride, seg_elem_stride, labels_stride;
    int frame_stride, frame_offset;
    int B, N, max_signal, max_labels, k, first, max_dwell;
    double two_f;                       // 2^frac_bits
    int* out_kmer;                      // the caller's rows, or nullptr
    int* out_start;
    int* out_len;
    long long* out_sum;
    long long* out_sumsq;
    int* row_kmer;                      // what the second launch reads: the caller's rows or the workspace's
    int* row_len;
    long long* row_sum;
    long long* row_sumsq;
    int* read_counts;                   // [B][4] or nullptr
    unsigned long long* kmer_stats;     // [4^k][5] or nullptr
    unsigned long long* dwell_hist;     // [4^k][D + 1] or nullptr
    int* flag;                          // workspace: [B]
    int* counts;                        // workspace: [B][4]
    int* bad;
};

template <typename T>
__global__ __launch_bounds__(kEvThreads) void kmer_events_kernel(const EventArgs a) {
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const long long j64 = (long long)blockIdx.x * kEvThreads + tid;
    const int sl = a.signal_lengths[b], ll = a.label_lengths[b], ne = a.events[b];
    const bool lengths_ok = sl >= 0 && sl <= a.max_signal && ll >= 0 && ll <= a.max_labels && ne >= 0 && ne <= a.N;
    if (!lengths_ok) {                                               // nothing of such a read is looked at; the second launch fills its rows
        if (blockIdx.x == 0 && tid == 0) atomicOr(a.flag + b, 1);
        return;
    }
    const bool in_row = j64 < a.N;
    const int j = (int)j64;
    int code = -4, start = 0, len = 0;
    bool bad = false;
    if (in_row && j < ne) {
        const long long so = (long long)b * a.seg_row_stride + (long long)j * a.seg_elem_stride;
        const int bg = a.seg_begin[so], en = a.seg_end[so];
        bool ok = bg >= 0 && en >= bg;
        if (j > 0) ok = ok && bg >= a.seg_end[so - a.seg_elem_stride];          // gaps are fine, overlaps are not
        if (!ok) {
            bad = true;
        } else {
            const long long s0 = (long long)bg * a.frame_stride + a.frame_offset, s1 = (long long)en * a.frame_stride + a.frame_offset;
            const long long c0 = s0 < sl ? s0 : sl, c1 = s1 < sl ? s1 : sl;
            start = (int)c0;
            len = (int)(c1 - c0);
            const long long w0 = j64 + a.first;
            if (len == 0) {
                code = -2;
            } else if (s1 > sl || len > kEvMaxLen) {
                code = -3;
            } else if (w0 < 0 || w0 + a.k > ll) {
                code = -1;
            } else {
                bool labels_ok = true;
                const int idx = kmer_code(a.labels + (long long)b * a.labels_stride + w0, a.k, &labels_ok);
                bad = !labels_ok;
                code = bad ? -4 : idx;
            }
        }
    }

    // ---- the sums of the events that are used so far
    const T* sig = (const T*)a.signal + (long long)b * a.signal_stride;
    const auto [scaled, scale, shift] = read_scale(a.scale_shift, b);
    const bool need = code >= 0;
    long long sum = 0, sumsq = 0;
    if (need && len <= kEvShort) {
        for (int t = 0; t < len; ++t) {                              // start + t < sl <= max_signal
            int q;
            if (!quantise(sig[start + t], scaled, scale, shift, a.two_f, &q)) { bad = true; q = 0; }
            sum += q;
            sumsq += (long long)q * q;
        }
    }
    unsigned long long wide = __ballot(need && len > kEvShort);
    while (wide) {                                                   // wave-uniform
        const int src = __ffsll((long long)wide) - 1;
        wide &= wide - 1;
        const int st = __shfl(start, src), ln = __shfl(len, src);
        long long s = 0, s2 = 0;
        int bd = 0;
        for (int t = lane; t < ln; t += 64) {
            int q;
            if (!quantise(sig[st + t], scaled, scale, shift, a.two_f, &q)) { bd = 1; q = 0; }
            s += q;
            s2 += (long long)q * q;
        }
        wave_reduce_each(OpAdd(), s, s2);
        bd = wave_reduce(bd, OpOr());
        if (lane == src) { sum = s; sumsq = s2; bad = bad || bd != 0; }
    }
    if (bad) { code = -4; sum = 0; sumsq = 0; }                      // the read is bad: the second launch rewrites its rows

    if (__ballot(bad) != 0ull && lane == 0) atomicOr(a.flag + b, 1);
    const int n_used = __popcll(__ballot(code >= 0)), n_off = __popcll(__ballot(code == -1));
    const int n_skip = __popcll(__ballot(code == -2 || code == -3));
    const int n_samples = wave_reduce(code >= 0 ? len : 0, OpAdd());     // <= 64 * 65536 per wave
    if (lane == 0) {
        if (n_used) atomicAdd(a.counts + 4 * b + 0, n_used);
        if (n_off) atomicAdd(a.counts + 4 * b + 1, n_off);
        if (n_skip) atomicAdd(a.counts + 4 * b + 2, n_skip);
        if (n_samples) atomicAdd(a.counts + 4 * b + 3, n_samples);
    }
    if (!in_row) return;
    const long long e = (long long)b * a.N + j;
    if (code < 0) { sum = 0; sumsq = 0; }
    if (code == -4) { start = 0; len = 0; }
    a.row_kmer[e] = code;
    a.row_len[e] = len;
    a.row_sum[e] = sum;
    a.row_sumsq[e] = sumsq;
    if (a.out_start) a.out_start[e] = start;
}

__global__ __launch_bounds__(kEvThreads) void kmer_tables_kernel(const EventArgs a, long long total, long long chunk) {
    extern __shared__ unsigned long long s_stats[];                  // [4^k][5] when the table is privatised
    const int tid = threadIdx.x;
    const int entries = 5 << (2 * a.k);
    const bool lds = a.kmer_stats != nullptr && a.k <= kEvLdsK;
    if (lds) {
        for (int i = tid; i < entries; i += kEvThreads) s_stats[i] = 0ull;
        __syncthreads();
    }
    const long long e0 = (long long)blockIdx.x * chunk, e1 = e0 + chunk < total ? e0 + chunk : total;
    for (long long e = e0 + tid; e < e1; e += kEvThreads) {
        const int b = (int)(e / a.N), j = (int)(e - (long long)b * a.N);
        const bool read_bad = a.flag[b] != 0;
        if (j == 0) {                                                // one thread per read
            if (a.read_counts)
                for (int i = 0; i < 4; ++i) a.read_counts[4 * b + i] = read_bad ? -1 : a.counts[4 * b + i];
            if (read_bad && a.bad) atomicAdd(a.bad, 1);
        }
        if (read_bad) {
            if (a.out_kmer) a.out_kmer[e] = -4;
            if (a.out_start) a.out_start[e] = 0;
            if (a.out_len) a.out_len[e] = 0;
            if (a.out_sum) a.out_sum[e] = 0;
            if (a.out_sumsq) a.out_sumsq[e] = 0;
            continue;
        }
        const int code = a.row_kmer[e];
        if (code < 0 || (!a.kmer_stats && !a.dwell_hist)) continue;
        const int len = a.row_len[e];                                // 1 .. 65536, written by the first launch
        if (a.kmer_stats) {
            const unsigned long long s1 = (unsigned long long)a.row_sum[e], s2 = (unsigned long long)a.row_sumsq[e];
            unsigned long long* t = (lds ? s_stats : a.kmer_stats) + 5 * code;
            atomicAdd(t + 0, 1ull);
            atomicAdd(t + 1, (unsigned long long)len);
            atomicAdd(t + 2, s1);                                    // two's complement: the signed sum
            atomicAdd(t + 3, s2 & 0xffffffffull);
            atomicAdd(t + 4, s2 >> 32);
        }
        if (a.dwell_hist)
            atomicAdd(a.dwell_hist + (long long)code * (a.max_dwell + 1) + (len < a.max_dwell ? len : a.max_dwell), 1ull);
    }
    if (lds) {
        __syncthreads();
        for (int i = tid; i < entries; i += kEvThreads) {
            const unsigned long long v = s_stats[i];
            if (v != 0ull) atomicAdd(a.kmer_stats + i, v);
        }
    }
}

static size_t events_header_bytes(int batch) { return align256((size_t)batch * 5 * sizeof(int)); }

}  // namespace wn
using namespace wn;

size_t wn_kmer_events_workspace_bytes(int batch, int max_events) {
    if (batch < 1 || batch > 65535 || max_events < 1) return 0;
    const size_t rows = (size_t)batch * (size_t)max_events;
    return events_header_bytes(batch) + 2 * align256(rows * sizeof(int)) + 2 * align256(rows * sizeof(long long));
}

int wn_kmer_events(const void* signal, int signal_kind, long long signal_stride, const int* signal_lengths, const float* scale_shift,
                   const int* seg_begin, const int* seg_end, long long seg_row_stride, long long seg_elem_stride, int frame_stride,
                   int frame_offset, const int* labels, long long labels_stride, const int* label_lengths, const int* events,
                   int batch, int max_signal, int max_labels, int max_events, int k, int first, int frac_bits, int max_dwell,
                   int* ev_kmer, int* ev_start, int* ev_len, long long* ev_sum, long long* ev_sumsq, int* read_counts,
                   long long* kmer_stats, long long* dwell_hist, void* workspace, size_t workspace_bytes, int* bad,
                   wn_stream_t stream) {
    if (batch < 1 || max_events < 1 || max_signal < 1 || max_labels < 1) return WN_ERR_BAD_SHAPE;
    if (signal_stride < 0 || seg_row_stride < 0 || seg_elem_stride < 0 || labels_stride < 0) return WN_ERR_BAD_SHAPE;
    if (frame_stride < 1 || frame_offset < 0 || signal_kind < 0 || signal_kind > 1) return WN_ERR_BAD_SHAPE;
    if (k < 1 || k > kSigMaxK || first < -kSigMaxFirst || first > kSigMaxFirst) return WN_ERR_UNSUPPORTED;
    if (frac_bits < 0 || frac_bits > kSigMaxFrac || max_dwell < 1 || max_dwell > kEvMaxDwell) return WN_ERR_UNSUPPORTED;
    if (batch > 65535 || (long long)max_signal * frame_stride >= (1ll << 31)) return WN_ERR_UNSUPPORTED;
    if (!signal || !signal_lengths || !seg_begin || !seg_end || !labels || !label_lengths || !events) return WN_ERR_NULL;
    if (!workspace) return WN_ERR_NULL;                              // the per-read flags live there: tables or not
    if (!ev_kmer && !ev_start && !ev_len && !ev_sum && !ev_sumsq && !read_counts && !kmer_stats && !dwell_hist) return WN_ERR_NULL;
    if (workspace_bytes < wn_kmer_events_workspace_bytes(batch, max_events) || ((size_t)workspace & 15)) return WN_ERR_WORKSPACE;
    if (!signal_aligned(signal, signal_kind)) return WN_ERR_WORKSPACE;

    const size_t rows = (size_t)batch * (size_t)max_events;
    char* ws = (char*)workspace;
    EventArgs a = {};
    a.flag = (int*)ws;
    a.counts = a.flag + batch;
    ws += events_header_bytes(batch);
    int* ws_kmer = (int*)ws;            ws += align256(rows * sizeof(int));
    int* ws_len = (int*)ws;             ws += align256(rows * sizeof(int));
    long long* ws_sum = (long long*)ws; ws += align256(rows * sizeof(long long));
    long long* ws_sumsq = (long long*)ws;
    a.signal = signal; a.signal_lengths = signal_lengths; a.scale_shift = scale_shift;
    a.seg_begin = seg_begin; a.seg_end = seg_end; a.labels = labels; a.label_lengths = label_lengths; a.events = events;
    a.signal_stride = signal_stride; a.seg_row_stride = seg_row_stride; a.seg_elem_stride = seg_elem_stride;
    a.labels_stride = labels_stride;
    a.frame_stride = frame_stride; a.frame_offset = frame_offset;
    a.B = batch; a.N = max_events; a.max_signal = max_signal; a.max_labels = max_labels; a.k = k; a.first = first;
    a.max_dwell = max_dwell;
    a.two_f = (double)(1 << frac_bits);
    a.out_kmer = ev_kmer; a.out_start = ev_start; a.out_len = ev_len; a.out_sum = ev_sum; a.out_sumsq = ev_sumsq;
    a.row_kmer = ev_kmer ? ev_kmer : ws_kmer;
    a.row_len = ev_len ? ev_len : ws_len;
    a.row_sum = ev_sum ? ev_sum : ws_sum;
    a.row_sumsq = ev_sumsq ? ev_sumsq : ws_sumsq;
    a.read_counts = read_counts;
    a.kmer_stats = (unsigned long long*)kmer_stats; a.dwell_hist = (unsigned long long*)dwell_hist;
    a.bad = bad;

    hipStream_t st = (hipStream_t)stream;
    WN_HIP(hipMemsetAsync(a.flag, 0, (size_t)batch * 5 * sizeof(int), st), "kmer_events flags");
    const dim3 grid1((unsigned)cdiv(max_events, kEvThreads), (unsigned)batch);
    if (signal_kind)
        hipLaunchKernelGGL(kmer_events_kernel<short>, grid1, dim3(kEvThreads), 0, st, a);
    else
        hipLaunchKernelGGL(kmer_events_kernel<float>, grid1, dim3(kEvThreads), 0, st, a);
    WN_HIP(hipGetLastError(), "kmer_events");
    const long long total = (long long)rows;
    long long blocks = (total + kEvTableChunk - 1) / kEvTableChunk;
    blocks = blocks < 1 ? 1 : blocks > kEvTableBlocks ? kEvTableBlocks : blocks;
    const long long chunk = ((total + blocks - 1) / blocks + kEvThreads - 1) / kEvThreads * kEvThreads;
    const size_t lds = kmer_stats && k <= kEvLdsK ? (size_t)(5 << (2 * k)) * sizeof(unsigned long long) : 0;
    hipLaunchKernelGGL(kmer_tables_kernel, dim3((unsigned)blocks), dim3(kEvThreads), lds, st, a, total, chunk);
    WN_HIP(hipGetLastError(), "kmer_tables");
    return WN_OK;
}
