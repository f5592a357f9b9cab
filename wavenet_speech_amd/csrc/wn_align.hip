// CTC forced alignment on the device: given the model's frame log-probabilities and a KNOWN label sequence, the single best
// alignment (Viterbi path) over the 2 L + 1 blank-extended states -- which frames belong to which label -- with its
// log-probability.  The third CTC operation next to the loss (wn_ctc.hip, the sum over all alignments) and the decoders
// (wn_decode.hip, labels unknown).  The input is read in place through element strides, as the decoders read it.
//
//   ctc_align_kernel<multi>   one workgroup per utterance, two phases in one launch.
//
//     forward   delta_t(s) = lp[l'_s][t] + max(delta_{t-1}(s), delta_{t-1}(s-1), [delta_{t-1}(s-2)])    in float64, max-plus: one
//               compare/select and one add per predecessor, no exp / log in the loop.  Every thread owns 8 CONSECUTIVE states
//               (s = 8 tid + i), so its delta values stay in registers and only ONE value crosses lanes per step: state 8 tid is
//               a blank (no skip into it) and state 8 tid + 1 skips from 8 tid - 1, so both need the left neighbour's last
//               state only.  Inside a wave that is one DPP wavefront shift (two dwords); across waves it goes through a
//               double-buffered LDS slot and one workgroup barrier per step.  Up to 255 labels (511 states) fit in ONE wave:
//               that instantiation has no barrier in its step at all.  The thread's eight 2-bit backpointers are one 16-bit
//               store to the workspace, bp[b][t][Sp / 4] bytes.  Frame log-probabilities are staged 64 frames at a time in LDS
//               as float64 [frame][class]; logits get their log-softmax there (float64 exp / log, one lane per frame).
//     trace     backwards in chunks of 64 frames.  The path moves at most 2 states per frame, so a chunk that ends in state s
//               reads backpointer columns (s - 128, s] only: 9 words per frame, loaded into LDS by all threads; one lane walks
//               the 64 steps in LDS (no chain of dependent global loads), then the threads write states, frame labels and span
//               boundaries of the chunk.  A span starts where the state is odd and differs from the previous frame's.
//
// Ties (part of the contract, tests/ctc_align_ref.py holds the same rule): predecessors are tried in the order s, s-1, s-2 and a
// later one replaces an earlier one only if strictly greater; the path ends in S-1 unless delta(S-2) is strictly greater.
// float64 because a score near -5400 over 4096 frames carries 1e-3 of fp32 rounding while per-frame decision margins of random
// logits go down to 4e-4.  States at or beyond S hold values that are never read by a state below S (moves only go up).
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"
#include "wn_wave_dev.h"

namespace wn {

constexpr int kAlnPer = 8;              // consecutive states per thread
constexpr int kAlnMaxThreads = 512;     // 4096 states: 2047 labels
constexpr int kAlnChunk = 64;           // frames staged (forward) and walked (trace) at a time
constexpr int kAlnWinWords = 9;         // 32-bit backpointer words (16 states each) per frame of a trace window
constexpr int kAlnMaxClasses = 64;
constexpr int kAlnMaxLabels = 2047;
constexpr int kAlnMaxLength = 1 << 24;

struct AlignArgs {
    const float* x;                     // element (b, c, t) at x[b * sb + c * sc + t * st]
    long long sb, sc, st;
    const long long* labels;            // [B][Lmax]
    const long long* label_len;         // [B]
    const long long* input_len;         // [B] or nullptr (= T)
    int* states;                        // [B][T]
    int* frame_labels;                  // [B][T] or nullptr
    int* spans;                         // [B][Lmax][2] or nullptr
    float* score;                       // [B]
    unsigned short* bp;                 // [B][T][row_threads]: eight 2-bit backpointers per entry
    int* bad;
    int B, C, T, Lmax, row_threads, blank, kind;   // kind: 0 logits, 1 probabilities, 2 log-probabilities
};

template <bool kMulti>
__global__ __launch_bounds__(kMulti ? kAlnMaxThreads : 64) void ctc_align_kernel(const AlignArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* ly = reinterpret_cast<double*>(smem);                        // [kAlnChunk][C] frame log-probabilities
    __shared__ double edge[2][kAlnMaxThreads / 64];                      // last state of every wave, by step parity
    __shared__ double fin[2];                                            // delta_{Tb-1}(S-2), delta_{Tb-1}(S-1)
    __shared__ unsigned win[kAlnChunk * kAlnWinWords];
    __shared__ int pth[kAlnChunk + 2];                                   // [0] state before the chunk, [1 + f], then the state after
    __shared__ int lbad;
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, T = a.T, blank = a.blank;
    const double kNegInf = -__builtin_huge_val();
    long long Tb = a.input_len ? a.input_len[b] : T;
    long long Lb = a.label_len[b];
    const bool bad_len = Tb < 0 || Tb > T || Lb < 0 || Lb > a.Lmax;
    if (bad_len) { Tb = 0; Lb = 0; }
    const int S = 2 * (int)Lb + 1, nT = (int)Tb;
    const long long* lab = a.labels + (long long)b * a.Lmax;
    if (tid == 0) { lbad = bad_len ? 1 : 0; fin[0] = kNegInf; fin[1] = kNegInf; }
    __syncthreads();

    // this thread's states 8 tid .. 8 tid + 7: even ones are blanks, odd ones the labels 4 tid .. 4 tid + 3
    int cls[kAlnPer / 2];
    unsigned skipm = 0;                                                  // bit k: label 4 tid + k differs from the one before it
    bool my_bad = false;
#pragma unroll
    for (int k = 0; k < kAlnPer / 2; ++k) {
        const int j = (kAlnPer / 2) * tid + k;
        cls[k] = blank;
        if (j < (int)Lb) {
            const long long l = lab[j];
            if (l < 0 || l >= C || l == blank) my_bad = true;            // the value is never used as an index
            else cls[k] = (int)l;
            if (j >= 1 && l != lab[j - 1]) skipm |= 1u << k;
        }
    }
    if (my_bad) atomicOr(&lbad, 1);
    __syncthreads();
    const bool poisoned = lbad != 0;

    double d[kAlnPer];
#pragma unroll
    for (int i = 0; i < kAlnPer; ++i) d[i] = kNegInf;
    const float* xb = a.x + (long long)b * a.sb;
    const bool run = !poisoned && nT > 0;
    if (run) {
        unsigned short* bprow = a.bp + (long long)b * T * a.row_threads;
        for (int t = 0; t < nT; ++t) {
            const int kc = t & (kAlnChunk - 1);
            if (kc == 0) {
                __syncthreads();                                         // the previous chunk is no longer read
                for (int i = tid; i < C * kAlnChunk; i += nthr) {
                    const int c = i / kAlnChunk, kk = i - c * kAlnChunk;
                    double v = 0.0;
                    if (t + kk < nT) {
                        v = (double)xb[(long long)c * a.sc + (long long)(t + kk) * a.st];
                        if (a.kind == 1) v = log(v);                     // a probability of 0 becomes -inf
                    }
                    ly[kk * C + c] = v;
                }
                __syncthreads();
                if (a.kind == 0 && tid < kAlnChunk) {                    // log-softmax over the classes, one lane per frame
                    double* r = ly + tid * C;
                    double m = r[0];
                    for (int c = 1; c < C; ++c) m = fmax(m, r[c]);
                    double sum = 0.0;
                    for (int c = 0; c < C; ++c) sum += exp(r[c] - m);
                    const double z = m + log(sum);
                    for (int c = 0; c < C; ++c) r[c] -= z;
                }
                __syncthreads();
            }
            const double* row = ly + kc * C;
            const double eb = row[blank];
            double el[kAlnPer / 2];
#pragma unroll
            for (int k = 0; k < kAlnPer / 2; ++k) el[k] = row[cls[k]];
            double n[kAlnPer];
            unsigned bpw = 0;
            if (t == 0) {                                                // paths start in the first blank or the first label
#pragma unroll
                for (int i = 0; i < kAlnPer; ++i) n[i] = kNegInf;
                if (tid == 0) { n[0] = eb; n[1] = S > 1 ? el[0] : kNegInf; }
            } else {
                double left = wave_shr1(d[kAlnPer - 1], kNegInf);        // the left neighbour's last state
                if (kMulti && lane == 0 && wave > 0) left = edge_left(edge, t, wave);
#pragma unroll
                for (int i = 0; i < kAlnPer; ++i) {
                    double m = d[i];
                    unsigned bp = 0;
                    const double p1 = i == 0 ? left : d[i - 1];
                    if (p1 > m) { m = p1; bp = 1; }
                    if (i & 1) {
                        const double p2 = i == 1 ? left : d[i >= 2 ? i - 2 : 0];
                        if (((skipm >> (i >> 1)) & 1u) && p2 > m) { m = p2; bp = 2; }
                    }
                    n[i] = m + ((i & 1) ? el[i >> 1] : eb);
                    bpw |= bp << (2 * i);
                }
            }
#pragma unroll
            for (int i = 0; i < kAlnPer; ++i) d[i] = n[i];
            if (kMulti) {
                edge_publish(edge, t, lane, wave, d[kAlnPer - 1]);
                __syncthreads();                                         // one barrier per step: the slot of step t-1 is free again
            }
            if (tid < a.row_threads) bprow[(long long)t * a.row_threads + tid] = (unsigned short)bpw;
        }
#pragma unroll
        for (int i = 0; i < kAlnPer; ++i) {
            const int s = kAlnPer * tid + i;
            if (s == S - 1) fin[1] = d[i];
            if (s == S - 2) fin[0] = d[i];
        }
    }
    __syncthreads();                                                     // fin, and this workgroup's backpointer rows, are visible

    // paths end in the last blank or the last label; the last blank unless the label is strictly better
    const double d_last = fin[1], d_label = fin[0];
    int s_end = d_label > d_last ? S - 2 : S - 1;
    const double best = d_label > d_last ? d_label : d_last;
    const bool traced = run && best > kNegInf;
    if (tid == 0) {
        float sc;
        if (poisoned) sc = __builtin_nanf("");
        else if (nT == 0) sc = Lb == 0 ? 0.0f : -__builtin_huge_valf();  // no frames: only the empty labelling aligns
        else sc = (float)best;
        a.score[b] = sc;
        if (poisoned && a.bad) atomicAdd(a.bad, 1);
    }
    int* st_out = a.states + (long long)b * T;
    int* fl_out = a.frame_labels ? a.frame_labels + (long long)b * T : nullptr;
    int* sp_out = a.spans ? a.spans + (long long)b * a.Lmax * 2 : nullptr;
    for (int t = (traced ? nT : 0) + tid; t < T; t += nthr) {
        st_out[t] = -1;
        if (fl_out) fl_out[t] = -1;
    }
    if (sp_out)
        for (int i = (traced ? 2 * (int)Lb : 0) + tid; i < 2 * a.Lmax; i += nthr) sp_out[i] = -1;
    if (!traced) return;

    const int row_words = a.row_threads / 2;
    const unsigned* bpw32 = reinterpret_cast<const unsigned*>(a.bp + (long long)b * T * a.row_threads);
    int after = -1;                                                      // state of the frame after the chunk
    for (int t0 = (nT - 1) / kAlnChunk * kAlnChunk; t0 >= 0; t0 -= kAlnChunk) {
        const int nf = min(kAlnChunk, nT - t0);
        const int w0 = max(s_end - (2 * kAlnChunk - 1), 0) >> 4;         // first word of the window (s_end - 128, s_end]
        for (int i = tid; i < nf * kAlnWinWords; i += nthr) {
            const int f = i / kAlnWinWords, w = w0 + (i - f * kAlnWinWords);
            win[i] = w < row_words ? bpw32[(long long)(t0 + f) * row_words + w] : 0u;
        }
        __syncthreads();                                                 // window loaded; pth of the previous chunk was read
        if (tid == 0) {
            pth[nf + 1] = after;
            int s = s_end;
            for (int f = nf - 1; f >= 0; --f) {
                pth[f + 1] = s;
                const unsigned w = win[f * kAlnWinWords + ((s >> 4) - w0)];
                s -= (int)((w >> ((s & 15) * 2)) & 3u);                  // row 0 holds zeros: the state of frame 0 stays
            }
            pth[0] = t0 > 0 ? s : -1;
        }
        __syncthreads();
        for (int f = tid; f < nf; f += nthr) {
            const int prev = pth[f], pi = pth[f + 1], next = pth[f + 2], t = t0 + f;
            st_out[t] = pi;
            if (fl_out) fl_out[t] = (pi & 1) ? (int)lab[pi >> 1] : blank;
            if (sp_out && (pi & 1)) {
                if (prev != pi) sp_out[(pi >> 1) * 2] = t;
                if (next != pi) sp_out[(pi >> 1) * 2 + 1] = t + 1;
            }
        }
        s_end = pth[0];
        after = pth[1];
    }
}

}  // namespace wn

using namespace wn;

static int check_align(int batch, int classes, int length, int max_label_len) {
    if (batch <= 0 || classes <= 1 || length <= 0 || max_label_len <= 0) return WN_ERR_BAD_SHAPE;
    if (classes > kAlnMaxClasses || max_label_len > kAlnMaxLabels || length > kAlnMaxLength || batch > 65535)
        return WN_ERR_UNSUPPORTED;
    if ((double)batch * (double)length >= 2147483648.0) return WN_ERR_UNSUPPORTED;
    return WN_OK;
}
// workspace: backpointers, 2 bits per state, [B][T][Sp / 4] bytes (Sp a multiple of 64: every row a multiple of 16 bytes)
size_t wn_ctc_align_workspace_bytes(int batch, int classes, int length, int max_label_len) {
    if (check_align(batch, classes, length, max_label_len) != WN_OK) return 0;
    return (size_t)batch * (size_t)length * (size_t)(ctc_states_padded(max_label_len) / 4);
}

int wn_ctc_align(const float* x, long long sb, long long sc, long long st, int input_kind, const long long* labels,
                 const long long* label_lengths, const long long* input_lengths, int batch, int classes, int length,
                 int max_label_len, int blank, int* states, int* frame_labels, int* spans, float* score, void* workspace,
                 size_t workspace_bytes, int* bad, wn_stream_t stream) {
    const int rc = check_align(batch, classes, length, max_label_len);
    if (rc == WN_ERR_BAD_SHAPE) return rc;
    if (input_kind < 0 || input_kind > 2 || blank < 0 || blank >= classes) return WN_ERR_BAD_SHAPE;
    if (rc != WN_OK) return rc;
    if (!x || !labels || !label_lengths || !states || !score || !workspace) return WN_ERR_NULL;
    if (workspace_bytes < wn_ctc_align_workspace_bytes(batch, classes, length, max_label_len)) return WN_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return WN_ERR_WORKSPACE;
    AlignArgs a = {};
    a.x = x; a.sb = sb; a.sc = sc; a.st = st; a.labels = labels; a.label_len = label_lengths; a.input_len = input_lengths;
    a.states = states; a.frame_labels = frame_labels; a.spans = spans; a.score = score; a.bad = bad;
    a.bp = reinterpret_cast<unsigned short*>(workspace);
    a.B = batch; a.C = classes; a.T = length; a.Lmax = max_label_len; a.blank = blank; a.kind = input_kind;
    a.row_threads = ctc_states_padded(max_label_len) / kAlnPer;
    const int threads = (a.row_threads + 63) / 64 * 64;                  // 64 (one wave, no barrier per step) up to 512
    const size_t lds = (size_t)kAlnChunk * classes * sizeof(double);
    hipStream_t s = (hipStream_t)stream;
    if (threads == 64) hipLaunchKernelGGL(ctc_align_kernel<false>, dim3(batch), dim3(64), lds, s, a);
    else hipLaunchKernelGGL(ctc_align_kernel<true>, dim3(batch), dim3(threads), lds, s, a);
    WN_HIP(hipGetLastError(), "ctc_align");
    return WN_OK;
}
