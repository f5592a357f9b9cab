// CTC decoding on the device: what the reference's evaluation notebooks run after the model (softmax, argmax_decode +
// labels2strings, then ctcdecode's CTCBeamDecoder), on the stack's own [B][C][T] logits -- or any (batch, class, time)
// element strides, so ctcdecode's (B, T, C) probabilities are read in place too.
//
//   ctc_greedy_kernel      one workgroup per utterance.  Per chunk of 256 frames: argmax over the classes per lane (ties to the
//                          lowest class, as torch.argmax), emit = label != blank && label != previous frame's label, a
//                          workgroup prefix scan of the emit flags (wave ballots + 4 wave totals), compacted stores.
//   ctc_beam_kernel        CTC prefix beam search without a language model (Hannun et al. 2014), one workgroup per utterance,
//                          T sequential steps of three barriers each:
//                            1. merge map: beam w' (prefix l') is the extension of beam w by last(l') when
//                               hash(l) == hash(l'[:-1]) and len(l) == len(l') - 1;  one search of W x W per step
//                            2. W x C candidates: the stay of each beam (blank / repeat, plus the merged extension) and its
//                               C - 1 extensions; each gets a 64-bit key: orderable score bits high, ~candidate key low
//                            3. selection by rank: a candidate with fewer than W larger keys is kept, in slot = its rank
//                          Scores are log-space fp32 relative to the best beam of the previous step; the offset is summed in
//                          float64.  Every kept extension writes a node {parent node, frame, label} to a caller-owned pool.
//   ctc_beam_walk_kernel   one workgroup per (beam, utterance): walk the final beam's node chain (len(prefix) dependent loads)
//                          and write labels / frames back to front, zero padding after.
//
// Candidate key: a stay of the beam of rank r at t-1 has key (r, 0), an extension of it by class c has (r, 1 + c); equal scores
// go to the smaller key, and a merged candidate (an extension that equals a live beam's prefix, summed into that beam's stay)
// keeps the smaller of the two keys and that contributor's backpointer.  Keys are unique, so the selection is a total order.
// The one deviation from exact prefix merging: two different prefixes of equal length whose 64-bit hashes collide.
#include "../../include/wavenet_amd.h"
#include "wn_host.h"
#include "wn_kernels.h"

namespace wn {

constexpr int kDecThreads = 256;
constexpr int kDecChunk = 32;           // frames of log-probabilities staged per refill (beam)
constexpr int kDecMaxClasses = 64;
constexpr int kDecMaxBeam = 64;
constexpr int kDecMaxLength = 1 << 24;  // node ids t * W + slot stay below 2^31

struct DecodeArgs {
    const float* x;                     // element (b, c, t) at x[b * sb + c * sc + t * st]
    long long sb, sc, st;
    const long long* input_len;         // [B] or nullptr (= T)
    int* labels;                        // greedy [B][T], beam [B][W][T]
    int* frames;                        // same shape or nullptr
    int* lengths;                       // greedy [B], beam [B][W]
    float* scores;                      // beam [B][W]
    int2* nodes;                        // beam [B][T][W] {parent node, frame << 7 | label}
    int* final_node;                    // beam [B][W]
    int* bad;
    int B, C, T, W, blank, kind;        // kind: 0 logits, 1 probabilities, 2 log-probabilities
};

// ---------------------------------------------------------------------------------------------------------------- greedy

__global__ __launch_bounds__(kDecThreads) void ctc_greedy_kernel(const DecodeArgs a) {
    __shared__ int wave_total[kDecThreads / 64];
    __shared__ int wave_last[kDecThreads / 64];
    __shared__ int last_of_chunk;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int C = a.C, T = a.T;
    long long Tb = a.input_len ? a.input_len[b] : T;
    const bool bad = Tb < 0 || Tb > T || a.blank < 0 || a.blank >= C;
    if (bad) {
        Tb = 0;
        if (tid == 0 && a.bad) atomicAdd(a.bad, 1);
    }
    if (tid == 0) last_of_chunk = -1;
    const float* xb = a.x + (long long)b * a.sb;
    int* lab = a.labels + (long long)b * T;
    int* frm = a.frames ? a.frames + (long long)b * T : nullptr;
    int count = 0;                                                   // labels emitted before this chunk (same in every thread)
    for (int t0 = 0; t0 < (int)Tb; t0 += kDecThreads) {
        const int t = t0 + tid;
        int best = -1;                                               // -1: past the utterance
        if (t < (int)Tb) {
            const float* p = xb + (long long)t * a.st;
            float m = p[0];
            best = 0;
            for (int c = 1; c < C; ++c) {
                const float v = p[(long long)c * a.sc];
                if (v > m) { m = v; best = c; }                      // strict: ties keep the lowest class
            }
        }
        if (lane == 63) wave_last[wave] = best;
        __syncthreads();                                             // wave_last and the previous chunk's last frame visible
        int prev = __shfl_up(best, 1);
        if (lane == 0) prev = wave == 0 ? last_of_chunk : wave_last[wave - 1];
        const bool emit = best >= 0 && best != a.blank && best != prev;
        const unsigned long long emask = __ballot(emit);
        if (lane == 0) wave_total[wave] = __popcll(emask);
        __syncthreads();
        int before = count, total = 0;
#pragma unroll
        for (int w = 0; w < kDecThreads / 64; ++w) {
            const int n = wave_total[w];
            before += w < wave ? n : 0;
            total += n;
        }
        if (emit) {
            const int pos = before + __popcll(emask & ((1ull << lane) - 1ull));
            lab[pos] = best;
            if (frm) frm[pos] = t;
        }
        count += total;
        __syncthreads();                                             // wave_total, wave_last, last_of_chunk are rewritten
        if (tid == kDecThreads - 1) last_of_chunk = best;
    }
    for (int i = count + tid; i < T; i += kDecThreads) {
        lab[i] = 0;
        if (frm) frm[i] = 0;
    }
    if (tid == 0) a.lengths[b] = count;
}

// ------------------------------------------------------------------------------------------------------------------ beam

__device__ __forceinline__ float lse2(float p, float q) {
    const float m = fmaxf(p, q);
    if (m == -__builtin_huge_valf()) return m;
    return m + log1pf(expf(fminf(p, q) - m));
}

__device__ __forceinline__ unsigned long long prefix_hash(unsigned long long h, int c) {
    unsigned long long z = h ^ ((unsigned long long)(c + 1) * 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
constexpr unsigned long long kEmptyHash = 0x243F6A8885A308D3ull;

// larger is better: orderable score bits, then the complement of the candidate key (smaller key wins a tie); 0 = no candidate
__device__ __forceinline__ unsigned long long cand_key(float s, int ckey) {
    if (!(s > -__builtin_huge_valf())) return 0ull;                  // -inf and NaN: not a candidate
    const unsigned u = __float_as_uint(s);
    const unsigned ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)ord << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)ckey);
}

// LDS carve of ctc_beam_kernel (every piece a multiple of 16 bytes)
struct BeamLds {
    unsigned long long* key;            // [N]      candidate keys
    unsigned long long* h;              // [2][W]   prefix hash
    unsigned long long* hp;             // [2][W]   hash of the prefix without its last label
    float* ly;                          // [kDecChunk][C] staged frame log-probabilities
    float* lsef;                        // [kDecChunk]   log-normaliser of logits frames
    float* clb;                         // [N]      candidate log p_b
    float* clnb;                        // [N]      candidate log p_nb
    float* lb;                          // [2][W]
    float* lnb;                         // [2][W]
    int* len;                           // [2][W]   -1: slot empty
    int* last;                          // [2][W]
    int* node;                          // [2][W]   -1: the empty prefix
    int* mparent;                       // [W]      beam whose extension by last(w) is beam w, or -1
    int* merge_to;                      // [W][C]   beam an extension merges into, or -1
};

__host__ __device__ inline size_t beam_lds_bytes(int W, int C, BeamLds* L, char* base) {
    const int N = W * C;
    size_t off = 0;
    auto take = [&](size_t bytes) { char* p = base + off; off += (bytes + 15) / 16 * 16; return p; };
    char* p;
    p = take((size_t)N * 8);              if (L) L->key = reinterpret_cast<unsigned long long*>(p);
    p = take((size_t)2 * W * 8);          if (L) L->h = reinterpret_cast<unsigned long long*>(p);
    p = take((size_t)2 * W * 8);          if (L) L->hp = reinterpret_cast<unsigned long long*>(p);
    p = take((size_t)kDecChunk * C * 4);  if (L) L->ly = reinterpret_cast<float*>(p);
    p = take((size_t)kDecChunk * 4);      if (L) L->lsef = reinterpret_cast<float*>(p);
    p = take((size_t)N * 4);              if (L) L->clb = reinterpret_cast<float*>(p);
    p = take((size_t)N * 4);              if (L) L->clnb = reinterpret_cast<float*>(p);
    p = take((size_t)2 * W * 4);          if (L) L->lb = reinterpret_cast<float*>(p);
    p = take((size_t)2 * W * 4);          if (L) L->lnb = reinterpret_cast<float*>(p);
    p = take((size_t)2 * W * 4);          if (L) L->len = reinterpret_cast<int*>(p);
    p = take((size_t)2 * W * 4);          if (L) L->last = reinterpret_cast<int*>(p);
    p = take((size_t)2 * W * 4);          if (L) L->node = reinterpret_cast<int*>(p);
    p = take((size_t)W * 4);              if (L) L->mparent = reinterpret_cast<int*>(p);
    p = take((size_t)N * 4);              if (L) L->merge_to = reinterpret_cast<int*>(p);
    return off;
}

__global__ __launch_bounds__(kDecThreads) void ctc_beam_kernel(const DecodeArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    BeamLds L;
    beam_lds_bytes(a.W, a.C, &L, smem);
    const int b = blockIdx.x, tid = threadIdx.x;
    const int C = a.C, T = a.T, W = a.W, N = W * C, blank = a.blank;
    long long Tb = a.input_len ? a.input_len[b] : T;
    const bool bad = Tb < 0 || Tb > T || blank < 0 || blank >= C;
    if (bad) Tb = 0;

    for (int i = tid; i < N; i += kDecThreads) L.merge_to[i] = -1;
    for (int w = tid; w < W; w += kDecThreads) {
        L.len[w] = w == 0 ? 0 : -1; L.len[W + w] = -1;
        L.lb[w] = w == 0 ? 0.0f : -__builtin_huge_valf(); L.lnb[w] = -__builtin_huge_valf();
        L.last[w] = -1; L.node[w] = -1; L.h[w] = kEmptyHash; L.hp[w] = 0ull;
    }
    const float* xb = a.x + (long long)b * a.sb;
    int2* pool = a.nodes + (long long)b * T * W;
    double offset = 0.0;                                             // log-scale of the stored scores (same in every thread)
    __syncthreads();

    for (int t = 0; t < (int)Tb; ++t) {
        const int kc = t % kDecChunk;
        if (kc == 0) {
            // stage frames t .. t+chunk-1 as log-probabilities ly[kk][c]
            for (int i = tid; i < C * kDecChunk; i += kDecThreads) {
                const int c = i / kDecChunk, kk = i - c * kDecChunk;
                float v = 0.0f;
                if (t + kk < (int)Tb) {
                    v = xb[(long long)c * a.sc + (long long)(t + kk) * a.st];
                    if (a.kind == 1) v = logf(v);
                }
                L.ly[kk * C + c] = v;
            }
            __syncthreads();
            if (tid < kDecChunk) {
                float z = 0.0f;
                if (a.kind == 0) {                                   // log-softmax of logits, as the loss does
                    const float* r = L.ly + tid * C;
                    float m = r[0];
                    for (int c = 1; c < C; ++c) m = fmaxf(m, r[c]);
                    float s = 0.0f;
                    for (int c = 0; c < C; ++c) s += expf(r[c] - m);
                    z = m + logf(s);
                }
                L.lsef[tid] = z;
            }
        }
        const int cur = (t & 1) * W, nxt = W - cur;
        // ---- 1. merge map; empty the next buffer
        {
            const int w2 = tid >> 2, part = tid & 3;                 // 4 lanes search for the parent of beam w2
            int found = -1;
            if (w2 < W) {
                const int l2 = L.len[cur + w2];
                if (l2 >= 1) {
                    const unsigned long long hp2 = L.hp[cur + w2];
                    for (int w = part; w < W; w += 4)
                        if (L.len[cur + w] == l2 - 1 && L.h[cur + w] == hp2) found = w;
                }
            }
            found = max(found, __shfl_xor(found, 1));
            found = max(found, __shfl_xor(found, 2));
            if (w2 < W && part == 0) {
                L.mparent[w2] = found;
                if (found >= 0) L.merge_to[found * C + L.last[cur + w2]] = w2;
                L.len[nxt + w2] = -1;
            }
        }
        __syncthreads();
        // ---- 2. candidates, relative to the best beam of the previous step (slot 0)
        const float best0 = L.len[cur] >= 0 ? lse2(L.lb[cur], L.lnb[cur]) : 0.0f;   // slot 0 empty: all are
        offset += (double)best0;
        const float* y = L.ly + kc * C;
        const float lz = L.lsef[kc];
        for (int i = tid; i < N; i += kDecThreads) {
            const int w = i / C, c = i - w * C;
            float cb = -__builtin_huge_valf(), cnb = -__builtin_huge_valf();
            int ckey = 0;
            const int lw = L.len[cur + w];
            if (lw >= 0) {
                const float pb = L.lb[cur + w] - best0, pnb = L.lnb[cur + w] - best0;
                const int lastw = L.last[cur + w];
                if (c == blank) {                                    // stay: blank, repeat of the last label, merged extension
                    cb = lse2(pb, pnb) + (y[blank] - lz);
                    if (lw > 0) cnb = pnb + (y[lastw] - lz);
                    ckey = w * 65;
                    const int wp = L.mparent[w];
                    if (wp >= 0) {
                        const float qb = L.lb[cur + wp] - best0, qnb = L.lnb[cur + wp] - best0;
                        const float e = (lastw == L.last[cur + wp] ? qb : lse2(qb, qnb)) + (y[lastw] - lz);
                        cnb = lse2(cnb, e);
                        if (wp < w) ckey = wp * 65 + 1 + lastw;
                    }
                } else if (L.merge_to[w * C + c] < 0) {              // extension l + c (a merged one is counted in the stay)
                    cnb = (c == lastw ? pb : lse2(pb, pnb)) + (y[c] - lz);
                    ckey = w * 65 + 1 + c;
                }
            }
            L.clb[i] = cb; L.clnb[i] = cnb;
            L.key[i] = cand_key(lse2(cb, cnb), ckey);
        }
        __syncthreads();
        // ---- 3. keep the W largest keys, each in the slot of its rank
        for (int i = tid; i < N; i += kDecThreads) {
            const unsigned long long k = L.key[i];
            int rank = k ? 0 : W;
            for (int j0 = 0; j0 < N; j0 += 64) {
                if (__all(rank >= W)) break;                          // no lane of this wave can still be kept
                const int j1 = min(j0 + 64, N);
#pragma unroll 16
                for (int j = j0; j < j1; ++j) rank += L.key[j] > k ? 1 : 0;   // independent broadcast reads: keep many in flight
            }
            if (rank < W) {
                const int w = i / C, c = i - w * C, s = nxt + rank;
                const unsigned ckey = 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull);
                const int pw = (int)(ckey / 65u), sub = (int)(ckey - (unsigned)pw * 65u);
                L.lb[s] = L.clb[i]; L.lnb[s] = L.clnb[i];
                if (c == blank) {                                    // the prefix of beam w
                    L.len[s] = L.len[cur + w]; L.last[s] = L.last[cur + w];
                    L.h[s] = L.h[cur + w]; L.hp[s] = L.hp[cur + w];
                } else {
                    L.len[s] = L.len[cur + w] + 1; L.last[s] = c;
                    L.h[s] = prefix_hash(L.h[cur + w], c); L.hp[s] = L.h[cur + w];
                }
                if (sub == 0) {
                    L.node[s] = L.node[cur + w];
                } else {                                             // created by an extension of beam pw: a new node
                    const int lbl = sub - 1;
                    pool[(long long)t * W + rank] = make_int2(L.node[cur + pw], (t << 7) | lbl);
                    L.node[s] = t * W + rank;
                }
            }
        }
        for (int w = tid; w < W; w += kDecThreads) {
            const int wp = L.mparent[w];
            if (wp >= 0) L.merge_to[wp * C + L.last[cur + w]] = -1;
        }
        __syncthreads();
    }
    const int fin = ((int)Tb & 1) * W;
    for (int w = tid; w < W; w += kDecThreads) {
        const long long o = (long long)b * W + w;
        const int lw = L.len[fin + w];
        float sc = -__builtin_huge_valf();
        if (bad) sc = __builtin_nanf("");
        else if (lw >= 0) sc = (float)(offset + (double)lse2(L.lb[fin + w], L.lnb[fin + w]));
        a.scores[o] = sc;
        a.lengths[o] = lw > 0 ? lw : 0;
        a.final_node[o] = lw > 0 ? L.node[fin + w] : -1;
    }
    if (bad && tid == 0 && a.bad) atomicAdd(a.bad, 1);
}

__global__ __launch_bounds__(64) void ctc_beam_walk_kernel(const DecodeArgs a) {
    const int w = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int T = a.T, W = a.W;
    const long long o = (long long)b * W + w;
    const int n = a.lengths[o];
    int* lab = a.labels + o * T;
    int* frm = a.frames ? a.frames + o * T : nullptr;
    if (lane == 0) {
        const int2* pool = a.nodes + (long long)b * T * W;
        int nd = a.final_node[o];
        for (int i = n - 1; i >= 0; --i) {
            const int2 e = pool[nd];
            lab[i] = e.y & 127;
            if (frm) frm[i] = e.y >> 7;
            nd = e.x;
        }
    }
    for (int i = n + lane; i < T; i += 64) {
        lab[i] = 0;
        if (frm) frm[i] = 0;
    }
}

}  // namespace wn

using namespace wn;

static int check_decode(int batch, int classes, int length) {
    if (batch <= 0 || classes <= 1 || length <= 0) return WN_ERR_BAD_SHAPE;
    if (classes > kDecMaxClasses || length > kDecMaxLength || batch > 65535) return WN_ERR_UNSUPPORTED;
    return WN_OK;
}

static int check_beam(int batch, int classes, int length, int beam_width) {
    const int rc = check_decode(batch, classes, length);
    if (rc != WN_OK) return rc;
    if (beam_width <= 0) return WN_ERR_BAD_SHAPE;
    if (beam_width > kDecMaxBeam) return WN_ERR_UNSUPPORTED;
    return WN_OK;
}

// workspace: node pool [B][T][W] int2, then the final node of every beam [B][W] int
static size_t beam_nodes_bytes(int batch, int length, int beam_width) {
    return ((size_t)batch * (size_t)length * (size_t)beam_width * 8 + 15) / 16 * 16;
}

size_t wn_ctc_decode_workspace_bytes(int batch, int classes, int length, int beam_width) {
    if (check_beam(batch, classes, length, beam_width) != WN_OK) return 0;
    return beam_nodes_bytes(batch, length, beam_width) + ((size_t)batch * (size_t)beam_width * 4 + 15) / 16 * 16;
}

int wn_ctc_greedy_decode(const float* x, long long sb, long long sc, long long st, const long long* input_lengths, int batch,
                         int classes, int length, int blank, int* labels, int* frames, int* lengths, int* bad,
                         wn_stream_t stream) {
    const int rc = check_decode(batch, classes, length);
    if (rc != WN_OK) return rc;
    if (!x || !labels || !lengths) return WN_ERR_NULL;
    DecodeArgs a = {};
    a.x = x; a.sb = sb; a.sc = sc; a.st = st; a.input_len = input_lengths;
    a.labels = labels; a.frames = frames; a.lengths = lengths; a.bad = bad;
    a.B = batch; a.C = classes; a.T = length; a.W = 1; a.blank = blank;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ctc_greedy_kernel, dim3(batch), dim3(kDecThreads), 0, s, a);
    WN_HIP(hipGetLastError(), "ctc_greedy");
    return WN_OK;
}

int wn_ctc_beam_decode(const float* x, long long sb, long long sc, long long st, int input_kind,
                       const long long* input_lengths, int batch, int classes, int length, int blank, int beam_width,
                       int* labels, int* frames, int* lengths, float* scores, void* workspace, size_t workspace_bytes,
                       int* bad, wn_stream_t stream) {
    const int rc = check_beam(batch, classes, length, beam_width);
    if (rc != WN_OK) return rc;
    if (input_kind < 0 || input_kind > 2) return WN_ERR_BAD_SHAPE;
    if (!x || !labels || !lengths || !scores || !workspace) return WN_ERR_NULL;
    if (workspace_bytes < wn_ctc_decode_workspace_bytes(batch, classes, length, beam_width)) return WN_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return WN_ERR_WORKSPACE;
    DecodeArgs a = {};
    a.x = x; a.sb = sb; a.sc = sc; a.st = st; a.input_len = input_lengths;
    a.labels = labels; a.frames = frames; a.lengths = lengths; a.scores = scores; a.bad = bad;
    a.nodes = reinterpret_cast<int2*>(workspace);
    a.final_node = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + beam_nodes_bytes(batch, length, beam_width));
    a.B = batch; a.C = classes; a.T = length; a.W = beam_width; a.blank = blank; a.kind = input_kind;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = beam_lds_bytes(beam_width, classes, nullptr, nullptr);
    WN_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(ctc_beam_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
           "ctc_beam attribute");
    hipLaunchKernelGGL(ctc_beam_kernel, dim3(batch), dim3(kDecThreads), lds, s, a);
    WN_HIP(hipGetLastError(), "ctc_beam");
    hipLaunchKernelGGL(ctc_beam_walk_kernel, dim3(beam_width, batch), dim3(64), 0, s, a);
    WN_HIP(hipGetLastError(), "ctc_beam_walk");
    return WN_OK;
}
