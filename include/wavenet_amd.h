/*
 * wavenet_amd.h -- C ABI of libwavenet_amd.so: the MI355X (gfx950) implementation of the
 * WaveNet dilated residual-block hot path of paultsw/wavenet-speech.
 *
 * The reference has no FFI layer (it is pure Python on stock PyTorch ops); the
 * boundary it exposes for this path is the nn.Module surface
 *     modules/conv_ops.py:8-79   CausalConv1d / NonCausalConv1d
 *     modules/block.py:15-82     ResidualBlock(in,out,k,d,causal).forward(seq) -> (residual_out, skip_out)
 *     modules/wavenet.py:98-100  the per-layer loop  out,skip = convolutions[l](out); skips_sum += bottlenecks[l](skip)
 * Each entry point below names the reference code it replaces.  The Python host side
 * (wavenet_speech_amd/) binds these with ctypes and re-creates that nn.Module surface on top.
 *
 * Conventions
 *  - plain C: raw DEVICE pointers, ints, a stream handle (hipStream_t passed as void*).  No torch types.
 *  - the library never allocates or frees device memory and keeps no device state: every buffer
 *    (activations, packed weights, saved tensors, workspaces) is owned by the caller.  Host-side state it does keep:
 *    the measurement hooks' event lists (wn_prof_*, off by default, process-wide behind a mutex) and the text of the last
 *    HIP error per thread (wn_last_hip_error).
 *  - every function only enqueues work on `stream` and returns 0 or a negative wn_status code;
 *    no exceptions cross the ABI.  wn_strerror() gives the text.
 *  - re-entrant; one process per GPU for data parallelism.
 *  - dtype: the wn_block_* / wn_conv_* / wn_skipsum_* entry points are fp32 storage and fp32 arithmetic
 *    (v_mfma_f32_32x32x2_f32, exact fp32 fma chains); the wn_h* entry points further down are the half-precision-MFMA modes
 *    (wn_precision: f16x3 = two fp16 planes per operand and three products, f16, bf16; fp32 accumulation, their own
 *    "half series" layout).
 *
 * Padded series layout (all activation tensors -- "series" of B utterances x C channels x L steps)
 *    float buf[B][Cp][ld],  Cp = wn_round_up(C, 8),  ld = halo + wn_round_up(L,128) + halo
 *    sample (b, c, t) lives at buf[(b*Cp + c)*ld + halo + t];   halo = wn_round_up(max |tap offset|, 4)
 *    EVERYTHING outside the valid [C][L] window (pad rows, both halos, the tail up to the next
 *    multiple of 128) MUST be zero on input and is kept zero on output.  This is what lets the
 *    kernels read the dilated taps x[t-d] with unmasked, time-coalesced 16-byte loads.
 *    wn_series_layout() computes (ld, halo, Cp) so host code never hard-codes the rule.
 */
#ifndef WAVENET_AMD_H
#define WAVENET_AMD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WN_VERSION 300 /* 0.3.0: round-3 entry points (fused forward, block-group weight gradients, pack tables, series convs, front-ends) */

typedef void* wn_stream_t; /* hipStream_t */

typedef enum wn_status {
    WN_OK = 0,
    WN_ERR_BAD_SHAPE = -1,   /* non-positive / inconsistent dimension, or layout (ld, halo) too small for the taps */
    WN_ERR_UNSUPPORTED = -2, /* kernel_width > WN_MAX_TAPS, channels > WN_MAX_CHANNELS, or channels*ld*4 >= 2^32 */
    WN_ERR_NULL = -3,        /* a required pointer is NULL */
    WN_ERR_HIP = -4,         /* a HIP runtime call or kernel launch failed (see wn_last_hip_error) */
    WN_ERR_WORKSPACE = -5    /* workspace smaller than wn_*_workspace_bytes(), or not 16-byte aligned */
} wn_status;

#define WN_MAX_TAPS 8
#define WN_MAX_CHANNELS 1024

/* Shape of one residual block call.  Mirrors ResidualBlock.__init__ (modules/block.py:22-51)
 * plus the batch geometry.  `skip_rows` is the row count of the skip projection: Co for the
 * stand-alone block (conv1x1_skip), or out_dim when the host has folded the stack's bottleneck
 * 1x1 into it (W = bottleneck.W @ conv1x1_skip.W, modules/wavenet.py:99-100). */
typedef struct wn_block_shape {
    int batch;        /* B */
    int length;       /* L, valid time steps */
    int in_channels;  /* Ci */
    int out_channels; /* Co */
    int skip_rows;    /* Ms */
    int kernel_width; /* k  (1..WN_MAX_TAPS) */
    int dilation;     /* d */
    int causal;       /* 1: CausalConv1d taps (j-(k-1))*d ; 0: NonCausalConv1d taps j*d - autopad(k,d) */
    int ld;           /* row pitch of every series buffer, floats */
    int halo;         /* zero columns before t=0 (and after the 128-rounded tail) */
} wn_block_shape;

/* The ten parameter tensors of a ResidualBlock in PyTorch's native layouts
 * (state_dict keys of modules/block.py:42-48).  Used for parameters and for their gradients. */
typedef struct wn_block_params {
    float* w_tanh;    /* conv_tanh.conv1d.weight     [Co][Ci][k] */
    float* b_tanh;    /* conv_tanh.conv1d.bias       [Co]        */
    float* w_sigmoid; /* conv_sigmoid.conv1d.weight  [Co][Ci][k] */
    float* b_sigmoid; /* conv_sigmoid.conv1d.bias    [Co]        */
    float* w_res;     /* conv1x1_residual.weight     [Co][Co](1) */
    float* b_res;     /* conv1x1_residual.bias       [Co]        */
    float* w_skip;    /* conv1x1_skip.weight         [Ms][Co](1)  (or the folded bottleneck*skip matrix) */
    float* b_skip;    /* conv1x1_skip.bias           [Ms]        */
    float* w_proj;    /* residual_proj.weight        [Co][Ci]    */
    float* b_proj;    /* residual_proj.bias          [Co]        */
} wn_block_params;

int wn_version(void);
const char* wn_strerror(int status);
/* text of the last HIP error seen by this thread's calls (empty string if none) */
const char* wn_last_hip_error(void);

int wn_round_up(int x, int multiple);
/* modules/conv_ops.py:104-116 autopad and the tap offsets of both conv flavours (off[j], j<k). */
int wn_autopad(int kernel_width, int dilation);
int wn_tap_offsets(int kernel_width, int dilation, int causal, int* off /* [k] */);
/* Padded series layout for L steps and taps reaching at most max_abs_offset columns away. */
int wn_series_layout(int length, int max_abs_offset, int* ld, int* halo);
/* floats in one series buffer of `channels` channels: B * round_up(C,8) * ld */
size_t wn_series_floats(int batch, int channels, int ld);

/* ---- weights: repack PyTorch-layout parameters into MFMA-fragment order -------------------
 * Once per optimizer step (weights are constant across the batch).  `packed` must hold
 * wn_block_packed_bytes() bytes; it is consumed by wn_block_forward / wn_block_backward_data. */
size_t wn_block_packed_bytes(const wn_block_shape* s);
int wn_block_pack(const wn_block_shape* s, const wn_block_params* p, void* packed, wn_stream_t stream);

/* ---- forward: replaces ResidualBlock.forward (modules/block.py:54-82) ----------------------
 *   a = conv_tanh(x), g = conv_sigmoid(x); ta = tanh(a), sg = sigmoid(g); z = ta*sg
 *   r    = W_res z + b_res + W_proj x + b_proj                       -> r_out (may be NULL: not needed)
 *   skip = W_skip z + b_skip                                         -> skip  (skip_accumulate=0)
 *   skip += W_skip z + b_skip   (the stack's running skips_sum)       -> skip  (skip_accumulate=1)
 *   skip == NULL: the skip product is left to wn_skipsum_forward (below)
 *   z (always written) and sg (may be NULL for inference) are what the backward pass needs: the tanh is recovered as z / sg
 *   there, which saves one tensor per block in the forward launch's stores and in the state held until backward.
 * x: [B][Ci8][ld]; r_out, sg, z: [B][Co8][ld]; skip: [B][Ms8][ld]. */
int wn_block_forward(const wn_block_shape* s, const void* packed, const float* x,
                     float* r_out, float* skip, int skip_accumulate,
                     float* sg, float* z, wn_stream_t stream);

/* ---- skips_sum of a whole stack as ONE long-K product (training, where every block's z is kept anyway) ----
 *   skip (+)= sum_l W_skip_l z_l + bias_total        == the sum over l of modules/wavenet.py:100
 * Call wn_block_forward with skip == NULL for each block (it then skips the per-block accumulation) and this once
 * per group of <= WN_MAX_STACK_GROUP blocks: K = sum_l C_l amortises the per-wave costs that dominate the per-block
 * K = C_l product and removes 2 HBM passes over skips_sum per block.
 * w_skip / z are HOST arrays of nblocks DEVICE pointers ([Ms][C_l] matrices and [B][C_l 8][ld] series). */
#define WN_MAX_STACK_GROUP 32
typedef struct wn_skipsum_shape {
    int batch, length, skip_rows, nblocks, ld, halo;
    int channels[WN_MAX_STACK_GROUP]; /* C_l */
} wn_skipsum_shape;
size_t wn_skipsum_packed_bytes(const wn_skipsum_shape* s);
int wn_skipsum_pack(const wn_skipsum_shape* s, const float* const* w_skip, const float* bias_total /* [Ms] or NULL */,
                    void* packed, wn_stream_t stream);
int wn_skipsum_forward(const wn_skipsum_shape* s, const void* packed, const float* const* z, float* skip,
                       int accumulate, wn_stream_t stream);

/* ---- backward (data): what autograd computes through modules/block.py:54-82 ----------------
 *   dz = W_res^T dr + W_skip^T dskip ;  da = dz*sg*(1-ta^2) ;  dg = dz*ta*sg*(1-sg), ta = z/sg     -> da, dg
 *   dx[t] = W_proj^T dr[t] + sum_j (W_tanh_j^T da + W_sigmoid_j^T dg)[t - off_j]         -> dx (may be NULL)
 * dr may be NULL (residual output unused, e.g. the last block of the stack).
 * dr, da, dg: [B][Co8][ld]; dskip: [B][Ms8][ld]; dx: [B][Ci8][ld]. */
int wn_block_backward_data(const wn_block_shape* s, const void* packed,
                           const float* dr, const float* dskip, const float* z, const float* sg,
                           float* da, float* dg, float* dx, wn_stream_t stream);

/* ---- backward (weights): time/batch-summed outer products -> gradients in PyTorch layouts ---
 *   dW_tanh[:,:,j] = sum da[t] x[t+off_j]^T, dW_sigmoid likewise with dg, dW_res = sum dr z^T,
 *   dW_proj = sum dr x^T, dW_skip = sum dskip z^T, biases = row sums.  Deterministic (split-K
 *   partial slabs reduced in a fixed order).  Gradients are OVERWRITTEN, not accumulated.
 *   dr may be NULL (no consumer of the residual output: the last block of a stack).  The four residual-path
 *   gradient pointers (w_res, b_res, w_proj, b_proj) may then be NULL too -- "no gradient", as autograd leaves
 *   them in the reference -- and any of them that is given is written as zeros. */
size_t wn_block_wgrad_workspace_bytes(const wn_block_shape* s);
int wn_block_backward_weights(const wn_block_shape* s, const float* x, const float* z,
                              const float* da, const float* dg, const float* dr, const float* dskip,
                              const wn_block_params* grads, void* workspace, size_t workspace_bytes,
                              wn_stream_t stream);

/* ---- stand-alone dilated conv: CausalConv1d / NonCausalConv1d (modules/conv_ops.py:8-79) ---
 * and, with kernel_width=1, any 1x1 Conv1d.  y = sum_j W[:,:,j] x[t+off_j] + b. */
typedef struct wn_conv_shape {
    int batch, length, in_channels, out_channels, kernel_width, dilation, causal, ld, halo;
} wn_conv_shape;
size_t wn_conv_packed_bytes(const wn_conv_shape* s);
int wn_conv_pack(const wn_conv_shape* s, const float* weight /*[Co][Ci][k]*/, const float* bias /*[Co] or NULL*/,
                 void* packed, wn_stream_t stream);
int wn_conv_forward(const wn_conv_shape* s, const void* packed, const float* x, float* y, wn_stream_t stream);
int wn_conv_backward_data(const wn_conv_shape* s, const void* packed, const float* dy, float* dx, wn_stream_t stream);
size_t wn_conv_wgrad_workspace_bytes(const wn_conv_shape* s);
int wn_conv_backward_weights(const wn_conv_shape* s, const float* x, const float* dy,
                             float* dweight, float* dbias /* may be NULL */,
                             void* workspace, size_t workspace_bytes, wn_stream_t stream);

/* ---- next-sample NLL head: replaces the L-iteration CrossEntropyLoss loop of Loss.py:38-43 /
 * legacy_code/train.py:37-39.  logits: dense [B][C][L] floats; target: [B][L] int64 class indices.
 *   forward : lse = [2][B][L] floats, the two terms of logsumexp_c logits[b][c][t] kept apart: lse[0][b][t] = max_c logits,
 *             lse[1][b][t] = log sum_c exp(logits - max);  partial[i] = sum over workgroup i of ((max - logits[target]) + lse[1])
 *             (wn_nll_partials(B, L) floats; the caller sums them in order and divides by B: deterministic)
 *             A target outside [0, C) is never used as an index: it is counted in *bad_targets (one DEVICE int the caller
 *             zeroed; may be NULL) and makes its workgroup's partial NaN (torch asserts on the device in that case).
 *             A logit of -inf (a masked class) contributes nothing, whatever its position; a target on one gives a loss of +inf.
 *   backward: dlogits = (exp((logits - lse[0]) - lse[1]) - onehot(target)) * gscale[0]   (gscale: one DEVICE float, = dloss / B) */
size_t wn_nll_partials(int batch, int length);
int wn_nll_forward(const float* logits, const long long* target, float* lse, float* partial, int* bad_targets,
                   int batch, int classes, int length, wn_stream_t stream);
int wn_nll_backward(const float* logits, const long long* target, const float* lse, const float* gscale, float* dlogits,
                    int batch, int classes, int length, wn_stream_t stream);

/* ---- entry conv on quantised levels: replaces entry_conv1d(one_hot(levels)) of
 * modules/wavenet.py:54,93 + modules/fns.py:6-15 without materialising the [B][classes][L] one-hot.
 *   forward : y[b][co][t] = bias[co] + sum_j W[co][levels[b][t + j - (k-1)]][j]   (causal, dilation 1; y dense [B][Co][L])
 *   backward: no entry point of its own: dW[co][c][j] = sum over (b,t) with levels[b][t + j - (k-1)] == c of dy[b][co][t] is
 *             formed by wn_conv_backward_weights against a one-hot the caller builds for the duration of the backward call
 *             (the host mirror does; a gather-form kernel without it was measured 3.5x slower and removed in round 3).
 * levels: [B][L] int64 in [0, classes); anything else is counted in *bad_levels (DEVICE int, caller-zeroed, may be NULL)
 * and contributes nothing.  classes <= 512. */
int wn_embed_forward(const long long* levels, const float* weight, const float* bias, float* y, int batch, int length,
                     int classes, int out_channels, int kernel_width, int* bad_levels, wn_stream_t stream);
/* ---- synthetic reads on the device: the reference's on-line generator
 * utils/gaussian_kmer_model.py:53-104 (gaussian_model_fn :53-73, quantize_fn :79-86, one_hot_fn :89-97), float64 like its
 * numpy arithmetic.  All pointers are DEVICE pointers.
 *   wn_synth_bases     nucleotides 1..4 [B][nbases] int64 from a counter-based Philox4x32-10 stream of `seed`
 *   wn_synth_signal    picoamps[b][t] = means[k] + stdvs[k] * z,  k = 5-mer index of bases[b][p+2 .. p+6], p = t / upsampling
 *                      (scipy generic_filter's centred window after the [4:-4] trim: n bases give (n - 8) * upsampling
 *                      samples), z ~ N(0,1) from a second Philox stream of `seed`, or noise[b][t] when `noise` is not NULL
 *                      (the deterministic stages can then be checked against fixtures).  means / stdvs: 1024 doubles.
 *                      A base outside 1..4 is counted in *bad_bases (DEVICE int, caller-zeroed, may be NULL).
 *                      Also leaves per-tile (sum, min, max) partials in `workspace` for the next call.
 *   wn_synth_quantize  per read (x - mean) / (max - min), mu-law with mu = num_levels, np.digitize against `edges`
 *                      (num_levels ascending doubles: linspace(-1, 1, num_levels)); levels [B][L] int64 and, unless
 *                      one_hot is NULL, the dense one-hot [B][num_levels][L] fp32.  The per-read mean is a fixed-order sum:
 *                      results are bit-reproducible. */
size_t wn_synth_workspace_bytes(int batch, int length);
int wn_synth_bases(unsigned long long seed, int batch, int nbases, long long* bases, wn_stream_t stream);
int wn_synth_signal(const long long* bases, int batch, int nbases, int length, int upsampling, const double* means,
                    const double* stdvs, unsigned long long seed, const double* noise /* may be NULL */, double* picoamps,
                    void* workspace, size_t workspace_bytes, int* bad_bases /* may be NULL */, wn_stream_t stream);
int wn_synth_quantize(const double* picoamps, const void* workspace, size_t workspace_bytes, int batch, int length,
                      int num_levels, const double* edges, long long* levels, float* one_hot /* may be NULL */,
                      wn_stream_t stream);

/* ---- CTC on the device: replaces the warp-ctc call of Loss.py:49-53 (legacy_code/train.py:46,
 * pretrain_tnt.py:145,159, which copies the activations to the CPU every step).  warp-ctc semantics: softmax over the
 * classes inside the loss, one negative log likelihood per utterance (the caller sums them), and the gradient with respect
 * to the activations comes back with the loss.  Layout is the stack's own: logits / dlogits dense [B][C][T], time fastest --
 * nothing is permuted.  All pointers are DEVICE pointers.
 *   labels         [B][max_label_len] int64, utterance b uses the first label_lengths[b]; values in [0, C) and != blank
 *   label_lengths  [B] int64;  input_lengths [B] int64 or NULL (= every utterance has `length` frames)
 *   nll            [B] fp32: -log p(labels | logits); +inf when no alignment fits (its gradient rows are zero)
 *   dlogits        d nll[b] / d logits[b], or NULL for the loss alone
 * A label outside [0, C), equal to blank, or a length outside its range poisons that utterance (nll = NaN, zero gradient)
 * and is counted in *bad_labels (DEVICE int, caller-zeroed, may be NULL).  The recursions run in float64.
 * Limits: C <= 64, max_label_len <= 2047. */
size_t wn_ctc_workspace_bytes(int batch, int classes, int length, int max_label_len);
int wn_ctc_loss(const float* logits, const long long* labels, const long long* label_lengths,
                const long long* input_lengths /* may be NULL */, int batch, int classes, int length, int max_label_len,
                int blank, float* nll, float* dlogits /* may be NULL */, void* workspace, size_t workspace_bytes,
                int* bad_labels /* may be NULL */, wn_stream_t stream);

/* ---- CTC decoding on the device: replaces the tail of the reference's evaluation notebooks (argmax_decode + labels2strings,
 * modules/sequence_decoders.py, and ctcdecode's CTCBeamDecoder).  The input is read through element strides: element
 * (b, c, t) at x[b * sb + c * sc + t * st], so the stack's [B][C][T] (sb = C*T, sc = T, st = 1) and ctcdecode's (B, T, C)
 * (sb = T*C, sc = 1, st = C) are both read in place.  fp32.  All pointers are DEVICE pointers; input_lengths [B] int64 or
 * NULL (= every utterance has `length` frames).  An input length outside [0, length] or a blank outside [0, classes) makes
 * that utterance decode to nothing (beam scores NaN) and is counted in *bad (DEVICE int, caller-zeroed, may be NULL).
 *   greedy   argmax per frame (ties to the lowest class), repeats collapsed, blanks dropped:
 *            labels [B][length] int32 (zero-padded), frames [B][length] (frame of each label, may be NULL), lengths [B]
 *   beam     CTC prefix beam search, no language model, beam_width prefixes:  labels / frames [B][W][length] (frames may be
 *            NULL), lengths [B][W], scores [B][W] = natural log probability of the prefix summed over the alignments the
 *            search kept, sorted descending; slots past the distinct prefixes found: length 0, score -inf.
 *            input_kind: 0 logits (log-softmax over the classes inside), 1 probabilities, 2 log-probabilities.
 * Limits: classes <= 64, 1 <= beam_width <= 64, length <= 2^24 (WN_ERR_UNSUPPORTED, nothing launched).
 * wn_ctc_decode_workspace_bytes is 0 for a bad or unsupported shape. */
size_t wn_ctc_decode_workspace_bytes(int batch, int classes, int length, int beam_width);
int wn_ctc_greedy_decode(const float* x, long long sb, long long sc, long long st, const long long* input_lengths /* may be NULL */,
                         int batch, int classes, int length, int blank, int* labels, int* frames /* may be NULL */, int* lengths,
                         int* bad /* may be NULL */, wn_stream_t stream);
int wn_ctc_beam_decode(const float* x, long long sb, long long sc, long long st, int input_kind,
                       const long long* input_lengths /* may be NULL */, int batch, int classes, int length, int blank,
                       int beam_width, int* labels, int* frames /* may be NULL */, int* lengths, float* scores, void* workspace,
                       size_t workspace_bytes, int* bad /* may be NULL */, wn_stream_t stream);

/* ---- CTC forced alignment on the device: the best single alignment (Viterbi path) of a KNOWN label sequence to the frames --
 * which frames belong to which label -- where wn_ctc_loss sums over all alignments.  x, its element strides and input_kind as
 * in wn_ctc_beam_decode; labels [B][max_label_len] int64, label_lengths [B] int64, input_lengths [B] int64 or NULL as in
 * wn_ctc_loss.  With l' the blank-extended labelling (2 L + 1 states: even = blank, odd s = label (s - 1) / 2) a path starts in
 * state 0 or 1, ends in state S - 1 or S - 2 and moves by 0, +1, or +2 (only onto a label that differs from the label two
 * states back); its score is the sum of the frame log-probabilities of its states.  The recursion runs in float64.
 * Ties: predecessors are tried in the order s, s - 1, s - 2 and a later one wins only if strictly greater; the path ends in
 * S - 1 unless S - 2 scores strictly higher.
 *   states        [B][length] int32: the state of every frame t < input_lengths[b], -1 after
 *   frame_labels  [B][length] int32 or NULL: l' of that state (a label or the blank), -1 in the same places
 *   spans         [B][max_label_len][2] int32 or NULL: label j < label_lengths[b] occupies frames [first, one past last);
 *                 rows j >= label_lengths[b] are (-1, -1)
 *   score         [B] fp32: the path's log-probability
 * No alignment fits (fewer frames than labels + adjacent repeats, or every alignment has probability 0): score -inf, every
 * state / label / span entry -1.  No frames: score 0 for an empty label sequence, else -inf.  A label outside [0, classes),
 * equal to blank, or a length outside its range poisons the utterance as in wn_ctc_loss: score NaN, every entry -1, counted
 * in *bad (DEVICE int, caller-zeroed, may be NULL).
 * workspace: wn_ctc_align_workspace_bytes (2 bits per state and frame; 0 for a bad or unsupported shape), 16-byte aligned.
 * Limits: classes <= 64, 1 <= max_label_len <= 2047, length <= 2^24, batch <= 65535, batch * length < 2^31
 * (WN_ERR_UNSUPPORTED, nothing launched). */
size_t wn_ctc_align_workspace_bytes(int batch, int classes, int length, int max_label_len);
int wn_ctc_align(const float* x, long long sb, long long sc, long long st, int input_kind, const long long* labels,
                 const long long* label_lengths, const long long* input_lengths /* may be NULL */, int batch, int classes,
                 int length, int max_label_len, int blank, int* states, int* frame_labels /* may be NULL */,
                 int* spans /* may be NULL */, float* score, void* workspace, size_t workspace_bytes, int* bad /* may be NULL */,
                 wn_stream_t stream);

/* ---- Global pairwise alignment of two label sequences with affine gaps (Needleman-Wunsch / Gotoh, int32, exact): how close
 * a decoded read is to the truth -- what the reference's evaluation notebook asks EMBOSS needle.  ref [B] rows of ref_stride
 * elements (rows i = 1..N), query likewise (columns j = 1..M): int32 labels, compared for equality only (no class limit);
 * values past ref_lengths[b] / query_lengths[b] are never read.  A gap of length n costs gap_open + (n - 1) gap_extend.
 *   E[i][j] = max(H[i][j-1] - go, E[i][j-1] - ge),  F[i][j] = max(H[i-1][j] - go, F[i-1][j] - ge): opening wins a tie
 *   H[i][j] = diagonal + (match | mismatch), then E, then F: a later candidate replaces an earlier one only if strictly greater
 *   borders H[i][0], H[0][j]: 0 with end_gaps_free, else -(go + ge (k - 1)); H[0][0] = 0
 *   end cell (N, M); with end_gaps_free the best of (N, M), the last row from j = M down, the last column from i = N down,
 *   replaced only by a strictly greater one.  The trace runs back until i == 0 or j == 0; the unconsumed head and tail of
 *   either sequence are end gaps: they appear in ops and count in the gap columns and the length.
 *   score    [B] int32
 *   stats    [B][4] int32 or NULL: matches, mismatches, gap columns, alignment length
 *   ops      [B][max_ref_len + max_query_len] bytes or NULL, front to back: 1 match, 2 mismatch, 3 reference label against a
 *            gap, 4 query label against a gap, 0 padding;  ops_len [B] int32, required if and only if ops is given
 * ops == NULL and stats == NULL is the score-only form: no workspace (with costs 0, -1, 1, 1 and end gaps penalised,
 * -score is the Levenshtein distance).  A length that is negative or above its maximum poisons the pair: score INT_MIN, stats
 * -1, ops_len 0, counted in *bad (DEVICE int, caller-zeroed, may be NULL).  Length 0 is valid: all end gaps.
 * workspace: wn_pair_align_workspace_bytes (0 for a bad or unsupported shape), 16-byte aligned.
 * Limits: max_query_len <= 8192, max_ref_len <= 65535, batch <= 65535, 0 <= gap_extend <= gap_open <= 1024,
 * |match|, |mismatch| <= 1024 (WN_ERR_UNSUPPORTED, nothing launched). */
size_t wn_pair_align_workspace_bytes(int batch, int max_ref_len, int max_query_len);
int wn_pair_align(const int* ref, long long ref_stride, const int* ref_lengths, const int* query, long long query_stride,
                  const int* query_lengths, int batch, int max_ref_len, int max_query_len, int match, int mismatch,
                  int gap_open, int gap_extend, int end_gaps_free, int* score, int* stats /* may be NULL */,
                  unsigned char* ops /* may be NULL */, int* ops_len /* with ops */, void* workspace, size_t workspace_bytes,
                  int* bad /* may be NULL */, wn_stream_t stream);

/* ---- Ragged synthetic reads on the device: the data of the reference's RawCTCNet workloads (RawGaussianModelLoader with
 * random_upsample=True, utils/gaussian_kmer_model.py:181-319; RawSignalGenerator, utils/raw_signal_generator.py): reads of random
 * length, every 5-mer held for a random number of samples (its dwell), raw fp32 picoamps zero-padded to a common row length,
 * the bases as CTC targets.  Two launches; all pointers are DEVICE pointers; rows of bases / dwell / starts are max_bases ints.
 * Random numbers are Philox4x32-10 of `seed`: stream 2 counter b for a length, stream 0 counter (b << 32) | i for a base,
 * stream 3 counter (b << 32) | p for a dwell, stream 1 counter (b << 32) | t for a sample's noise -- read b's draws depend on
 * (seed, b) only, not on the batch.
 *   wn_reads_plan, one workgroup per read:
 *     base_lengths[b]  uniform in [min_bases, max_bases), or base_lengths_in[b]; a given length outside [5 + 2 window, max_bases)
 *                      poisons the read
 *     bases[b][i]      1..4 for i < base_lengths[b], 0 after (the reference's batchify), or bases_in (a value outside 1..4
 *                      inside the length poisons the read)
 *     window           2: the loader's [4:-4] trim, k-mer p = bases[p+2 .. p+6];  0: RawSignalGenerator's [2:-2], k-mer p =
 *                      bases[p .. p+4].  K_b = base_lengths[b] - 4 - 2 window k-mers
 *     dwell[b][p] >= 1 for p < K_b, 0 after.  WN_DWELL_FIXED: p0.  WN_DWELL_UNIFORM (r = p0, w = p1): an integer in
 *                      [max(r - w, 1), r + w) by multiply-high of one 32-bit word (bias <= range / 2^32 per value).
 *                      WN_DWELL_GAMMA (shape p0, rate p1, sample rate p2): max(1, (int)(g * p2)), g ~ Gamma(shape, scale 1 / rate)
 *                      by Marsaglia-Tsang with Box-Muller normals (shape < 1 through Gamma(shape + 1) U^(1 / shape)); the
 *                      rejection loop is bounded at 16 attempts (sub-counter = attempt), all of them failing has probability
 *                      < 1e-21 and then g = max(shape, shape + 1 below 1) / rate with U = 1/2.  Or dwell_in (an entry < 1 below
 *                      K_b poisons the read).  Values above max_dwell are clamped to it and counted in *clamped.
 *     starts[b][p]     exclusive prefix sum of the dwell for p <= K_b; = signal_lengths[b] for every p >= K_b
 *     signal_lengths[b] = starts[b][K_b]
 *     A poisoned read has base length 0, signal length 0, bases / dwell / starts all 0 and is counted in *bad; its given
 *     values are never used as an index.  workspace (wn_reads_workspace_bytes, 16-byte aligned) receives the 5-mer index of
 *     every k-mer for wn_reads_signal.
 *   wn_reads_signal, grid (ceil(ld / 256), batch); ld = the caller's row capacity of signal / sample_kmer / noise:
 *     signal[b][t]     (float)(means[k] + stdvs[k] * z) evaluated in float64, t < signal_lengths[b]; k = 5-mer index of the k-mer
 *                      p with starts[b][p] <= t < starts[b][p + 1]; z ~ N(0, 1) by Box-Muller, or noise[b][t].  means / stdvs:
 *                      1024 doubles.  0.0f for signal_lengths[b] <= t < ld
 *     sample_kmer[b][t] p, -1 past the read (may be NULL).  Every element of both rows is written.
 *     A read longer than ld is truncated at ld and counted in *bad; clipped_lengths[b] = min(signal_lengths[b], ld).
 * bad / clamped: DEVICE ints, caller-zeroed, may be NULL.
 * Checked before any launch, in this order.  WN_ERR_BAD_SHAPE: batch, max_bases, ld < 1; window not 0 or 2; min_bases outside
 * [5 + 2 window, max_bases); max_dwell < 1; an unknown dwell model, r < 1, an empty uniform interval, shape / rate / sample
 * rate not positive and finite.  WN_ERR_UNSUPPORTED: batch > 65535, max_bases > 65536, (max_bases - 5) max_dwell >= 2^31,
 * ld > 2^31 - 257.  Then WN_ERR_NULL, then WN_ERR_WORKSPACE. */
enum { WN_DWELL_FIXED = 0, WN_DWELL_UNIFORM = 1, WN_DWELL_GAMMA = 2 };
size_t wn_reads_workspace_bytes(int batch, int max_bases);
int wn_reads_plan(unsigned long long seed, int batch, int min_bases, int max_bases, int window, int dwell_model, double dwell_p0,
                  double dwell_p1, double dwell_p2, int max_dwell, const int* base_lengths_in /* may be NULL */,
                  const int* bases_in /* may be NULL */, const int* dwell_in /* may be NULL */, int* base_lengths, int* bases,
                  int* dwell, int* starts, int* signal_lengths, void* workspace, size_t workspace_bytes,
                  int* bad /* may be NULL */, int* clamped /* may be NULL */, wn_stream_t stream);
int wn_reads_signal(const int* base_lengths, const int* starts, const int* signal_lengths, const void* workspace,
                    size_t workspace_bytes, int batch, int max_bases, int window, int ld, const double* means,
                    const double* stdvs, unsigned long long seed, const double* noise /* may be NULL */, float* signal,
                    int* sample_kmer /* may be NULL */, int* clipped_lengths /* may be NULL */, int* bad /* may be NULL */,
                    wn_stream_t stream);

/* ---- Chunked whole-read inference (wavenet_speech_amd/basecalling.py): a read of any length is cut into chunks of `chunk`
 * samples overlapping by the network's receptive field, all chunks run through ONE fixed-shape forward, and every chunk keeps
 * only the frames whose receptive field lay inside it.  These are the two streaming launches around that forward.  All
 * pointers are DEVICE pointers.  The plan is made on the host, five ints per chunk:
 *     plan[n] = (read, s0, u_lo, t0, count)   chunk n holds samples [s0, s0 + chunk) of `read`; its frames [u_lo, u_lo + count)
 *                                             are frames [t0, t0 + count) of that read.  count = 0 marks a dead chunk (padding
 *                                             of a micro-batch): its other fields are not looked at.
 *   wn_chunk_gather, grid (ceil(chunk / 1024), n_chunks), 4 consecutive samples per thread, one 16-byte store each:
 *     signal           [batch][ld] fp32, or int16 DAC counts when signal_is_int16 != 0; signal_lengths[b] <= ld samples are valid
 *     out[n][i]        x_b[s0 + i] for s0 + i < signal_lengths[b], 0.0f otherwise and in every dead chunk; [n_chunks][chunk]
 *                      fp32, 16-byte aligned.  x_b[s] = (float(signal[b][s]) + shift[b]) * scale[b], two separately rounded
 *                      fp32 operations (never an FMA); scale / shift: [batch] fp32, each may be NULL (then left out)
 *     A live row with read outside [0, batch), s0 outside [0, ld), count < 0, or a length outside [0, ld] is counted in *bad
 *     and written as zeros; none of these values is used as an index.
 *   wn_chunk_stitch, grid (ceil(y_frames / 256), classes, n_chunks), one element per thread:
 *     y                [n_chunks][classes][y_frames] fp32 through its element strides (stride_n, stride_c, stride_t >= 0)
 *     out[b][c][t0 + i] = y[n][c][u_lo + i] for i < count; out: [batch][classes][out_frames] fp32 through out_stride_b /
 *                      out_stride_c (unit stride in time), zero-filled by the caller
 *     A live row with read outside [0, batch), a negative field, u_lo + count > y_frames, t0 + count > frame_lengths[b] or
 *     frame_lengths[b] > out_frames is counted in *bad and skipped.
 * bad: a DEVICE int, caller-zeroed, may be NULL.
 * Checked before any launch, in this order.  WN_ERR_BAD_SHAPE: a dimension < 1, chunk % 4 != 0, a negative stride.
 * WN_ERR_UNSUPPORTED: n_chunks > 65535, classes > 65535, ld / chunk / y_frames / out_frames >= 2^31 - 1024, or a grid of 2^32
 * threads or more (256 ceil(chunk / 1024) n_chunks; 256 ceil(y_frames / 256) classes n_chunks): longer plans go in several calls.
 * ld is both the row stride and the row capacity: lengths up to ld are accepted, so rows must be dense.  Then WN_ERR_NULL, then WN_ERR_WORKSPACE for an `out` of wn_chunk_gather that is not 16-byte aligned. */
int wn_chunk_gather(const void* signal, int signal_is_int16, int batch, int ld, const int* signal_lengths,
                    const float* scale /* may be NULL */, const float* shift /* may be NULL */, const int* plan, int n_chunks,
                    int chunk, float* out, int* bad /* may be NULL */, wn_stream_t stream);
int wn_chunk_stitch(const float* y, long long stride_n, long long stride_c, long long stride_t, int y_frames, const int* plan,
                    int n_chunks, int classes, int batch, float* out, long long out_stride_b, long long out_stride_c,
                    int out_frames, const int* frame_lengths, int* bad /* may be NULL */, wn_stream_t stream);

/* ---- Read normalisation (wavenet_speech_amd/normalise.py): exact order statistics of ragged reads, from which the median, the
 * MAD and quantiles give the (scale, shift) of wn_chunk_gather.  All pointers but the workspace size are DEVICE pointers.
 *     out[b][k] = the ranks[b][k]-th smallest (0-based) of the first signal_lengths[b] samples of read b, as fp32
 *   signal           [batch][ld] fp32, or int16 with signal_is_int16 != 0; ld is both the row stride and the row capacity
 *   ranks            [batch][K] int32, 1 <= K <= 8
 *   center           [batch] fp32 or NULL.  Given, the elements are the absolute deviations d = |(float)x - center[b]| (one
 *                    correctly rounded fp32 subtraction), and out holds the ranks[b][k]-th smallest deviation
 *   out              [batch][K] fp32: the element itself (x or d), never a value rebuilt from counts
 * A most-significant-digit radix select, 8 bits per pass, over an order-preserving unsigned key: int16 (uint16)x ^ 0x8000, two
 * passes; fp32 u ^ (sign ? 0xFFFFFFFF : 0x80000000), u the bits of x, four passes; with center the bits of d, four passes.
 * Integer histograms only: exact, and bitwise the same from run to run.  -0.0 sorts directly below +0.0 (either may come
 * back; they compare equal); a NaN with its sign bit clear sorts above +inf, one with it set below -inf.  One memset, one
 * launch per pass, grid (ceil(ld / 8192), batch), and one small closing launch: the count depends on the dtype and on center
 * only, nothing is read back, the call can be captured into a HIP graph.
 * Checked on the device: a read with signal_lengths[b] < 0 or > ld, and a rank outside [0, signal_lengths[b]) (every rank of
 * an empty read), write 0.0f to their out[b][k] and count once each in *bad (DEVICE int, caller-zeroed, may be NULL); no
 * sample at or past a length is read.
 * workspace: wn_read_select_workspace_bytes(batch, K, signal_is_int16, has_center) bytes, 16-byte aligned, zeroed by the call
 * itself on the stream; 0 for an unsupported shape (batch or K out of range).
 * Checked before any launch, in this order.  WN_ERR_BAD_SHAPE: batch, ld or K < 1.  WN_ERR_UNSUPPORTED: K > 8, batch > 65535,
 * ld >= 2^31 - 1024, or a grid of 2^32 threads or more (256 ceil(ld / 8192) batch).  Then WN_ERR_NULL (center and bad are
 * optional), then WN_ERR_WORKSPACE: a workspace that is too small or not 16-byte aligned, or a signal not aligned to its
 * element size. */
size_t wn_read_select_workspace_bytes(int batch, int K, int signal_is_int16, int has_center);
int wn_read_select(const void* signal, int signal_is_int16, int batch, int ld, const int* signal_lengths, const int* ranks, int K,
                   const float* center /* may be NULL */, float* out, void* workspace, size_t workspace_bytes,
                   int* bad /* may be NULL */, wn_stream_t stream);

/* ---- Per-base quality of a decoded read (wavenet_speech_amd.decoding.ctc_base_qualities): how much to
 * trust each label a decoder emitted when the truth is not known -- a Phred quality per base, a mean error per read.  x, its
 * element strides, input_kind and input_lengths as in wn_ctc_beam_decode.  labels / frames: int32 rows of labels_stride /
 * frames_stride elements (>= 0), max_labels of them used -- the outputs of wn_ctc_greedy_decode, or one beam of
 * wn_ctc_beam_decode in place; lengths [B] int32.  All pointers are DEVICE pointers.  For utterance b with T_b frames:
 *     w_t(c)    expf(x_t(c) - max_c x_t(c)) for logits and log-probabilities, x_t(c) for probabilities
 *     eps_t(l)  sum over c != l of w_t(c)  /  sum over c of w_t(c): both sums formed directly in fp32 in class order, never 1 - p
 *     a_t       the lowest class among the maxima of x_t (the greedy decoder's rule)
 *     run of base j (label l, frame f): frame f, then the frames t = f + 1, f + 2, ... below min(the next base's frame, T_b)
 *               (T_b for the last base) for as long as a_t == l.  It always holds f, argmax or not (a beam path's emission
 *               frame need not be one); on a greedy path it is the collapsed run.
 *   dwell  [B][max_labels] int32    frames in the run
 *   error  [B][max_labels] fp32     stat 0: the mean of eps_t(l) over the run, summed in frame order in float64;
 *                                   stat 1: the least eps_t(l) of the run
 *   qual   [B][max_labels] bytes    floor(Q + 0.5) clamped to [0, 93], Q = qscale (-10 log10 error) + qbias in float64 (error 0
 *                                   gives 93, NaN gives 0); the FASTQ character is qual + 33
 *   read_error [B] fp32             the mean of error[b][j] over j < lengths[b]: every thread of one workgroup sums a strided
 *                                   share in order in float64, then a fixed tree; NaN for an empty read.  Uncalibrated.
 * Any of the four may be NULL, not all.  Every launch is bitwise reproducible (no floating-point atomics).
 * Checked on the device: a base with a label outside [0, classes) or equal to blank, a frame outside [0, T_b), or a frame not
 * above its predecessor's has error NaN, qual 0, dwell 0, makes read_error[b] NaN and counts once in *bad (DEVICE int,
 * caller-zeroed, may be NULL).  A read with lengths[b] outside [0, max_labels] or input_lengths[b] outside [0, length] has
 * every entry of its rows so, read_error NaN, and counts once.  Entries at and past lengths[b] are NaN / 0 / 0 too (not
 * counted).  None of these values is used as an index.
 * One thread per base, grid (ceil(max_labels / 256), batch); work per base is its own run.  No workspace.
 * Checked before any launch, in this order.  WN_ERR_BAD_SHAPE: batch, length or max_labels < 1, classes < 2, a negative row
 * stride, an unknown input_kind or stat, qscale not finite and positive, qbias not finite.  WN_ERR_UNSUPPORTED: classes > 64,
 * length > 2^24, max_labels > length, batch > 65535, or a grid of 2^32 threads or more (256 ceil(max_labels / 256) batch).
 * Then WN_ERR_NULL. */
int wn_ctc_base_quality(const float* x, long long sb, long long sc, long long st, int input_kind,
                        const long long* input_lengths /* may be NULL */, const int* labels, long long labels_stride,
                        const int* frames, long long frames_stride, const int* lengths, int batch, int classes, int length,
                        int max_labels, int blank, int stat /* 0 mean, 1 best */, float qscale, float qbias,
                        float* error /* may be NULL */, unsigned char* qual /* may be NULL */, int* dwell /* may be NULL */,
                        float* read_error /* may be NULL */, int* bad /* may be NULL */, wn_stream_t stream);

/* ---- Quality calibration tables and the error profile of aligned reads (wavenet_speech_amd.decoding.quality_profile,
 * DESIGN.md section 7i): walks the ops wn_pair_align wrote for (ref, query) pairs, decides for every query base whether it was
 * right, and tabulates that against the quality and the dwell claimed for it.  Integer arithmetic only.  ops: rows of
 * ops_stride bytes with ops_len [B] int32; ref / query / their lengths: as wn_pair_align takes them; qual: rows of qual_stride
 * bytes, the uncalibrated qual of wn_ctc_base_quality; dwell: int32 rows of dwell_stride elements.  All pointers are DEVICE
 * pointers.  For pair b, column c of its ops:
 *     i_c, j_c   the number of ops in [0, c) with a code in {1, 2, 3} / in {1, 2, 4}: the reference / query index of the column
 *     lo, hi     the first / last column whose op is 1 or 2.  With count_ends = 0 the columns outside [lo, hi] -- every column
 *                when there is no such column -- are END COLUMNS (the unaligned heads and tails an end-gap-free alignment
 *                leaves); with count_ends = 1 there are none
 *   outcome    [B][max_query_len] bytes   of query base j, from its column: 1 match, 2 mismatch, 3 insertion (op 4, not an end
 *                                         column), 4 end (op 4 in an end column); 0 for j >= query_lengths[b]
 *   ref_index  [B][max_query_len] int32   i_c for outcomes 1 and 2, -1 otherwise
 *   read_counts [B][5] int32              matches, mismatches, insertions, deletions (op 3, not an end column), end columns:
 *                                         they sum to ops_len[b]
 *   q_counts   [94][3] int64              row qual[b][j], column outcome - 1, for outcomes 1-3          (given with qual)
 *   dwell_counts [33][3] int64            row min(dwell[b][j], 32), the same columns                     (given with dwell)
 *   confusion  [classes + 1][classes + 1] int64, index `classes` = the gap: [ref[i]][query[j]] for match and mismatch columns,
 *                                         [classes][query[j]] for insertions, [ref[i]][classes] for deletions
 * The three tables are ADDED INTO (64-bit integer adds), never cleared: the caller zeroes them or carries them from batch to
 * batch.  End columns enter no table.  Any output may be NULL, not all.  Two runs are bitwise identical.
 * Checked on the device.  A pair is bad when ops_len[b] is outside [0, max_ops] or a length outside its range; an op in
 * [0, ops_len) is not 1..4; the ops do not consume exactly ref_lengths[b] and query_lengths[b] labels; an op 1 lies where the
 * labels differ or an op 2 where they are equal; a label they consume is outside [0, classes); a qual they consume is above 93
 * or a dwell negative (end columns included).  Its outcome row is 0, its ref_index row -1, its read_counts -1, it adds nothing
 * to any table and counts once in *bad (DEVICE int, caller-zeroed, may be NULL).  A poisoned pair of wn_pair_align (ops_len 0,
 * a length out of range) is such a pair.  No bad value is used as an index.
 * One workgroup per pair, two passes over its ops; no workspace.
 * Checked before any launch, in this order.  WN_ERR_BAD_SHAPE: batch, max_ref_len, max_query_len, max_ops or classes < 1, a
 * negative stride, count_ends not 0 or 1.  WN_ERR_UNSUPPORTED: classes > 64, max_query_len > 8192, max_ref_len > 65535,
 * max_ops > max_ref_len + max_query_len, batch > 65535.  WN_ERR_NULL: ops, ops_len, ref, ref_lengths, query or query_lengths;
 * q_counts without qual or qual without q_counts, likewise dwell_counts and dwell; every output NULL. */
int wn_quality_profile(const unsigned char* ops, long long ops_stride, const int* ops_len, const int* ref, long long ref_stride,
                       const int* ref_lengths, const int* query, long long query_stride, const int* query_lengths,
                       const unsigned char* qual /* may be NULL */, long long qual_stride, const int* dwell /* may be NULL */,
                       long long dwell_stride, int batch, int max_ref_len, int max_query_len, int max_ops, int classes,
                       int count_ends, long long* q_counts /* with qual */, long long* dwell_counts /* with dwell */,
                       long long* confusion /* may be NULL */, int* read_counts /* may be NULL */,
                       unsigned char* outcome /* may be NULL */, int* ref_index /* may be NULL */, int* bad /* may be NULL */,
                       wn_stream_t stream);

/* ---- Event tables and k-mer pore-model tables from a segmentation (wavenet_speech_amd.events.kmer_events, DESIGN.md section
 * 7j): signal + event boundaries + bases give, per event, its k-mer, its sample range and the integer sum and sum of squares of
 * its samples; the used events are added into per-k-mer tables from which a pore model (level mean and stdv per k-mer) and a
 * dwell model are fitted on the host.  The device-side counterpart of what the reference's utils/dump_distributions.py and
 * utils/dump_durations_from_eventalign.py read out of nanopolish eventalign files.  All pointers are DEVICE pointers.
 *   signal           rows of signal_stride elements of which max_signal may be read: fp32 (signal_kind 0) or int16 (1)
 *   signal_lengths   [B] int32, in [0, max_signal]
 *   scale_shift      [B][2] fp32 (scale, shift) or NULL
 *   seg_begin, seg_end   int32: event j of read b begins at seg_begin[b seg_row_stride + j seg_elem_stride] and ends (exclusive)
 *                    at seg_end[the same offset].  spans [B][N][2] of wn_ctc_align: (spans, spans + 1, 2 N, 2); starts
 *                    [B][N + 1] of wn_reads_plan: (starts, starts + 1, N + 1, 1)
 *   frame_stride, frame_offset   event j covers the samples [begin frame_stride + frame_offset, end frame_stride + frame_offset)
 *                    intersected with [0, signal_lengths[b]); positions are formed in 64 bits
 *   labels           int32 rows of labels_stride elements, bases in 1..4; label_lengths [B] int32 in [0, max_labels]
 *   events           [B] int32 in [0, max_events]: the events of each read
 *   k, first         the k-mer of event j is labels[j + first .. j + first + k); its index is sum_i (label_i - 1) 4^(k-1-i), the
 *                    first base most significant.  first = -2, k = 5: centred 5-mers over force-aligned bases; first = 2 / 0:
 *                    the "loader" / "generator" windows of wn_reads_plan
 *   frac_bits F, max_dwell D
 * Arithmetic (the definition).  v = (double)x (double)scale + (double)shift -- the product is exact in double for both kinds,
 * so there is one rounding and a fused multiply-add gives the same bits -- or v = (double)x without scale_shift;
 * q = llrint(v 2^F), ties to even.  A used sample must be finite with |q| < 2^23; a used event holds at most 65536 samples, so
 * sum q^2 < 2^62.  All sums are integers: any reduction order and any atomic order gives the same bits, two runs are bitwise
 * identical.
 * Per-event outputs [B][max_events], each may be NULL:
 *   ev_kmer  int32   the k-mer index when the event is USED, else the first of these that applies:
 *                    -4 in a bad read, or j >= events[b];   -2 no samples after clipping;   -3 cut by signal_lengths[b] (its
 *                    unclipped end lies past it) or longer than 65536 samples;   -1 the window runs off [0, label_lengths[b])
 *   ev_start, ev_len int32   the clipped range [min(s0, n), min(s1, n)), n = signal_lengths[b]; 0, 0 with code -4
 *   ev_sum, ev_sumsq int64   sum q and sum q^2 over the samples of a used event; 0 for every other event (its samples are
 *                    not looked at)
 * read_counts [B][4] int32: events used, events with code -1, events with code -2 or -3, samples in used events.
 * Tables, ADDED INTO with 64-bit integer adds and never cleared; only used events of good reads enter:
 *   kmer_stats [4^k][5] int64   events, samples, sum of ev_sum, sum of (ev_sumsq & 0xffffffff), sum of (ev_sumsq >> 32): the two
 *                    limbs are taken PER EVENT, so sum q^2 = column 4 * 2^32 + column 3 exactly, beyond 64 bits
 *   dwell_hist [4^k][D + 1] int64   column min(ev_len, D)
 * Checked on the device.  A read is bad when signal_lengths[b], label_lengths[b] or events[b] is out of range (nothing else
 * of it is then read); a boundary of an event j < events[b] is negative, begin > end, or begin_j < end_(j-1) (gaps are fine,
 * overlaps are not); a label in the window of an event that would otherwise be used is outside 1..4; a sample of such an
 * event is not finite or has |q| >= 2^23 (scale and shift included).  Samples and labels of events with a negative code are
 * never read and cannot make a read bad.  A bad read has ev_kmer -4, ev_start / ev_len / ev_sum / ev_sumsq 0, read_counts -1
 * throughout, adds nothing to any table and counts once in *bad (DEVICE int, caller-zeroed, may be NULL).  No bad value is
 * used as an index.
 * One memset and two launches through the workspace (validity must be known before anything reaches a shared table): events
 * first, grid (ceil(max_events / 256), batch) so that a long read does not serialise on one workgroup; tables second.  Nothing
 * is read back: the call can be captured into a HIP graph.  workspace: wn_kmer_events_workspace_bytes(batch, max_events)
 * bytes, 16-byte aligned (per-read flags and counts, and the per-event rows the caller passes NULL for); 0 for batch or
 * max_events out of range.
 * Checked before any launch, in this order.  WN_ERR_BAD_SHAPE: batch, max_events, max_signal or max_labels < 1, a negative
 * stride, frame_stride < 1, frame_offset < 0, signal_kind not 0 or 1.  WN_ERR_UNSUPPORTED: k outside 1..6, |first| > 8, F
 * outside 0..20, D outside 1..65536, batch > 65535, max_signal frame_stride >= 2^31.  WN_ERR_NULL: signal, signal_lengths,
 * seg_begin, seg_end, labels, label_lengths, events or the workspace (with or without tables); every output NULL (bad is no
 * output).  WN_ERR_WORKSPACE: a workspace too small or not 16-byte aligned, a signal not aligned to its element size. */
size_t wn_kmer_events_workspace_bytes(int batch, int max_events);
int wn_kmer_events(const void* signal, int signal_kind, long long signal_stride, const int* signal_lengths,
                   const float* scale_shift /* may be NULL */, const int* seg_begin, const int* seg_end, long long seg_row_stride,
                   long long seg_elem_stride, int frame_stride, int frame_offset, const int* labels, long long labels_stride,
                   const int* label_lengths, const int* events, int batch, int max_signal, int max_labels, int max_events, int k,
                   int first, int frac_bits, int max_dwell, int* ev_kmer /* may be NULL */, int* ev_start /* may be NULL */,
                   int* ev_len /* may be NULL */, long long* ev_sum /* may be NULL */, long long* ev_sumsq /* may be NULL */,
                   int* read_counts /* may be NULL */, long long* kmer_stats /* may be NULL */,
                   long long* dwell_hist /* may be NULL */, void* workspace, size_t workspace_bytes, int* bad /* may be NULL */,
                   wn_stream_t stream);

/* ---- Signal-to-base alignment under the k-mer pore model (wavenet_speech_amd.events.signal_align): the
 * raw samples of a read against the k-mers of its KNOWN bases, the minimum-cost monotone path inside a band around the
 * diagonal.  The segmentation nanopolish `eventalign` makes before the reference's utils/dump_distributions.py reads it, with
 * no network; its `starts` go straight into wn_kmer_events.  All pointers are DEVICE pointers.
 *   signal, signal_kind, signal_stride, signal_lengths, scale_shift, labels, labels_stride, label_lengths: as wn_kmer_events
 *   model            [4^k][3] int32: level, weight, offset per k-mer
 *   k, first         read b has N_b = label_lengths[b] - (k - 1) - 2 first STATES; state j is the k-mer labels[j + first .. j +
 *                    first + k), index sum_i (label_i - 1) 4^(k-1-i).  first = 2 / 0: the "loader" / "generator" windows of
 *                    wn_reads_plan
 *   frac_bits F, weight_shift S, max_cost, band W
 * Arithmetic (the definition; tests/signal_align_ref.py mirrors it).  Samples exactly as wn_kmer_events: v = (double)x
 * (double)scale + (double)shift, or (double)x; q = llrint(v 2^F), ties to even; v finite and |q| < 2^23.  With d = |q - level|
 * (< 2^24), the cost of a sample in a state is   min((d d weight) >> S, max_cost) + offset,   the product in full (79 bits).
 * A path has s_0 = 0, s_(T-1) = N - 1 and moves by 0 (stay) or +1 (step) per sample: no skips, every k-mer holds at least one
 * sample, and no transition costs (they would be the same constant on every path).  Its cost is the sum of its sample costs
 * (below 2^24 (2^31 + 2^30) in magnitude: int64).  The result is the minimum-cost path INSIDE THE BAND:
 *   c(t) = ((2 t + 1) N) / (2 T) in 64-bit integer division;   lo(t) = clamp(c(t) - W / 2, 0, max(N - W, 0));
 *   state j is allowed at sample t if and only if lo(t) <= j < lo(t) + W.
 * For N <= T the centre line c is itself a path inside the band, so an alignment exists whenever T >= N >= 1.  Ties: at (t, j)
 * the stay predecessor (t - 1, j) is taken first, the step predecessor (t - 1, j - 1) replaces it only if strictly smaller.
 * Outputs:
 *   starts        [B][max_events + 1] int32   starts[j] = the first sample of state j; every entry j >= N_b is T_b (the
 *                 convention of wn_reads_plan: event j = [starts[j], starts[j + 1]))
 *   score         [B] int64   the cost of the path
 *   band_hits     [B] int32   the samples t whose state is lo(t) with lo(t) > 0, or lo(t) + W - 1 with lo(t) + W < N: the
 *                 caller's sign that the band was too narrow
 *   sample_state  [B][max_signal] int32, may be NULL   the state of every sample, -1 past the read
 * Checked on the device, in this order.  A read is BAD when signal_lengths[b] is outside [0, max_signal], label_lengths[b]
 * outside [0, max_labels] or N_b > max_events (nothing else of it is then read): score LLONG_MIN, every other output -1, counted
 * once in *bad (DEVICE int, caller-zeroed, may be NULL).  A read with N_b < 1 or T_b < N_b gives NO ALIGNMENT: score LLONG_MAX,
 * starts and sample_state -1, band_hits 0; nothing else of it is read and it is not bad.  Every other read is bad (as above)
 * when a label in labels[first .. first + N_b + k - 1) is outside 1..4, a sample in [0, T_b) is not finite or has |q| >= 2^23,
 * or the model row of one of its k-mers has weight < 1, |level| >= 2^23 or |offset| >= 2^30.  Samples past T_b are never read.
 * No bad value is used as an index.
 * One launch, one workgroup per read: T_b sequential steps over band / 8 threads, then the trace.  Nothing is read back: the
 * call can be captured into a HIP graph.  workspace: wn_signal_align_workspace_bytes(batch, max_signal, band) bytes, 16-byte
 * aligned (1 bit per sample and band slot); 0 for an argument out of range.
 * Checked before any launch, in this order.  WN_ERR_BAD_SHAPE: batch, max_signal, max_labels or max_events < 1, a negative
 * stride, signal_kind not 0 or 1.  WN_ERR_UNSUPPORTED: k outside 1..6, first outside 0..8, F outside 0..20, S outside 16..63,
 * max_cost < 1, band not a multiple of 64 in [64, 2048], batch > 65535, max_signal > 2^24, max_events > 2^20.  WN_ERR_NULL:
 * signal, signal_lengths, labels, label_lengths, model, starts, score, band_hits or the workspace.  WN_ERR_WORKSPACE: a
 * workspace too small or not 16-byte aligned, a signal not aligned to its element size. */
size_t wn_signal_align_workspace_bytes(int batch, int max_signal, int band);
int wn_signal_align(const void* signal, int signal_kind, long long signal_stride, const int* signal_lengths,
                    const float* scale_shift /* may be NULL */, const int* labels, long long labels_stride,
                    const int* label_lengths, const int* model, int batch, int max_signal, int max_labels, int max_events, int k,
                    int first, int frac_bits, int weight_shift, int max_cost, int band, int* starts, long long* score,
                    int* band_hits, int* sample_state /* may be NULL */, void* workspace, size_t workspace_bytes,
                    int* bad /* may be NULL */, wn_stream_t stream);

/* ---- Signal-to-reference mapping under the k-mer pore model (wavenet_speech_amd.mapping.signal_map): the
 * first samples of a read against EVERY state of a reference's k-mer sequence, start free and end free -- the subsequence form
 * of wn_signal_align's dynamic program, under the same model.  It says where the read lies, at what cost, and how far ahead of
 * the next best locus that is; wn_signal_align on the mapped span then gives the path.  All pointers are DEVICE pointers.
 * Reference.  ref [ref_len] int32: bases 1..4, and 0 for a break (an N, a contig boundary, the joint between the two strands).
 * It has M = ref_len - k + 1 STATES, state j the k-mer ref[j .. j + k) (index as wn_signal_align).  A state whose window holds a
 * 0 is a WALL: no path is ever in it.  wn_signal_map_reference turns ref and model ([4^k][3] int32: level, weight, offset) into
 * the opaque buffer `prepared` (wn_signal_map_reference_bytes(ref_len, k) bytes, 16-byte aligned; 0 for ref_len < k, k outside
 * 1..6 or ref_len > 2^26) in one launch, once per (reference, model).  A label outside 0..4 counts once in *bad (DEVICE int,
 * caller-zeroed, may be NULL) and is treated as 0; a state whose window lies in 1..4 but whose model row is out of range
 * (weight < 1, |level| >= 2^23, |offset| >= 2^30) counts once in *bad and is a wall.  Nothing bad is used as an index.  Checked
 * before the launch, in this order.  WN_ERR_BAD_SHAPE: ref_len < 1 or ref_len < k.  WN_ERR_UNSUPPORTED: k outside 1..6, ref_len
 * > 2^26.  WN_ERR_NULL: ref, model or prepared.  WN_ERR_WORKSPACE: prepared too small or not 16-byte aligned.
 * Samples: signal, signal_kind, signal_stride, signal_lengths, scale_shift and their quantisation q exactly as wn_signal_align;
 * T_b = signal_lengths[b].  The cost of a sample in a state is wn_signal_align's, min((d d weight) >> S, max_cost) + offset.
 * Recurrence (the definition; tests/signal_map_ref.py mirrors it), int64 throughout, +inf = 2^62:
 *   D(0, j) = cost(q_0, j) for every state j that is no wall (the start is free);
 *   D(t, j) = cost(q_t, j) + min(D(t-1, j), D(t-1, j-1)): stay or step, no skips.  Column -1 and walls are +inf; a wall stays
 *   +inf, a state whose two predecessors are +inf is +inf.  The origin O(0, j) = j, O(t, j) = the origin of the predecessor
 *   taken; ties as wn_signal_align: the stay first, the step only if strictly smaller.
 * Outputs per read:
 *   score      [B] int64   min_j D(T_b - 1, j);   end [B] int32   the smallest such j;   start [B] int32   O(T_b - 1, end), so
 *              0 <= end - start <= T_b - 1
 *   block_cost [B][ceil(M / 64)] int64, block_end [B][ceil(M / 64)] int32   block g covers the end states [64 g, 64 g + 64)
 *              below M: the minimum of the last row over the block and its smallest argmin; LLONG_MAX and -1 for a block with
 *              no finite cell.  The granule 64 is WN_MAP_GRANULE, part of this ABI and not of the kernel's tiling
 *   runner_up  [B] int64   the minimum of block_cost[g] over the blocks with 64 g + 63 <= end - T_b or 64 g >= end + T_b (two
 *              paths whose ends are T_b apart share no state: the best other locus); LLONG_MAX if there is none
 *   end_cost   [B][M] int64, may be NULL   the whole last row, LLONG_MAX where it is +inf
 * Checked on the device, in this order.  T_b outside [0, max_signal]: the read is BAD and nothing else of it is read.  T_b ==
 * 0: NO MAPPING.  A sample in [0, T_b) that is not finite or has |q| >= 2^23: BAD.  A last row with no finite cell: NO MAPPING.
 * No mapping: score, runner_up, every block_cost (and end_cost) LLONG_MAX; end, start and every block_end -1.  A bad read has
 * LLONG_MIN in every int64 output (end_cost included) and -1 in every int32 output, and counts once in *bad (DEVICE int,
 * caller-zeroed, may be NULL).  Samples past T_b are never read.
 * strip_states: how many end states one workgroup owns, a multiple of 64 in [64, 2^20], or 0 for the library's choice from
 * max_signal, M and batch.  A tuning argument: NO OUTPUT DEPENDS ON IT.  Two launches (the strips, grid (ceil(M / strip),
 * batch); then one workgroup per read over the block table); integer arithmetic only, bitwise reproducible; nothing is read
 * back and nothing is allocated, so the call can be captured into a HIP graph.  workspace:
 * wn_signal_map_workspace_bytes(batch, max_signal, ref_len, k, strip_states) bytes, 16-byte aligned; 0 for an argument out of
 * range.
 * Checked before any launch, in this order.  WN_ERR_BAD_SHAPE: batch, max_signal or ref_len < 1, ref_len < k, a negative stride,
 * signal_kind not 0 or 1.  WN_ERR_UNSUPPORTED: k outside 1..6, F outside 0..20, S outside 16..63, max_cost < 1, max_signal >
 * 4096, ref_len > 2^26, batch > 65535, a strip_states that is neither 0 nor a multiple of 64 in [64, 2^20], a grid of 2^31
 * workgroups or more.  WN_ERR_NULL: signal, signal_lengths, prepared, score, end, start, runner_up, block_cost, block_end or the
 * workspace.  WN_ERR_WORKSPACE: a workspace too small or not 16-byte aligned, a signal not aligned to its element size. */
#define WN_MAP_GRANULE 64
size_t wn_signal_map_reference_bytes(int ref_len, int k);
int wn_signal_map_reference(const int* ref, int ref_len, const int* model, int k, void* prepared, size_t prepared_bytes,
                            int* bad /* may be NULL */, wn_stream_t stream);
size_t wn_signal_map_workspace_bytes(int batch, int max_signal, int ref_len, int k, int strip_states);
int wn_signal_map(const void* signal, int signal_kind, long long signal_stride, const int* signal_lengths,
                  const float* scale_shift /* may be NULL */, const void* prepared, int ref_len, int k, int batch, int max_signal,
                  int frac_bits, int weight_shift, int max_cost, int strip_states, long long* score, int* end, int* start,
                  long long* runner_up, long long* block_cost, int* block_end, long long* end_cost /* may be NULL */,
                  void* workspace, size_t workspace_bytes, int* bad /* may be NULL */, wn_stream_t stream);

/* ---- Event detection (wavenet_speech_amd.events.detect_events): a raw read in, the table of its events
 * out -- where its level changes -- with no bases and no network: what nanopolish, scrappie, UNCALLED and sigmap run before
 * anything else.  Its `starts` follow wn_signal_align's convention and its event means are a shorter "read" for wn_signal_map and
 * wn_signal_align.  All pointers are DEVICE pointers.
 *   signal, signal_kind, signal_stride, signal_lengths, scale_shift, frac_bits F: as wn_kmer_events; q_t = llrint(v_t 2^F), ties
 *   to even, |q| < 2^23; T_b = signal_lengths[b] in [0, max_signal].
 * Two detectors, `short` (d = 0) and `long` (d = 1), each with a window w_d in 1..16 (window_long = 0 switches the long detector
 * off; its other three arguments are then ignored), a radius r_d in 1..64, a threshold theta_d (int32 >= 1, on t^2 in units of
 * 2^-8) and a variance floor vmin_d = min_var_* (int64 in 1..2^55).
 * Arithmetic (the definition; tests/event_detect_ref.py mirrors it in Python integers).  For a position i with w <= i <= T - w:
 *   S1 = sum q[i-w .. i),  S2 = sum q[i .. i+w),  Q = sum of q^2 over both windows,
 *   A_i = w (S2 - S1)^2 (< 2^60),   V_i = max(w Q - S1^2 - S2^2, vmin) (<= 2^55),   score(i) = A_i / V_i:
 * Welch's t^2 between two equal windows.  Every other position has score 0.  Scores are compared exactly as rationals: A_i / V_i
 * > A_j / V_j iff A_i V_j > A_j V_i, in 128-bit products; i PASSES THE THRESHOLD iff 256 A_i >= theta V_i.  No floating-point
 * division or square root appears.  i is a PEAK of detector d iff it passes the threshold and, for every j != i in [i - r, i + r],
 * its score is strictly greater when j < i and greater or equal when j > i (ties go to the smaller index).
 * Boundaries of a read with T >= 1: position 0; every short peak; every long peak with no short peak within +-w_1 (distance
 * w_1 included).  Then every gap between consecutive boundaries -- T counts as the last boundary -- that is longer than
 * max_event_len (1..65536, so that an event's sum of q^2 stays below 2^62) also gets a FORCED boundary every max_event_len samples
 * after its left end.  Event e is [b_e, b_(e+1)).
 * Outputs ([B][max_events] unless said otherwise):
 *   n_events  [B] int32   the true count of events, even above max_events: the rows then hold the first max_events events whole
 *   starts    [B][max_events + 1] int32   starts[e] = b_e; every entry e >= n_events[b] is T_b (wn_signal_align's convention)
 *   ev_sum, ev_sumsq  int64   sum q and sum q^2 over the event; 0 past the last event
 *   ev_kind   int32, may be NULL   why the event begins: 0 the read's start, 1 a short peak, 2 a long peak, 3 forced; -1 past
 *             the last event
 * Checked on the device.  T_b = 0 gives 0 events and is not bad.  A read is BAD when T_b is outside [0, max_signal] (nothing
 * else of it is then read) or a sample in [0, T_b) is not finite or has |q| >= 2^23: n_events -1, starts -1, ev_sum / ev_sumsq
 * 0, ev_kind -1, counted once in *bad (DEVICE int, caller-zeroed, may be NULL).  Samples past T_b are never read.
 * chunk_samples: the positions one workgroup of the first launch decides, a multiple of 256 in [256, 16384], or 0 for the
 * library's choice.  A tuning argument: NO OUTPUT DEPENDS ON IT and it sizes nothing.  One memset and three launches (scores and
 * peaks, grid (ceil(max_signal / chunk), batch); ranks, one workgroup per read; sums, grid (ceil((max_events + 1) / 256), batch));
 * integer arithmetic only, two runs are bitwise identical; nothing is read back and nothing is allocated, so the call can be
 * captured into a HIP graph.  workspace: wn_event_detect_workspace_bytes(batch, max_signal) bytes, 16-byte aligned (a flag per
 * read and two bits per sample); 0 for batch outside 1..65535 or max_signal outside 1..2^24.
 * Checked before any launch, in this order.  WN_ERR_BAD_SHAPE: batch, max_signal or max_events < 1, a negative stride,
 * signal_kind not 0 or 1.  WN_ERR_UNSUPPORTED: F outside 0..20, batch > 65535, max_signal > 2^24, max_events > 2^24,
 * window_short outside 1..16, window_long outside 0..16, a radius outside 1..64, a threshold < 1, a min_var outside 1..2^55 (the
 * long detector's three only with window_long > 0), max_event_len outside 1..65536, a chunk_samples that is neither 0 nor a
 * multiple of 256 in [256, 16384].  WN_ERR_NULL: signal, signal_lengths, n_events, starts, ev_sum, ev_sumsq or the workspace.
 * WN_ERR_WORKSPACE: a workspace too small or not 16-byte aligned, a signal not aligned to its element size. */
size_t wn_event_detect_workspace_bytes(int batch, int max_signal);
int wn_event_detect(const void* signal, int signal_kind, long long signal_stride, const int* signal_lengths,
                    const float* scale_shift /* may be NULL */, int batch, int max_signal, int frac_bits, int window_short,
                    int window_long, int radius_short, int radius_long, int threshold_short, int threshold_long,
                    long long min_var_short, long long min_var_long, int max_event_len, int max_events, int chunk_samples,
                    int* n_events, int* starts, long long* ev_sum, long long* ev_sumsq, int* ev_kind /* may be NULL */,
                    void* workspace, size_t workspace_bytes, int* bad /* may be NULL */, wn_stream_t stream);

/* ---- Event alignment with skips (wavenet_speech_amd.events.event_align): the DETECTED events of a read
 * against the k-mers of its KNOWN bases.  An event may stay in the k-mer of the event before it (the detector cut one k-mer in
 * two), step to the next one, or skip one or two k-mers (the detector missed boundaries), and an event's cost weighs its length:
 * what nanopolish `eventalign` does, and what wn_signal_align, which never skips, cannot do for a read with fewer events than
 * k-mers.  All pointers are DEVICE pointers.
 * Events of read b: n_events [B] int32, ev_starts [B][max_events + 1] int32, ev_sum and ev_sumsq [B][max_events] int64 -- exactly
 * what wn_event_detect writes.  E_b = n_events[b]; event e has n = ev_starts[e + 1] - ev_starts[e] samples, S = ev_sum[e] (the sum
 * of its quantised samples q) and Q = ev_sumsq[e] (of q^2); T_b = ev_starts[E_b].  A caller whose table is truncated passes
 * min(n_events, max_events).
 * Bases: labels, labels_stride, label_lengths, k, first as wn_signal_align: N_b = label_lengths[b] - (k - 1) - 2 first STATES, state
 * j the k-mer labels[j + first .. j + first + k), index sum_i (label_i - 1) 4^(k-1-i).
 * Model: model [4^k][3] int32 (level, weight, offset), frac_bits F, weight_shift S and max_cost as wn_signal_align (F only says
 * in what units the events and the levels are; it is range-checked and otherwise unused).
 * Moves: move_cost0 .. move_cost3, the cost of advancing by 0 (stay), 1 (step), 2 or 3 states between consecutive events, each
 * in [0, 2^30) or -1 for a move that is FORBIDDEN; the step must be allowed.
 * Arithmetic (the definition; tests/event_align_ref.py mirrors it in Python integers).  In a state with the row (level, weight,
 * offset), D = Q - 2 level S + n level^2, the exact sum of (q - level)^2 over the event's samples; 0 <= D < 65536 (2^24 - 2)^2 <
 * 2^64 for a valid event, so D is formed modulo 2^64.  The cost of the event in the state is
 *   min((D weight) >> S, n max_cost) + n offset,
 * the product in full (95 bits) and compared before it is narrowed.  For n = 1 this is wn_signal_align's cost of the sample q.
 * A path gives every event a state: s_0 = 0, s_(E-1) = N - 1, s_e - s_(e-1) in {0, 1, 2, 3} and allowed.  Its cost is the sum of
 * its event costs and of move_cost[s_e - s_(e-1)] over e >= 1 (below 2^24 (2^31 + 2^30) + 2^20 2^30 in magnitude: int64).  The
 * result is the minimum-cost path INSIDE THE BAND, W = band:
 *   c(e) = ((2 e + 1) N) / (2 E) in 64-bit integer division;   lo(e) = clamp(c(e) - W / 2, 0, max(N - W, 0));
 *   state j is allowed at event e if and only if lo(e) <= j < lo(e) + W.
 * Ties: at (e, j) the stay is taken first, then each larger move only if strictly cheaper, its move cost included.
 * Outputs:
 *   starts        [B][max_states + 1] int32   starts[j] = the first SAMPLE of state j (ev_starts of its first event), the
 *                 convention of wn_reads_plan; a skipped state is empty, starts[j] = starts[j + 1]; every entry j >= N_b is T_b.
 *                 It goes into wn_kmer_events as it stands
 *   score         [B] int64   the cost of the path
 *   event_state   [B][max_events] int32, may be NULL   the state of every event, -1 past E_b
 *   move_counts   [B][4] int32   the events that arrived by each move: 1 + sum = E_b, counts[1] + 2 counts[2] + 3 counts[3] = N_b - 1
 *   band_hits     [B] int32   the events e whose state is lo(e) with lo(e) > 0, or lo(e) + W - 1 with lo(e) + W < N
 * Checked on the device, in this order.  (1) A read is BAD when n_events[b] is outside [0, max_events], label_lengths[b] outside
 * [0, max_labels] or N_b > max_states (nothing else of it is then read): score LLONG_MIN, every other output -1, counted once in
 * *bad (DEVICE int, caller-zeroed, may be NULL).  (2) E_b < 1, N_b < 1 or N_b - 1 > (the largest allowed move) (E_b - 1) gives
 * NO ALIGNMENT: score LLONG_MAX, starts and event_state -1, move_counts and band_hits 0; nothing else of it is read and it is not
 * bad.  (3) Every other read is bad (as above) when a label in labels[first .. first + N_b + k - 1) is outside 1..4, the model
 * row of one of its k-mers has weight < 1, |level| >= 2^23 or |offset| >= 2^30, ev_starts[0] < 0 or T_b > 2^24, or an event in
 * [0, E_b) has n outside [1, 65536], |S| > n (2^23 - 1), Q < 0, Q > n (2^23 - 1)^2 or S^2 > n Q (compared exactly in 128 bits:
 * this is what makes D >= 0).  (4) A good read with no allowed path inside the band gives no alignment.  No bad value is used as
 * an index; events past E_b are never read.
 * One launch, one workgroup per read: E_b sequential steps over band / 8 threads, then the trace.  Integer arithmetic only, two
 * runs are bitwise identical; nothing is read back and nothing is allocated, so the call can be captured into a HIP graph.
 * workspace: wn_event_align_workspace_bytes(batch, max_events, band) bytes, 16-byte aligned (2 bits per event and band slot); 0
 * for an argument out of range.
 * Checked before any launch, in this order.  WN_ERR_BAD_SHAPE: batch, max_events, max_labels or max_states < 1, a negative
 * stride.  WN_ERR_UNSUPPORTED: k outside 1..6, first outside 0..8, F outside 0..20, S outside 16..63, max_cost < 1, band not a
 * multiple of 64 in [64, 2048], move_cost1 < 0, a move cost that is neither -1 nor in [0, 2^30), batch > 65535, max_events or
 * max_states > 2^20.  WN_ERR_NULL: n_events, ev_starts, ev_sum, ev_sumsq, labels, label_lengths, model, starts, score,
 * move_counts, band_hits or the workspace.  WN_ERR_WORKSPACE: a workspace too small or not 16-byte aligned. */
size_t wn_event_align_workspace_bytes(int batch, int max_events, int band);
int wn_event_align(const int* n_events, const int* ev_starts, const long long* ev_sum, const long long* ev_sumsq,
                   const int* labels, long long labels_stride, const int* label_lengths, const int* model, int batch,
                   int max_events, int max_labels, int max_states, int k, int first, int frac_bits, int weight_shift, int max_cost,
                   int band, int move_cost0, int move_cost1, int move_cost2, int move_cost3, int* starts, long long* score,
                   int* event_state /* may be NULL */, int* move_counts, int* band_hits, void* workspace, size_t workspace_bytes,
                   int* bad /* may be NULL */, wn_stream_t stream);

/* ---- Barcode demultiplexing and adapter trimming of decoded reads (csrc/wn_demux.hip): which sample a
 * read belongs to, and where its adapters and barcodes end -- what guppy, dorado, porechop and qcat do right after basecalling.
 * Two launches; all pointers are DEVICE pointers; int32 and exact.
 *   wn_demux_scores: SEMI-GLOBAL alignment with affine gaps of each of K patterns against the front or the rear WINDOW of each of
 *   B reads.  labels [B] rows of labels_stride elements with lengths [B] (the decoders' rows, read in place): int32, compared for
 *   equality only; values past lengths[b] are never read.  patterns [K] rows of pattern_stride elements with pattern_lengths [K];
 *   patterns [0, n_front) belong to the FRONT of the read, [n_front, K) to its REAR (the caller sorts them by end).  For a read of
 *   length n the front window is labels[0 .. min(n, window)), the rear window labels[max(0, n - window) .. n).
 *   The pattern (rows i = 1..P) is consumed whole; its start and end in the window (columns j = 1..W) are free.  A gap of n columns
 *   costs gap_open + (n - 1) gap_extend.  Every cell is a pair (score, start) and every maximum is lexicographic on (score, -start):
 *     H[0][j] = (0, j);  H[i][0] = F[i][0] = (-(go + (i-1) ge), 0);  E[0][j] = F[0][j] = E[i][0] = -infinity
 *     E[i][j] = max(H[i][j-1] - go, E[i][j-1] - ge);   F[i][j] = max(H[i-1][j] - go, F[i-1][j] - ge)
 *     H[i][j] = max(H[i-1][j-1] + (equal ? match : mismatch), E[i][j], F[i][j])
 *     result  = max over j in [0, W] of (H[P][j].score, -start, -j)
 *   which does not depend on the order of the candidates: the greatest score over all semi-global alignments, among those the
 *   smallest start, then the smallest end (tests/demux_ref.py holds the same definition).
 *   score, start, end [B][K] int32: start and end = j in READ coordinates, end exclusive; start == end: the pattern met only gaps.
 *   A read length outside [0, max_len] poisons its row, a pattern length outside [1, max_pattern_len] its column: score INT_MIN,
 *   start and end -1, every poisoned entry counted in *bad (DEVICE int, caller-zeroed, may be NULL); no bad value is used as an
 *   index.  Length 0 is valid: the window is empty and every score is -(go + (P-1) ge).
 *   Limits: window <= 512, n_patterns <= 1024, max_pattern_len <= 128, max_len <= 2^24, batch <= 65535, 0 <= gap_extend <= gap_open
 *   <= 1024, |match|, |mismatch| <= 1024 (WN_ERR_UNSUPPORTED, nothing launched).  No workspace.
 *   wn_demux_pick: one decision per read from those tables.  pattern_group [K] >= 0: the barcode or adapter a pattern stands for;
 *   min_score [K]; min_margin >= 0.  Per end (front: patterns [0, n_front), rear: the others; a poisoned entry is no candidate):
 *   the HIT is the greatest score, ties to the lower pattern index; the RUNNER-UP the greatest score among that end's patterns of
 *   another group, INT_MIN if there is none; the hit PASSES if score >= min_score[hit] and score - runner_up >= min_margin (with no
 *   runner-up the margin holds).
 *     barcode   [B]        require_both: the group of the front hit if both ends pass and agree, else -1; otherwise the group of the
 *                          passing end with the greater score, a tie to the front, -1 if neither passes
 *     trim      [B][2]     trim_start = the end of the front hit if it passes, else 0; trim_end = max(trim_start, the start of the
 *                          rear hit) if it passes, else lengths[b] as it stands
 *     hits      [B][2][4]  per end (pattern, score, start, end); four times -1 where the end has no candidate
 *     runner_up [B][2]
 * Checked before any launch, in this order.  WN_ERR_BAD_SHAPE: batch or n_patterns < 1, n_front outside [0, n_patterns], (scores)
 * max_len, max_pattern_len or window < 1, a negative stride.  WN_ERR_UNSUPPORTED: a limit above, (pick) min_margin < 0.
 * WN_ERR_NULL: any pointer but bad.  Nothing is read back or allocated: both calls can be captured into a HIP graph. */
int wn_demux_scores(const int* labels, long long labels_stride, const int* lengths, const int* patterns, long long pattern_stride,
                    const int* pattern_lengths, int batch, int max_len, int n_patterns, int n_front, int max_pattern_len,
                    int window, int match, int mismatch, int gap_open, int gap_extend, int* score, int* start, int* end,
                    int* bad /* may be NULL */, wn_stream_t stream);
int wn_demux_pick(const int* score, const int* start, const int* end, const int* lengths, const int* pattern_group,
                  const int* min_score, int batch, int n_patterns, int n_front, int min_margin, int require_both, int* barcode,
                  int* trim, int* hits, int* runner_up, wn_stream_t stream);

/* ---- Read mapping in base space (csrc/wn_readmap.hip): which stretch of a reference, on which strand, a
 * decoded read came from -- minimizer seeds looked up in an index of the reference and chained, the step minimap2 runs after
 * basecalling.  Three launches; all pointers are DEVICE pointers; everything written is an integer and exact.  Labels: int32, 1..4
 * are bases with complement 5 - v; anything else, 0 included, is a break.  tests/readmap_ref.py holds the same definition as plain
 * loops.
 *   K-MERS      the k-mer at p in [0, n - k]: forward code f = sum_i (label[p+i] - 1) 4^(k-1-i), reverse-complement code
 *               r = sum_i (4 - label[p+i]) 4^i (uint32).  INVALID if a label is outside 1..4 or f == r (a palindrome); else canon =
 *               min(f, r), strand = (r < f), hash = fmix32(canon) (murmur3's finaliser: x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13;
 *               x *= 0xC2B2AE35; x ^= x >> 16), key = (hash, p).
 *   MINIMIZERS  n_k = n - k + 1 >= 1; the windows are [s, s + w) for s in [0, n_k - w], or the single window [0, n_k) if n_k < w.
 *               p is a minimizer iff it holds a valid k-mer whose key is the lexicographic minimum over the valid k-mers of at least
 *               one window (equal hashes: the smallest position).  No result depends on how the row is cut into chunks.
 *   wn_minimizers: labels [B] rows of labels_stride elements with lengths [B] -> code [B][max_len] (the canon code of a minimizer, 0
 *   elsewhere) and flag [B][max_len] bytes (0 none, 1 the forward code is canonical, 2 the reverse complement's); every element of
 *   both is written.  chunk: positions per workgroup, 0 = chosen by the library; a tuning argument, no output depends on it.
 *   INDEX       `index` [n_index] int64, ascending: canon << 28 | pos << 1 | strand of every minimizer of the reference, i.e.
 *               sorted by (canon, pos); the caller builds it from wn_minimizers of the reference (batch 1) and sorts.
 *   ANCHORS     of a read of length n: its minimizers in ascending position q; for each the index entries of equal canon in
 *               ascending pos, all dropped if there are more than max_occ.  An anchor is (s, r, q'): s = strand_read ^ strand_ref,
 *               r = pos, q' = q if s == 0 else n - k - q.  The first anchors_per_read anchors of this enumeration are kept.
 *   wn_read_seeds: code, flag [B][max_len] of the reads (as wn_minimizers wrote them, same k) -> keys [B][anchors_per_read] int64, one
 *   word s << 43 | r << 16 | q' per kept anchor -- the first anchors_per_read of the enumeration, SORTED ascending (keys are distinct:
 *   one result), which is the order wn_chain reads -- then INT64_MAX; n_minimizers, n_anchors (kept), truncated (1 if there were more) [B].
 *   CHAINING    each strand on its own, its anchors in (r, q') order.  f(i) = max over candidates of (score, j), lexicographic: the
 *               fresh start (16 k, i); and every j in [max(0, i - h), i) with dr = r_i - r_j, dq = q'_i - q'_j, 0 < dr <= max_dist,
 *               0 < dq <= max_dist and dd = |dr - dq| <= bandwidth as (f(j) + 16 min(dr, dq, k) - gap(dd), j), gap(0) = 0, else
 *               gap(dd) = gap_base dd + gap_log floor(log2 dd).  A fresh start beats an equal extension; of equal extensions the
 *               nearest wins.  root(i) = i or root(pred); count(i) = 1 or count(pred) + 1.  16 k <= f <= 16 * 16 * 32768 = 2^23.
 *   wn_chain: keys [B][anchors_per_read] sorted rows with n_anchors [B], lengths [B] (the reads') -> result [B][8] int32: score,
 *   strand, ref_start, ref_end, query_start, query_end, n_anchors, runner_up.  The best anchor is the maximum of f over both strands,
 *   ties to the forward strand, then to the smallest i; ref_start = r_root, ref_end = r_best + k; query span in read orientation:
 *   forward [q'_root, q'_best + k), reverse [n - k - q'_best, n - q'_root); n_anchors = count; runner_up = the greatest f over all
 *   anchors whose (strand, root) differs from the best one's, INT_MIN if none.  No anchors: INT_MIN, five times -1, 0, INT_MIN.
 *   f, pred [B][anchors_per_read] int32 (both or neither): the whole table, pred an index into the sorted row, -1 for a fresh
 *   start; past n_anchors INT_MIN and -1.
 * A length outside [0, max_len] (wn_chain: also n_anchors outside [0, anchors_per_read]) makes the read one without anchors and is
 * counted in *bad (DEVICE int, caller-zeroed, may be NULL); no such value is used as an index.
 * Checked before any launch, in this order.  WN_ERR_BAD_SHAPE: batch or max_len < 1, a negative stride, chunk or n_index.
 * WN_ERR_UNSUPPORTED: outside 1 <= k <= 16, 1 <= w <= 64, chunk <= 2048, 1 <= max_occ <= 64, 1 <= h <= 1024, 1 <= anchors_per_read
 * <= 32768, 1 <= max_dist, bandwidth <= 2^26, 0 <= gap_base, gap_log <= 1024, batch <= 65535, max_len <= 2^26 (wn_minimizers) or
 * 65535 (the reads of wn_read_seeds and wn_chain), n_index <= 2^26.  WN_ERR_NULL: any pointer but bad (f and pred: one without the
 * other).  No workspace; nothing is read back or allocated: every call can be captured into a HIP graph. */
int wn_minimizers(const int* labels, long long labels_stride, const int* lengths, int batch, int max_len, int k, int w, int chunk,
                  unsigned* code, unsigned char* flag, int* bad /* may be NULL */, wn_stream_t stream);
int wn_read_seeds(const unsigned* code, const unsigned char* flag, const int* lengths, const long long* index, int n_index, int batch,
                  int max_len, int k, int max_occ, int anchors_per_read, long long* keys, int* n_minimizers, int* n_anchors,
                  int* truncated, int* bad /* may be NULL */, wn_stream_t stream);
int wn_chain(const long long* keys, const int* n_anchors, const int* lengths, int batch, int max_len, int anchors_per_read, int k,
             int h, int max_dist, int bandwidth, int gap_base, int gap_log, int* result, int* f /* may be NULL */,
             int* pred /* may be NULL */, int* bad /* may be NULL */, wn_stream_t stream);

/* ---- Pileup, consensus and variant calls from mapped reads (wavenet_speech_amd/pileup.py): what the reads
 * of a locus show together -- the counting step of samtools mpileup / consensus and bcftools call.  Integer arithmetic only; all
 * pointers are DEVICE pointers.  Labels 1..4 are bases with complement 5 - v.  tests/pileup_ref.py holds the same definitions as
 * plain loops.
 *   wn_pileup: read b is query row b (query_stride elements, query_lengths[b] labels; qual rows of qual_stride bytes beside it)
 *   aligned by the ops of row b (ops_stride bytes, ops_len[b] of them, as wn_pair_align wrote them) against the window
 *   [lo[b], lo[b] + ref_lengths[b]) of the reference's forward strand IN READ ORIENTATION: on strand[b] = 1 reference index i of
 *   the ops is forward position lo + ref_lengths - 1 - i and the read's labels are complemented.  With i_c / j_c the reference /
 *   query index of column c as for wn_quality_profile, and [first, last] the first and last column whose op is 1 or 2:
 *     counts      [R][2][6] int32   [forward position][strand][A, G, C, T, deletion, other]: a column in [first, last] with op 1 or
 *                                   2 adds 1 at its position under the forward-strand base of its query label, or under `other`
 *                                   if the label is outside 1..4 or its qual is below min_qual (only with qual); with op 3 under
 *                                   `deletion`
 *     ins_lengths [R][max_ins + 1]  a maximal run of l op-4 columns inside (first, last) lies between forward positions p and
 *                                   p + 1 and adds 1 at [p][min(l, max_ins + 1) - 1]
 *     ins_bases   [R][max_ins][4]   the k-th label of that run IN FORWARD ORDER, k < max_ins, adds 1 at [p][k][base] unless it is
 *                                   outside 1..4 or below min_qual
 *     used        [B] int8          1 added; 0 skipped: strand < 0, ref_lengths == 0, keep[b] == 0 (nothing else of such a read is
 *                                   looked at), or no column with op 1 or 2; -1 bad
 *   The tables are ADDED INTO (32-bit integer atomics: a position holds fewer than 2^31 reads), never cleared.  Columns outside
 *   [first, last] enter nothing.  Two runs are bitwise identical.  A read that is not skipped is BAD when strand > 1, lo < 0,
 *   ref_lengths < 0, lo + ref_lengths > reference_len, query_lengths outside [0, max_query_len], ops_len outside [0, max_ops], an
 *   op is outside 1..4, the ops do not consume exactly ref_lengths and query_lengths labels, or a qual before query_lengths is
 *   above 93: it adds nothing and counts once in *bad (DEVICE int, caller-zeroed, may be NULL).  No bad value is used as an index.
 *   One workgroup per read, two passes over its ops; no workspace.
 *   wn_consensus_call: per position p, with c[k] = counts[p][0][k] + counts[p][1][k] and d = c[0] + ... + c[4], r = reference[p]
 *   (clamped to [0, 255]):
 *     d < min_depth: the call is r, flag LOW_DEPTH.  Else the candidate is the k in 0..4 of greatest c[k], ties first to r - 1 (if r
 *     is 1..4), then to the smallest k; if c[k] den > num d it is called (label k + 1, or 0 for k = 4: deleted; flag DELETION, or
 *     SUBSTITUTION if the label is not r), else the call is r, flag AMBIGUOUS.  alt_count [R][2]: counts[p][.][k] of the called k
 *     (of r - 1 where r was kept; 0 if r is no base).
 *     The insertion after p, with n the sum of ins_lengths[p]: if d >= min_depth and n den > num d, its length is min(l + 1,
 *     max_ins) for the fullest column l (ties to the smallest l), the label of slot k the fullest of ins_bases[p][k] (ties to the
 *     smallest), and the first slot without any count ends it; ins_len [R] bytes its length, ins_out [R][max_ins] bytes the labels
 *     then 0; flag INSERTION if the length is at least 1.
 *   call, flags [R] bytes.  tile_offsets [ceil(R / 256)] int32: the exclusive prefix sum over tiles of 256 positions of the emitted
 *   labels (call != 0) + ins_len; *total their sum (the length of the consensus).  Two launches: the calls with the tile totals, then
 *   one workgroup that scans the totals.
 *   wn_consensus_emit: offsets[p], p < R: where position p lands in the consensus; consensus: the labels -- the call if it is
 *   not 0, then the insertion after p -- of which only indices below `capacity` are written.
 * Checked before any launch, in this order.  WN_ERR_BAD_SHAPE: batch, max_query_len, max_ops or reference_len < 1, a negative
 * stride, min_qual, max_ins, num or capacity, min_depth or den < 1.  WN_ERR_UNSUPPORTED: batch > 65535, max_query_len > 8192, max_ops
 * > 65535 + 8192, reference_len > 2^26, min_qual > 93, max_ins > 8, den > 2^15, num > den.  WN_ERR_NULL: any pointer but qual, keep
 * and bad; ins_bases and ins_out only with max_ins > 0, consensus only with capacity > 0.  Nothing is read back or allocated. */
#define WN_CALL_LOW_DEPTH 1
#define WN_CALL_AMBIGUOUS 2
#define WN_CALL_SUBSTITUTION 4
#define WN_CALL_DELETION 8
#define WN_CALL_INSERTION 16
int wn_pileup(const unsigned char* ops, long long ops_stride, const int* ops_len, const int* lo, const int* ref_lengths,
              const int* strand, const int* query, long long query_stride, const int* query_lengths,
              const unsigned char* qual /* may be NULL */, long long qual_stride, const unsigned char* keep /* may be NULL */,
              int batch, int max_query_len, int max_ops, int reference_len, int min_qual, int max_ins, int* counts,
              int* ins_lengths, int* ins_bases /* with max_ins > 0 */, signed char* used, int* bad /* may be NULL */,
              wn_stream_t stream);
int wn_consensus_call(const int* counts, const int* ins_lengths, const int* ins_bases /* with max_ins > 0 */,
                      const int* reference, int reference_len, int max_ins, int min_depth, int num, int den, unsigned char* call,
                      unsigned char* ins_len, unsigned char* ins_out /* with max_ins > 0 */, unsigned char* flags, int* alt_count,
                      int* tile_offsets, int* total, wn_stream_t stream);
int wn_consensus_emit(const unsigned char* call, const unsigned char* ins_len, const unsigned char* ins_out /* with max_ins > 0 */,
                      const int* tile_offsets, int reference_len, int max_ins, int capacity, int* offsets,
                      int* consensus /* with capacity > 0 */, wn_stream_t stream);

/* ---- Indel left-alignment of op strings (wavenet_speech_amd/leftalign.py): the step between wn_pair_align and
 * wn_pileup that bcftools norm and GATK LeftAlignIndels run.  Every gap run of a row moves as far toward the START OF THE FORWARD
 * STRAND as the sequences allow, so that forward and reverse reads place the gap of a repeat alike.  Integer comparisons only; all
 * pointers are DEVICE pointers; tests/leftalign_ref.py holds the same definition as plain loops.
 *   Row b of ops_in (ops_stride bytes, ops_len[b] ops as wn_pair_align wrote them: 1 match, 2 mismatch, 3 reference label against a
 *   gap, 4 query label against a gap) aligns ref row b (ref_stride elements, ref_lengths[b] labels: the window IN READ ORIENTATION,
 *   as wn_pair_align took it) with query row b.  WALK ORIENTATION is wn_pileup's: the row as it stands on strand[b] = 0; the row
 *   and both sequences read back to front on strand[b] = 1 (no complement: labels are only compared).  In walk orientation, with
 *   [first, last] the first and last column whose op is 1 or 2 and i_c / j_c the reference / query index of column c, one PASS is:
 *     a run is a maximal stretch [c, c + l) of one gap op v strictly inside (first, last) (3s next to 4s are two runs); its barrier
 *     g is the last column before c whose op is 3 or 4, or `first` if there is none after it; with (seq, x) = (ref, i_c) for v = 3
 *     and (query, j_c) for v = 4, its shift s is the largest s <= c - g - 1 with seq[x - t] == seq[x - t + l] for t = 1..s; the
 *     run's columns become [c - s, c - s + l) and the s aligned columns it passed follow it with their ops in the same order.
 *   All runs of a pass are decided on the pass's input (their territories (g, c + l) are disjoint).  Passes repeat until one moves
 *   nothing or max_passes have run; the result goes to row b of ops_out (out_stride bytes) turned back into read orientation.  The
 *   multiset of ops, and so ops_len and every count of wn_pair_align, is kept; the score under affine costs never drops.
 *     passes  [B] int32  the passes that moved a run (0: the row was normalised already)
 *     settled [B] int8   1 a pass moved nothing: a fixed point; 0 max_passes ran and each moved something: the row is that many
 *                        passes along and still a valid alignment; -1 bad
 *   All max_ops bytes of a row are copied to ops_out first, whatever they hold.  A read with strand < 0 or ref_lengths == 0 is
 *   SKIPPED: nothing else of it is looked at, passes 0, settled 1.  A read that is not skipped is BAD when strand > 1, ref_lengths
 *   outside [1, max_ref_len], query_lengths outside [0, max_query_len], ops_len outside [0, max_ops], an op is outside 1..4, or
 *   the ops do not consume exactly ref_lengths and query_lengths labels (a poisoned pair of wn_pair_align is one): its row stays
 *   the copy, passes 0, settled -1, and it counts once in *bad (DEVICE int, caller-zeroed, may be NULL).  No bad value is used as
 *   an index.  One launch, one workgroup per read, every pass in place on ops_out; nothing is read back or allocated.  ops_out must
 *   not overlap ops_in.  workspace is not used (NULL and 0 are fine): there is no wn_gap_left_align_workspace_bytes.
 * Checked before the launch, in this order.  WN_ERR_BAD_SHAPE: batch, max_ref_len, max_query_len, max_ops or max_passes < 1, a
 * negative stride.  WN_ERR_UNSUPPORTED: batch > 65535, max_query_len > 8192, max_ref_len > 65535, max_ops > 65535 + 8192,
 * max_passes > 64.  WN_ERR_NULL: any pointer but workspace and bad.  WN_ERR_UNSUPPORTED: ops_out == ops_in. */
int wn_gap_left_align(const unsigned char* ops_in, long long ops_stride, const int* ops_len, const int* ref, long long ref_stride,
                      const int* ref_lengths, const int* query, long long query_stride, const int* query_lengths, const int* strand,
                      int batch, int max_ref_len, int max_query_len, int max_ops, int max_passes, unsigned char* ops_out,
                      long long out_stride, int* passes, signed char* settled, void* workspace /* may be NULL */,
                      size_t workspace_bytes, int* bad /* may be NULL */, wn_stream_t stream);

/* ---- Genotype likelihoods and diploid calls (wavenet_speech_amd/genotype.py): what bcftools call and GATK
 * do after the pileup -- every base weighed by its quality, and a genotype of two alleles per position with its quality.  Integer
 * arithmetic only; all pointers are DEVICE pointers except weights_host.  tests/genotype_ref.py holds the same definitions as plain
 * loops.
 *   weights_host [3][94] int32 on the HOST: rows HOM, HET, MIS, columns qual 0..93, in units of 1/scale Phred, every entry in
 *   [0, 2^20].  It is read during the call and travels to the kernel by value: no allocation, no copy.  The model (which weights)
 *   is the caller's: genotype_weights() of the Python surface builds HOM = -10 log10(1 - e), HET = -10 log10((1 - e) / 2 + e / 6),
 *   MIS = -10 log10(e / 3) with e = min(10^(-q / 10), 3 / 4), times scale, rounded.
 *   wn_pileup_evidence: the walk of wn_pileup -- the same arguments, ops, end columns, orientation and complement, the same
 *   skipped and bad reads, the same `used` and *bad:
 *     evidence [R][5][3] int64   [forward position][A, G, C, T, deletion][HOM, HET, MIS]: a column that wn_pileup counts under base
 *                                k adds weights[.][min(q, cap[b])] at [p][k][.], q the base's qual, or flat_qual without qual; a
 *                                deletion column adds weights[.][min(gap_qual, cap[b])] at [p][4][.].  cap [B] bytes (the mapping
 *                                quality as a ceiling; NULL: none).  min_qual is compared with the UNCAPPED qual, as in wn_pileup:
 *                                the same columns go to `other` in both.  `other` and insertion columns add nothing.
 *   The table is ADDED INTO (64-bit integer atomics: sums stay below 2^51 for fewer than 2^31 reads), never cleared.  Two runs are
 *   bitwise identical.  One workgroup per read, two passes over its ops; no workspace.
 *   wn_genotype_call: per position p, with E = evidence[p], d the depth of wn_consensus_call from counts[p], r = reference[p]
 *   (clamped to [0, 255]), over the 15 unordered pairs (a <= b) of allele indices 0..4 in lexicographic order:
 *     L(a, a) = E[a][HOM] + sum over x != a of E[x][MIS];  L(a, b) = E[a][HET] + E[b][HET] + sum over x not in {a, b} of E[x][MIS]
 *     cost = L + alt_prior for every genotype but (r - 1, r - 1); with r outside 1..4 there is no such genotype and no prior is added
 *     costs   [R][15] int64 (may be NULL)
 *     alleles [R][2] bytes: the labels (k + 1, or 0 for the deletion) of the genotype least by (cost, is not (r - 1, r - 1), index),
 *                           in allele-index order;  gq [R] int32: the second-least cost minus the least;  qual [R] int32: the cost
 *                           of (r - 1, r - 1) minus the least; both clamped to 2^31 - 1
 *     flags   [R] bytes: SUBSTITUTION if a called allele is a base other than r, DELETION if one is the deletion, HET if the two
 *                           differ.  d < min_depth (looked at first): alleles (r, r), gq = qual = 0, flags LOW_DEPTH.  Else r
 *                           outside 1..4: alleles (r, r), gq = qual = 0, no flag.  costs are written in either case.
 *     The insertion after p, with n the sum of ins_lengths[p], m = max(d - n, 0) and HOM, HET, MIS the weights of gap_qual:
 *     c0 = n MIS + m HOM, c1 = (n + m) HET + alt_prior, c2 = n HOM + m MIS + alt_prior (64-bit products).  ins_copies [R] bytes: the
 *     index of the least, ties to fewer copies; ins_gq: the second least minus the least; ins_qual: c0 minus the least (clamped as
 *     above).  With copies >= 1 the length and the labels are wn_consensus_call's (the fullest length column, the fullest base per
 *     slot, the first empty slot ends it) without its fraction test, to ins_len [R] and ins_out [R][max_ins] bytes.  d < min_depth,
 *     or copies >= 1 with an empty sequence: copies, length, ins_gq and ins_qual are 0.  Flags INSERTION with copies >= 1, and
 *     INS_HET with copies == 1, whatever r is.
 *   One launch, one position per thread; nothing is read back or allocated.
 * Checked before any launch, in this order.  WN_ERR_BAD_SHAPE: batch, max_query_len, max_ops or reference_len < 1, a negative
 * stride, min_qual, flat_qual, gap_qual or max_ins, min_depth < 1.  WN_ERR_UNSUPPORTED: batch > 65535, max_query_len > 8192, max_ops
 * > 65535 + 8192, reference_len > 2^26, min_qual, flat_qual or gap_qual > 93, max_ins > 8, alt_prior outside [0, 2^30].
 * WN_ERR_NULL: any pointer but qual, keep, cap, bad and costs; ins_bases and ins_out only with max_ins > 0.  WN_ERR_UNSUPPORTED: a
 * weight outside [0, 2^20] (the table is read only once it is known not to be NULL). */
#define WN_CALL_HET 32
#define WN_CALL_INS_HET 64
int wn_pileup_evidence(const unsigned char* ops, long long ops_stride, const int* ops_len, const int* lo, const int* ref_lengths,
                       const int* strand, const int* query, long long query_stride, const int* query_lengths,
                       const unsigned char* qual /* may be NULL */, long long qual_stride,
                       const unsigned char* keep /* may be NULL */, int batch, int max_query_len, int max_ops, int reference_len,
                       const unsigned char* cap /* may be NULL */, const int* weights_host /* 3 * 94, HOST */, int flat_qual,
                       int gap_qual, int min_qual, long long* evidence, signed char* used, int* bad /* may be NULL */,
                       wn_stream_t stream);
int wn_genotype_call(const long long* evidence, const int* counts, const int* ins_lengths,
                     const int* ins_bases /* with max_ins > 0 */, const int* reference, int reference_len, int max_ins,
                     int min_depth, int alt_prior, const int* weights_host /* 3 * 94, HOST */, int gap_qual,
                     unsigned char* alleles, int* gq, int* qual, unsigned char* flags, unsigned char* ins_copies,
                     unsigned char* ins_len, unsigned char* ins_out /* with max_ins > 0 */, int* ins_gq, int* ins_qual,
                     long long* costs /* may be NULL */, wn_stream_t stream);

/* ---- Read-backed phasing and haplotags (wavenet_speech_amd/phase.py): what WhatsHap, longshot or HapCUT2 do
 * after the calls -- the alleles of neighbouring heterozygous sites linked through the reads that span them, and a haplotype tag
 * per read.  Integer arithmetic only; all pointers are DEVICE pointers.  tests/phase_ref.py holds the same definitions as plain
 * loops.
 *   A site s (0 <= s < n_sites) is a heterozygous position: site_of [R] int32 holds the site of a position or -1, alleles
 *   [n_sites][2] bytes its two called labels (0: deleted), pos [n_sites] int32 its position, ascending.
 *   An OBSERVATION of a read: a column that wn_pileup_evidence adds for (the same reads, arguments, ops, end columns, orientation,
 *   complement, min_qual rule, skipped and bad reads as wn_pileup) at a position with site_of >= 0.  It shows the label k (1..4, or 0
 *   for a deletion column) with the weight q' = min(q, cap[b]), q the base's qual, flat_qual without qual, gap_qual for a deletion;
 *   x = 0 if k == alleles[s][0], else 1 if k == alleles[s][1], else NEITHER.
 *   wn_phase_links: observed [n_sites][3] int32 += 1 at [s][x] (column 2: neither); links [n_sites][reach][2] int64: for every pair
 *   of observations of one read at sites s - d and s, 1 <= d <= reach, neither of them NEITHER, += min(q'(s - d), q'(s)) at
 *   [s][d - 1][x(s - d) xor x(s)] (0 cis, 1 trans).  Both tables are ADDED INTO (integer atomics), never cleared; two runs are
 *   bitwise identical.  used [B] and *bad as wn_pileup writes them.  One workgroup per read, two passes over its ops.
 *   wn_phase_chain: per site, margin_d = |cis - trans| of links[s][d - 1] for d in 1..min(reach, s), d* the greatest (ties to the
 *   least d).  s == 0 or margin_d* < min_margin: a root, parent[s] = s, flip[s] = 0, margin[s] = 0; else parent[s] = s - d*, flip[s]
 *   = (trans > cis), margin[s] = min(margin_d*, 2^31 - 1).  root[s]: the root of s's tree; parity[s]: the xor of the flips on the way
 *   there; ps[s] = pos[root[s]]; set_size[s]: the sites of that tree.  work: 2 * n_sites int32.  3 + ceil(log2 n_sites) launches
 *   (pointer doubling), nothing is read back.
 *   wn_haplotag: per read, over its observations with x in {0, 1} at sites with set_size > 1: its set is root[s] of the one with
 *   the greatest q' (ties to the least s); weight [B][2] int32: the sum of q' of those in that set at [x xor parity[s]]; n_observed
 *   [B][2] int32: how many lie in that set, and in others; hp [B] bytes: 1 if weight[0] > weight[1], 2 if less, else 0; ps [B] int32:
 *   pos[root] or -1 without such an observation.  A skipped or bad read: hp 0, ps -1, zeros; bad ones are counted in *bad.
 * Checked before any launch, in this order.  WN_ERR_BAD_SHAPE: batch, max_query_len, max_ops, reference_len, n_sites or reach < 1, a
 * negative stride, min_qual, flat_qual, gap_qual or min_margin.  WN_ERR_UNSUPPORTED: batch > 65535, max_query_len > 8192, max_ops >
 * 65535 + 8192, reference_len > 2^26, min_qual, flat_qual or gap_qual > 93, reach > 8, n_sites > reference_len (wn_phase_chain:
 * > 2^26).  WN_ERR_NULL: any pointer but qual, keep, cap and bad. */
int wn_phase_links(const unsigned char* ops, long long ops_stride, const int* ops_len, const int* lo, const int* ref_lengths,
                   const int* strand, const int* query, long long query_stride, const int* query_lengths,
                   const unsigned char* qual /* may be NULL */, long long qual_stride,
                   const unsigned char* keep /* may be NULL */, int batch, int max_query_len, int max_ops, int reference_len,
                   const unsigned char* cap /* may be NULL */, int flat_qual, int gap_qual, int min_qual, const int* site_of,
                   const unsigned char* alleles, int n_sites, int reach, long long* links, int* observed, signed char* used,
                   int* bad /* may be NULL */, wn_stream_t stream);
int wn_phase_chain(const long long* links, const int* pos, int n_sites, int reach, int min_margin, int* parent,
                   unsigned char* flip, int* margin, int* root, unsigned char* parity, int* ps, int* set_size, int* work,
                   wn_stream_t stream);
int wn_haplotag(const unsigned char* ops, long long ops_stride, const int* ops_len, const int* lo, const int* ref_lengths,
                const int* strand, const int* query, long long query_stride, const int* query_lengths,
                const unsigned char* qual /* may be NULL */, long long qual_stride, const unsigned char* keep /* may be NULL */,
                int batch, int max_query_len, int max_ops, int reference_len, const unsigned char* cap /* may be NULL */,
                int flat_qual, int gap_qual, int min_qual, const int* site_of, const unsigned char* alleles, int n_sites,
                const int* pos, const int* root, const unsigned char* parity, const int* set_size, unsigned char* hp, int* ps,
                int* weight, int* n_observed, int* bad /* may be NULL */, wn_stream_t stream);

/* ---- Realignment of reads against the called haplotypes (wavenet_speech_amd/realign.py): what GATK's indel
 * realigner and HaplotypeCaller, longshot and margin do after the calls -- a read is aligned against the two haplotypes the calls
 * and their phasing spell, the better score says which one it lies on, and that alignment is carried back to reference
 * coordinates.  The DP is wn_pair_align's, run by the caller once per haplotype; these are the two steps around it.  Integer
 * arithmetic only; all pointers are DEVICE pointers.  tests/realign_ref.py holds the same definitions as plain loops.
 *   A HAPLOTYPE h (0 <= h < haplotypes) over a reference of reference_len positions: call [haplotypes][R] bytes, the label it
 *   carries at forward position p (0: deleted); ins_len [haplotypes][R] bytes and ins_bases [haplotypes][R][max_ins] bytes, the
 *   insertion it carries after p.  reference [R] int32: the reference's labels.
 *   wn_haplotype_windows: for read b with the window [lo[b], lo[b] + n), n = ref_lengths[b], and haplotype h, two rows IN READ
 *   ORIENTATION.  In forward order position p gives, with v = call[h][p]: v == 0: op 3 and no label; else the label v and op 1 if
 *   v == reference[p], else op 2; then, only for p < lo + n - 1, ins_len[h][p] labels with op 4 (the insertion after the window's
 *   last position is outside the window, as in wn_pileup).  On strand[b] == 1 both rows are reversed and labels 1..4 complemented
 *   (5 - v), other labels kept: wn_pileup's orientation, so the label row is wn_pair_align's `ref`.
 *     labels  [haplotypes][B][max_hap_ops] int32, lengths [haplotypes][B] int32: the haplotype's labels over the window
 *     ops     [haplotypes][B][max_hap_ops] bytes, ops_len [haplotypes][B] int32: haplotype against reference: 1 / 2 both, 3 a
 *             reference label the haplotype lacks, 4 a haplotype label the reference lacks
 *     used    [B] int8: 1 written, 0 skipped, -1 bad
 *   Both rows are zero behind their lengths.  A read with strand < 0 or ref_lengths == 0 is SKIPPED: lengths 0, used 0.  A read that
 *   is not skipped is BAD when strand > 1, lo < 0, ref_lengths < 0, lo + n > R, an ins_len of its window is above max_ins, or a row
 *   of ANY of its haplotypes needs more than max_hap_ops ops: lengths 0 on every haplotype, used -1, counted once in *bad (DEVICE
 *   int, caller-zeroed, may be NULL).  No bad value is used as an index; a row is never truncated.  One launch, one workgroup per
 *   (read, haplotype), two passes over the window; no workspace, nothing is read back.
 *   wn_lift_ops: row b of a_ops[pick[b]] is A, the read against the haplotype as wn_pair_align wrote it (1 / 2 both, 3 a haplotype
 *   label only, 4 a read label only); row b of hap_ops[pick[b]] is Hh, wn_haplotype_windows' row.  Row (h, b) of a_ops is at a_ops +
 *   h * a_hap_stride + b * a_stride with a_ops_len [haplotypes][B]; hap_ops likewise, with hap_lengths [haplotypes][B] the
 *   haplotype's labels.  Their composition, the read against its reference window, is the sequential loop
 *     loop: while Hh's next op is 3: emit 3, take it;  while A's next op is 4: emit 4, take it;  if both rows are used up: stop;
 *           a = A's next op is 1 or 2 (else 3), g = Hh's next op is 1 or 2 (else 4), take both (they share one haplotype label);
 *           a and g: emit 1 if ref[i] == query[j] else 2 (i, j the reference and read labels emitted so far: compared afresh);
 *           a only: emit 4;  g only: emit 3;  neither: emit nothing
 *   written to row b of ops (ops_stride bytes, zero behind ops_len[b]) with stats [B][4] int32 = matches, mismatches, gap columns,
 *   length and score [B] int32 in half units under the affine costs with wn_pair_align's end-gap rule: a run of one gap op costs
 *   gap_open + (n - 1) gap_extend, and with end_gaps_free the runs that touch either end of the row cost nothing.  The result
 *   consumes exactly ref_lengths[b] and query_lengths[b] labels: it is an op row as wn_pair_align writes one.
 *   used[b] == 0 (a skipped window) passes through: ops_len 0, stats and score 0.  Otherwise a row is BAD when used[b] < 0, pick[b]
 *   outside [0, haplotypes), ref_lengths outside [1, max_ref_len], query_lengths outside [0, max_query_len], a length of A or Hh
 *   outside its row, hap_lengths outside [0, max_hap_len], an op outside 1..4, A does not consume exactly hap_lengths and
 *   query_lengths labels, Hh not exactly ref_lengths and hap_lengths, or the result would pass max_ops: ops_len 0, stats -1, score
 *   -2^31 (wn_pair_align's poison), counted once in *bad.  One launch, one workgroup per read.  workspace: wn_lift_ops_workspace_bytes (three int32 per
 *   haplotype index and read; 0 for a bad or unsupported shape), 4-byte aligned.
 * Checked before the launch, in this order.  WN_ERR_BAD_SHAPE: haplotypes, batch, reference_len, max_hap_ops, max_hap_len,
 * a_max_ops, max_ref_len, max_query_len or max_ops < 1, max_ins < 0, a negative stride, end_gaps_free not 0 or 1.
 * WN_ERR_UNSUPPORTED: haplotypes > 2, batch > 65535, reference_len > 2^26, max_ins > 8, max_hap_ops, max_hap_len or max_ref_len >
 * 65535, max_query_len > 8192, a_max_ops or max_ops > 65535 + 8192, the costs outside wn_pair_align's limits.  WN_ERR_NULL: any
 * pointer but bad; ins_bases only with max_ins > 0.  WN_ERR_WORKSPACE: workspace_bytes too small or workspace misaligned. */
int wn_haplotype_windows(const unsigned char* call, const unsigned char* ins_len, const unsigned char* ins_bases /* with max_ins > 0 */,
                         const int* reference, const int* lo, const int* ref_lengths, const int* strand, int haplotypes, int batch,
                         int reference_len, int max_ins, int max_hap_ops, int* labels, int* lengths, unsigned char* ops, int* ops_len,
                         signed char* used, int* bad /* may be NULL */, wn_stream_t stream);
size_t wn_lift_ops_workspace_bytes(int batch, int max_hap_len);
int wn_lift_ops(const unsigned char* a_ops, long long a_hap_stride, long long a_stride, const int* a_ops_len, int a_max_ops,
                const unsigned char* hap_ops, long long hap_hap_stride, long long hap_stride, const int* hap_ops_len,
                const int* hap_lengths, int max_hap_ops, int max_hap_len, const signed char* used, const int* pick, const int* ref,
                long long ref_stride, const int* ref_lengths, const int* query, long long query_stride, const int* query_lengths,
                int haplotypes, int batch, int max_ref_len, int max_query_len, int max_ops, int match, int mismatch, int gap_open,
                int gap_extend, int end_gaps_free, unsigned char* ops, long long ops_stride, int* ops_len, int* score, int* stats,
                void* workspace, size_t workspace_bytes, int* bad /* may be NULL */, wn_stream_t stream);

/* ---- Banded global pairwise alignment (wavenet_speech_amd.banded_align): wn_pair_align's recurrence, tie
 * rules, end-cell rule and op rows inside a per-pair stripe of diagonals.  ref, query, their strides and lengths, the costs,
 * end_gaps_free, score, stats, ops, ops_len and bad: as wn_pair_align takes them.  diag_lo, diag_hi: DEVICE int32 [B].
 *   Cell (i, j), 0 <= i <= N_b, 0 <= j <= M_b, is IN BAND iff diag_lo[b] <= j - i <= diag_hi[b]; the width is
 *   diag_hi - diag_lo + 1.  H, E and F of a cell that is not in band are -infinity wherever they are read; in-band cells with
 *   i, j >= 1 follow wn_pair_align's recurrence, candidate order and tie rules; in-band border cells take the full matrix's
 *   border values, whether or not (0, 0) is in band.
 *   End cell: (N, M) with end gaps penalised; with end_gaps_free the candidates (N, M), (N, M-1) .. (N, 0), (N-1, M) .. (0, M) in
 *   this order, in-band cells only: the first is taken and a later one replaces it only if strictly greater.
 *   NO ALIGNMENT (not an error): with end_gaps_free the stripe misses the rectangle (diag_lo > M_b or diag_hi < -N_b); with end
 *   gaps penalised (N_b, M_b) is not in band.  Then status 0, score INT_MIN, stats 0, ops_len 0, edge_hits 0; not counted in *bad.
 *   The trace and the end gaps are wn_pair_align's: an op row that consumes exactly N_b and M_b labels.  If every cell of the
 *   full matrix's traced path is in band, score, stats and ops equal wn_pair_align's; for any stripe the score is <= its score.
 *   status     [B] int8: 1 aligned, 0 no alignment, -1 a bad pair
 *   edge_hits  [B] int32 or NULL: the path cells (the cell where the trace stopped, then the cell after every op up to the end
 *              cell) with j - i == diag_lo or j - i == diag_hi; 0 when the stripe never held the path; -1 for a bad pair
 * A bad pair -- a length negative or above its maximum, diag_lo > diag_hi, or a width above max_band -- is poisoned as
 * wn_pair_align poisons one (score INT_MIN, stats -1, ops_len 0), has status -1 and counts once in *bad; no bad value is used
 * as an index.  ops == NULL and stats == NULL is the score-only form: no workspace, no trace, and edge_hits must be NULL.
 * workspace: wn_banded_align_workspace_bytes (0 for a bad or unsupported shape), 16-byte aligned:
 *   round_up(batch * (max_ref_len + max_query_len + 1) * ceil(max_band / 8) * 2, 16)       4 bits per in-band cell of a step
 *   + batch * round_up(max_ref_len + max_query_len, 16)                                      the path's ops, back to front
 * One launch, one workgroup per pair; widths up to 512 run in one wave, wider ones in 256 threads.  Nothing is read back.
 * Checked on the host in this order: batch, max_ref_len, max_query_len, max_band < 1 (WN_ERR_BAD_SHAPE); max_band > 2048,
 * max_ref_len > 65535, max_query_len > 65535, batch > 65535, the costs outside wn_pair_align's limits (WN_ERR_UNSUPPORTED); a
 * required pointer NULL, ops without ops_len or the reverse, edge_hits in the score-only form (WN_ERR_NULL); the workspace
 * (WN_ERR_WORKSPACE).  Nothing is launched then.  The tools that walk op rows keep their own limit of 8192 query labels. */
size_t wn_banded_align_workspace_bytes(int batch, int max_ref_len, int max_query_len, int max_band);
int wn_banded_align(const int* ref, long long ref_stride, const int* ref_lengths, const int* query, long long query_stride,
                    const int* query_lengths, const int* diag_lo, const int* diag_hi, int batch, int max_ref_len, int max_query_len,
                    int max_band, int match, int mismatch, int gap_open, int gap_extend, int end_gaps_free, int* score,
                    int* stats /* may be NULL */, unsigned char* ops /* may be NULL */, int* ops_len /* with ops */,
                    signed char* status, int* edge_hits /* may be NULL */, void* workspace, size_t workspace_bytes,
                    int* bad /* may be NULL */, wn_stream_t stream);

/* ---- CIGAR runs from op rows and back (wavenet_speech_amd.cigar_runs / cigar_ops): what SAM and BAM carry
 * of an alignment, written from and turned into the op rows of wn_pair_align.  Ops, walk index w, i, j, rev, the header and the
 * column validity are those of wn_pileup (csrc/wn_opscan.h); the window condition is wn_pileup's, lo >= 0 and lo + n_ref <= R.
 * first / last are the first and last aligned (op 1 or 2) walk index.  The walk reverses strand 1, so everything below is in
 * FORWARD reference orientation.
 *   wn_cigar_encode: op row -> runs.  ops .. query_lengths, keep, batch, max_query_len, max_ops, reference_len: as wn_pileup takes
 *   them (the query labels are not needed).  With i(w), j(w) the labels consumed before walk index w:
 *     pos = lo + i(first), 0-based;  ref_span = i(last) - i(first) + 1;  clip_front = j(first);  clip_back = n_query - j(last) - 1;
 *     nm = the columns of [first, last] with op 2, 3 or 4.
 *   Columns outside [first, last] enter nothing, as with wn_pileup: an op 4 there is soft-clipped, an op 3 only moves pos or
 *   shortens the span.  The runs, in order: (S, clip_front) if clip_front > 0; the run-length encoding of the columns first..last
 *   by class, op 1 -> '=', op 2 -> 'X' (both 'M' with eqx == 0), op 4 -> 'I', op 3 -> 'D'; (S, clip_back) if clip_back > 0.
 *     cigar    row b at cigar + b * cigar_stride (elements): one uint32 per run, len << 4 | code, BAM's codes M 0, I 1, D 2, N 3,
 *              S 4, H 5, P 6, = 7, X 8; n_cigar[b] runs, zero behind them up to max_cigar in every outcome
 *     fields   [B][5] int32: pos, ref_span, clip_front, clip_back, nm
 *     used     [B] int8: 1 written.  0 skipped: strand < 0, ref_lengths == 0, keep[b] == 0, or no aligned column; n_cigar 0, pos
 *              -1, the other fields 0.  -1 bad: exactly the rows wn_pileup calls bad for the same ops, lengths, strand and window
 *              (there is no qual); fields as for skipped; counted once in *bad (DEVICE int, caller-zeroed, may be NULL).  -2 the
 *              row needs more than max_cigar runs: nothing of it is written (a row is never truncated), n_cigar[b] holds the
 *              number needed, the fields are filled; counted once in *bad.
 *   A row of n_query labels has at most 2 n_query + 3 runs: deletion runs are separated by query-consuming columns.
 *   wn_cigar_decode: runs -> op row.  pos, strand [B]; reference [reference_len] labels; query row b at query + b * query_stride in
 *   READ orientation with query_lengths[b] labels.  The runs are walked in forward orientation: M, = and X emit one column per
 *   base, op 1 if reference[pos + i] equals the forward query label (on strand 1: 5 - v of a label v in 1..4, other labels kept,
 *   taken at n_query - 1 - j), else op 2; I and S emit op 4; D emits op 3; H, P and a run of length 0 emit nothing.  The row is
 *   written in READ orientation (reversed on strand 1), zero behind ops_len up to max_ops; ref_lengths = the reference labels
 *   consumed, stats [B][4] = matches, mismatches, gap columns, length as wn_pair_align counts them; the window's lo is pos.  The
 *   result is an op row as wn_pair_align writes one: it consumes exactly ref_lengths and query_lengths labels.
 *     used     [B] int8: 1 written.  0 skipped: strand < 0 or n_cigar == 0; ops_len, ref_lengths and stats 0.  -1 bad: strand > 1,
 *              n_cigar outside [0, max_cigar], pos < 0, query_lengths outside [0, max_query_len] (nothing else of such a read is
 *              looked at); a code above 8 or code N; more than max_ops columns; no reference label consumed; pos + the labels
 *              consumed > reference_len; the query labels consumed differ from query_lengths; with strict an '=' column whose
 *              labels differ or an 'X' column whose labels are equal.  Then ops_len 0, ref_lengths 0, stats -1, the row zero,
 *              counted once in *bad.
 *   No bad value is used as an index; a run's length enters the sums clamped to max_ops + 1 and the sums saturate, so nothing
 *   wraps.  workspace: wn_cigar_decode_workspace_bytes = round_up(batch * 3 * max_cigar * 4, 16), the scanned offsets of the runs
 *   (0 for a bad or unsupported shape), 16-byte aligned.
 * One launch each, one workgroup per read, nothing is read back.  Checked on the host in this order.  WN_ERR_BAD_SHAPE: batch,
 * max_query_len, max_ops, reference_len or max_cigar < 1, a negative stride, eqx / strict not 0 or 1.  WN_ERR_UNSUPPORTED: batch >
 * 65535, max_query_len > 8192, max_ops > 65535 + 8192, reference_len > 2^26, max_cigar > 65535 (BAM's own limit).  WN_ERR_NULL:
 * any pointer but keep and bad.  WN_ERR_WORKSPACE (wn_cigar_decode): workspace_bytes too small or the workspace misaligned. */
int wn_cigar_encode(const unsigned char* ops, long long ops_stride, const int* ops_len, const int* lo, const int* ref_lengths,
                    const int* strand, const int* query_lengths, const unsigned char* keep /* may be NULL */, int batch,
                    int max_query_len, int max_ops, int reference_len, int eqx, int max_cigar, unsigned* cigar,
                    long long cigar_stride, int* n_cigar, int* fields /* [B][5]: pos, ref_span, clip_front, clip_back, nm */,
                    signed char* used, int* bad /* may be NULL */, wn_stream_t stream);
size_t wn_cigar_decode_workspace_bytes(int batch, int max_cigar);
int wn_cigar_decode(const unsigned* cigar, long long cigar_stride, const int* n_cigar, const int* pos, const int* strand,
                    const int* reference, int reference_len, const int* query, long long query_stride, const int* query_lengths,
                    int batch, int max_cigar, int max_query_len, int max_ops, int strict, unsigned char* ops, long long ops_stride,
                    int* ops_len, int* ref_lengths, int* stats, signed char* used, void* workspace, size_t workspace_bytes,
                    int* bad /* may be NULL */, wn_stream_t stream);

/* ======================================================================================================================
 * Half-precision-MFMA modes of the same path (opt-in; the entry points above stay exact fp32).
 *
 *   WN_F16X3  every operand is split into two fp16 planes (hi, lo); each product is hi*hi + hi*lo + lo*hi on
 *             v_mfma_f32_32x32x16_f16 with fp32 accumulation: 22-bit operands at 3/16 of the fp32 MFMA cost (within 1e-4 of the
 *             fp32 path on conditioned models; 3-4x further from fp64 than fp32 on the reference's ill-conditioned random init).
 *   WN_F16 / WN_BF16   one plane of fp16 / bf16 storage, one MFMA per product, fp32 accumulation
 *             (the dtypes BASELINE.json configs[4] / configs[1] name).
 *
 * "Half series" layout of every activation:  T buf[B][P][G][ld][8],  P = planes (2 for F16X3), G = round_up(C,32)/8;
 *   sample (b, c, t) of plane p at ((((b*P + p)*G + c/8)*ld + halo + t)*8 + c%8.  Eight channels of one time step are one
 *   16-byte unit = one MFMA operand fragment; a dilated tap is the same unit stream at another start.  Halos, the tail up to
 *   ld (= 2*halo + round_up(L, 256)) and the pad channels MUST be zero on input and are kept zero.
 * Power-of-two scales (exact): the residual stream (x, r_out) is stored as value * wn_hseries_residual_scale() (= 1/16, so
 *   fp16 holds |r| up to 1e6); ta, sg, z as is; every gradient series as value * s, where s is one DEVICE scalar per
 *   backward call chosen by the caller (pass 1/s as dyn_inv_scale where results leave the half domain).
 * fp16 stores that overflow (|v| > 65504) set *overflow_flag (a DEVICE unsigned the caller zeroed; may be NULL) to 1.
 * Everything else (ownership, streams, status codes, dr == NULL for the last block) is as for the fp32 entry points, whose
 * reference counterparts (modules/block.py:54-82, modules/wavenet.py:98-100) these replace in the same way. */
typedef enum wn_precision { WN_F32 = 0, WN_F16X3 = 1, WN_F16 = 2, WN_BF16 = 3 } wn_precision;

int wn_hseries_layout(int length, int max_abs_offset, int* ld, int* halo);
size_t wn_hseries_bytes(int precision, int batch, int channels, int ld);
float wn_hseries_residual_scale(void);
/* dense fp32 [B][C][L] -> half series, multiplied by scale * (dyn_scale ? *dyn_scale : 1).  Only the valid window is written. */
int wn_hseries_load(int precision, const float* dense, void* series, int batch, int channels, int length, int ld, int halo,
                    float scale, const float* dyn_scale, unsigned* overflow_flag, wn_stream_t stream);

size_t wn_hblock_packed_bytes(const wn_block_shape* s, int precision);
int wn_hblock_pack(const wn_block_shape* s, int precision, const wn_block_params* p, void* packed, wn_stream_t stream);
/* the same; *overflow_flag (DEVICE unsigned, caller-zeroed, may be NULL) is set when a weight leaves fp16's range after its
 * built-in scale (256 * w / input scale: |w| >= 16 for gate / projection weights) -- the gate would saturate silently otherwise */
int wn_hblock_pack_checked(const wn_block_shape* s, int precision, const wn_block_params* p, void* packed, unsigned* overflow_flag,
                           wn_stream_t stream);
/* x, r_out (nullable), sg (nullable: inference), z: half series.  z = tanh(a) sigmoid(g) and sg = sigmoid(g) are what the
 * backward pass needs (the tanh is recovered as z / sg: one tensor less to write and to keep).  skip_dense (nullable): dense
 * fp32 [B][Ms][L] that receives (skip_accumulate: += ) W_skip z + b_skip -- the per-block form used for inference.
 * Blocks of <= 128 channels with two taps run as ONE launch in the one-plane modes (wn_hblock_forward_is_fused() == 1: gate,
 * z and both products fused, z never leaves the chip between them -- the span modules/block.py:65-79 of the reference); there z
 * may be NULL when sg is NULL (inference: nothing needs it).  The fused kernel writes to a 1 KiB scratch line inside `packed`. */
int wn_hblock_forward_is_fused(const wn_block_shape* s, int precision);
int wn_hblock_forward(const wn_block_shape* s, int precision, const void* packed, const void* x, void* r_out,
                      float* skip_dense, int skip_accumulate, void* sg, void* z, unsigned* overflow_flag,
                      wn_stream_t stream);
size_t wn_hskipsum_packed_bytes(const wn_skipsum_shape* s, int precision);
int wn_hskipsum_pack(const wn_skipsum_shape* s, int precision, const float* const* w_skip, const float* bias_total,
                     void* packed, wn_stream_t stream);
/* z[l]: half series of every block; skip_dense: dense fp32 [B][Ms][L] */
int wn_hskipsum_forward(const wn_skipsum_shape* s, int precision, const void* packed, const void* const* z,
                        float* skip_dense, int accumulate, wn_stream_t stream);
/* dr (nullable), dskip, z, sg (the forward pass's), da, dg: half series (gradients carry the scale s).  The input gradient goes
 * either to the half series dx (scaled by s, the next block's dr) or to dense fp32 dx_dense [B][Ci][L] multiplied by
 * *dyn_inv_scale.  Blocks that take the fused forward and whose skip path is as wide as the block (<= 128 channels, one-plane
 * modes) run dz and the series dx as column-owner streaming kernels (hcol_kernel, csrc/wn_col_dev.h: the autograd of the
 * reference's modules/block.py:65-79 with the activations read straight from the series into registers); same arguments, same
 * packed weights.  The 1x1 wn_hconv_*_series calls below do likewise. */
int wn_hblock_backward_data(const wn_block_shape* s, int precision, const void* packed, const void* dr, const void* dskip,
                            const void* z, const void* sg, void* da, void* dg, void* dx, float* dx_dense,
                            const float* dyn_inv_scale, unsigned* overflow_flag, wn_stream_t stream);
size_t wn_hblock_wgrad_workspace_bytes(const wn_block_shape* s, int precision);
/* gradients in PyTorch layouts, fp32, multiplied by *dyn_inv_scale (and by the residual-stream scale where x is an operand) */
int wn_hblock_backward_weights(const wn_block_shape* s, int precision, const void* x, const void* z, const void* da,
                               const void* dg, const void* dr, const void* dskip, const wn_block_params* grads,
                               const float* dyn_inv_scale, void* workspace, size_t workspace_bytes, wn_stream_t stream);

/* The convolutions AROUND the block stack kept in the half series (the callers either side of the path; reference
 * modules/wavenet.py:67-71,103 output_stack, raw_ctcnet.py:57-61,89-93,128,148 feature_layer / output_block): LeakyReLU and the
 * 1x1 convs run without dense fp32 round trips between them.
 *   wn_hskipsum_forward_series     out = leaky(skips_sum) * out_scale as a half series (instead of the dense fp32 of
 *                                  wn_hskipsum_forward): the activated input of the output block's first conv
 *   wn_hconv_forward_series        y = leaky(conv(x) + b) * out_scale, series in, series out (leaky_slope 1 = no activation)
 *   wn_hconv_backward_data_series  dx = (W^T dy) * leaky'(act): act = the conv's stored (activated) input, NULL = no activation
 * Weight gradients: wn_hconv_backward_weights (series operands already).  out_scale is the scale the stored tensor carries
 * (wn_hseries_residual_scale() by convention, so that fp16 cannot overflow); pack the consumer with that input_scale. */
int wn_hskipsum_forward_series(const wn_skipsum_shape* s, int precision, const void* packed, const void* const* z, void* out_series,
                               float out_scale, float leaky_slope, unsigned* overflow_flag, wn_stream_t stream);
int wn_hconv_forward_series(const wn_conv_shape* s, int precision, const void* packed, const void* x, void* y_series, float out_scale,
                            float leaky_slope, unsigned* overflow_flag, wn_stream_t stream);
int wn_hconv_backward_data_series(const wn_conv_shape* s, int precision, const void* packed, const void* dy, const void* act,
                                  float leaky_slope, void* dx_series, unsigned* overflow_flag, wn_stream_t stream);

/* dx of `upper` and dz (-> da, dg) of `lower`, the block directly below it in the stack, in ONE launch: dz is pointwise in time
 * and its dr operand is the dx tile the same wave has just computed, so it goes from the MFMA result registers straight back into
 * the MFMA (csrc/wn_col2.hip: the autograd of two consecutive `out, skip = block(out)` steps of modules/wavenet.py:98-100).
 * dx_upper is still written (the lower block's weight gradients read it as their dr).  Only for pairs for which
 * wn_hblock_backward_pair_is_fused() == 1 (both blocks take the column-owner kernels, equal widths and geometry); otherwise
 * WN_ERR_UNSUPPORTED and the caller uses wn_hblock_backward_data per block.  dr_upper nullable (the top block of a stack).
 * wn_hblock_backward_input: the input gradient of a block whose gate gradients exist already (the bottom of such a chain). */
int wn_hblock_backward_pair_is_fused(const wn_block_shape* upper, const wn_block_shape* lower, int precision);
int wn_hblock_backward_pair(const wn_block_shape* upper, const void* packed_upper, const wn_block_shape* lower, const void* packed_lower,
                            int precision, const void* dr_upper, const void* da_upper, const void* dg_upper, const void* dskip,
                            const void* z_lower, const void* sg_lower, void* dx_upper, void* da_lower, void* dg_lower,
                            unsigned* overflow_flag, wn_stream_t stream);
int wn_hblock_backward_input(const wn_block_shape* s, int precision, const void* packed, const void* dr, const void* da, const void* dg,
                             void* dx, float* dx_dense, const float* dyn_inv_scale, const void* x_act, float leaky_slope,
                             unsigned* overflow_flag, wn_stream_t stream);

/* The first block of a stack whose input x is the ACTIVATED output of a front-end conv kept in the series (x_act = leaky(.) as
 * stored): dx = (input gradient) * leaky'(x_act), written to the half series dx -- wn_hblock_backward_data plus the LeakyReLU
 * backward of the layer in front, in one epilogue. */
int wn_hblock_backward_data_masked(const wn_block_shape* s, int precision, const void* packed, const void* dr, const void* dskip,
                                   const void* z, const void* sg, void* da, void* dg, void* dx, const void* x_act, float leaky_slope,
                                   unsigned* overflow_flag, wn_stream_t stream);

/* Front-ends that are not GEMM-shaped, written straight into the stack's layouts (csrc/wn_front.hip):
 *   wn_hfeature_forward            RawCTCNet.feature_layer[0..1] (reference modules/raw_ctcnet.py:57-61,128): Conv1d(1 -> F, k,
 *                                  padding k - 1) + LeakyReLU of the raw signal x [B][length] -> half series of length length + k - 1,
 *                                  stored * out_scale (k multiply-adds per element: elementwise work, not a GEMM with 31/32 of K zero)
 *   wn_hfeature_backward_weights   dW [F][1][k], db [F] from the series gradient of that layer's output (* dyn_inv_scale / dy_scale);
 *                                  deterministic (per-slab partial sums reduced in slab order)
 *   wn_hseries_load_pooled /       WaveNetClassifier.mean_pool (reference modules/classifier.py:53,102): AvgPool1d(pool) fused into
 *   wn_series_load_pooled          the load of the stack's input (half series / fp32 padded series of length length / pool)
 *   wn_pool_backward               dx[b][c][t] = dpooled[b][c][t / pool] / pool (0 for a dropped tail), both dense fp32 */
int wn_hfeature_forward(int precision, const float* x, const float* weight, const float* bias, void* y_series, int batch, int length,
                        int features, int kernel_width, int ld, int halo, float out_scale, float leaky_slope, unsigned* overflow_flag,
                        wn_stream_t stream);
size_t wn_hfeature_wgrad_workspace_bytes(int batch, int length, int features, int kernel_width);
int wn_hfeature_backward_weights(int precision, const float* x, const void* dy_series, float dy_scale, float* dweight, float* dbias,
                                 int batch, int length, int features, int kernel_width, int ld, int halo, const float* dyn_inv_scale,
                                 void* workspace, size_t workspace_bytes, wn_stream_t stream);
int wn_hseries_load_pooled(int precision, const float* dense, void* series, int batch, int channels, int length, int pool, int ld, int halo,
                           float scale, const float* dyn_scale, unsigned* overflow_flag, wn_stream_t stream);
int wn_series_load_pooled(const float* dense, float* series, int batch, int channels, int length, int pool, int ld, int halo,
                          wn_stream_t stream);
int wn_pool_backward(const float* dpooled, float* dx, int batch, int channels, int length, int pool, wn_stream_t stream);
/* the dynamic gradient scale of a backward call in the fp16 modes: scale_and_inverse[0] = 2^floor(log2(target / max|x|)) (clamped to
 * 2^+-100), [1] = its reciprocal -- device floats, no host synchronisation.  `accumulator`: one DEVICE unsigned, zero before the
 * first call (the call leaves it zero again).  x 16-byte aligned. */
int wn_grad_scale(const float* x, long long count, float target, float* scale_and_inverse, unsigned* accumulator, wn_stream_t stream);

/* The weight gradients of SEVERAL blocks of one series geometry in one launch (+ one reduction): blocks of <= 128 channels are
 * two or three gradient tiles each, so per-block launches are short split-K jobs dominated by their partial slabs; keep the
 * operands of up to wn_hblocks_wgrad_group_max() blocks (after their wn_hblock_backward_data calls) and hand them over
 * together.  Arrays are indexed by block; dr[l] may be NULL (a last block).  Same results as per-block calls up to the
 * summation order over time splits (deterministic either way). */
int wn_hblocks_wgrad_group_max(const wn_block_shape* s, int precision);
size_t wn_hblocks_wgrad_workspace_bytes(const wn_block_shape* shapes, int nblocks, int precision);
int wn_hblocks_backward_weights(const wn_block_shape* shapes, int nblocks, int precision, const void* const* x, const void* const* z,
                                const void* const* da, const void* const* dg, const void* const* dr, const void* const* dskip,
                                const wn_block_params* grads, const float* dyn_inv_scale, void* workspace, size_t workspace_bytes,
                                wn_stream_t stream);

/* Every weight-pack job of a stack of blocks in ONE launch.  Training repacks all weights after each optimizer step (five
 * launches per block through wn_hblock_pack, one per group through wn_hskipsum_pack); the jobs' arguments depend only on
 * shapes, precision and pointers, so they are built ONCE into a table: wn_hstack_pack_table_build fills `table_host` (host
 * memory of wn_hstack_pack_table_bytes(nblocks) bytes), the caller copies it to the device and keeps it; each step
 * wn_hstack_pack_run(table_dev, ...) packs into `packed`, a device buffer of *packed_total bytes that may be a different
 * allocation every time.  Block l's packed weights (what wn_hblock_forward / backward_* take) then start at
 * packed + block_offsets[l]; with_skipsum != 0 also packs the long-K skips_sum weights of wn_hskipsum_forward from the
 * blocks' w_skip / b_skip, group g (WN_MAX_STACK_GROUP blocks each) at packed + skipsum_offsets[g] -- the b_skip vectors
 * must then be equally spaced in memory (WN_ERR_UNSUPPORTED otherwise: use the per-block entry points).
 * `dynamic` (<= 3 ranges): parameter tensors inside one of these address ranges are re-allocated between steps; the table
 * stores them as offsets and wn_hstack_pack_run receives the current bases, in the same order.  Rebuild the table when
 * any other pointer, a shape or the precision changes.  (No reference counterpart: the reference has no packed weights.) */
typedef struct wn_mem_range { const void* base; size_t bytes; } wn_mem_range;
size_t wn_hstack_pack_table_bytes(int nblocks);
int wn_hstack_pack_table_build(const wn_block_shape* shapes, const wn_block_params* params, int nblocks, int precision,
                               int with_skipsum, const wn_mem_range* dynamic, int ndynamic, void* table_host, size_t table_bytes,
                               size_t* block_offsets, size_t* skipsum_offsets, size_t* packed_total, int* njobs,
                               int* launch_blocks);
int wn_hstack_pack_run(const void* table_dev, int nblocks, int njobs, int launch_blocks, const void* const* dynamic_bases,
                       int ndynamic, void* packed, unsigned* overflow_flag /* as wn_hblock_pack_checked */, wn_stream_t stream);

/* ---- measurement hooks (bench.py): HIP-event timing of every kernel on its launch stream ----
 * Kernel classes: index into wn_prof_kernel_name().  wn_prof_collect() synchronises the recorded
 * events and adds them to the per-class totals; wn_prof_get() reads them. */
int wn_prof_enable(int on);
int wn_prof_reset(void);
int wn_prof_collect(void);
int wn_prof_num_kernels(void);
const char* wn_prof_kernel_name(int kernel_class);
int wn_prof_get(int kernel_class, double* total_ms, long long* launches, double* flops);

/* ---- stand-alone dilated conv in the half-precision modes: the half-series counterpart of wn_conv_* (CausalConv1d /
 * NonCausalConv1d of modules/conv_ops.py:8-79 and the 1x1 Conv1d members of the output stacks), so that a model switched to a
 * half mode runs ALL of its convolutions on the half kernels.  x and dy are half series (wn_hseries_load; x stored as
 * x * input_scale, dy as dy * the call's gradient scale); y, dx, dweight, dbias are dense fp32.
 *   forward          y[b][co][t]  = bias[co] + sum_j W[co][:][j] x[b][:][t + off_j]
 *   backward_data    dx[b][ci][t] = sum_j W[:][ci][j]^T dy[b][:][t - off_j]            (* *dyn_inv_scale when given)
 *   backward_weights dW[co][ci][j] = sum_{b,t} dy[b][co][t] x[b][ci][t + off_j] / input_scale;  db = row sums of dy   (same) */
size_t wn_hconv_packed_bytes(const wn_conv_shape* s, int precision);
int wn_hconv_pack(const wn_conv_shape* s, int precision, const float* weight /*[Co][Ci][k]*/, const float* bias /* may be NULL */,
                  float input_scale, void* packed, wn_stream_t stream);
int wn_hconv_forward(const wn_conv_shape* s, int precision, const void* packed, const void* x, float* y_dense, wn_stream_t stream);
int wn_hconv_backward_data(const wn_conv_shape* s, int precision, const void* packed, const void* dy, float* dx_dense,
                           const float* dyn_inv_scale /* DEVICE scalar, may be NULL */, wn_stream_t stream);
size_t wn_hconv_wgrad_workspace_bytes(const wn_conv_shape* s, int precision);
int wn_hconv_backward_weights(const wn_conv_shape* s, int precision, const void* x, const void* dy, float input_scale,
                              float* dweight, float* dbias /* may be NULL */, const float* dyn_inv_scale /* may be NULL */,
                              void* workspace, size_t workspace_bytes, wn_stream_t stream);

/* ---- the fp32 convolutions AROUND the block stack kept in the series layout (reference modules/wavenet.py:54,67-71,93,103:
 * entry_conv1d and output_stack): the entry conv writes the stack's input series, the output block reads the stack's result
 * as a series, and LeakyReLU rides in the epilogues -- no dense round trips and no stand-alone activation passes between them.
 *   wn_skipsum_forward_series     out = leaky_relu(sum_l W_skip_l z_l + bias_total) as a series (one group: nblocks <=
 *                                 WN_MAX_STACK_GROUP), the activated input of the output block's first conv
 *   wn_conv_forward_series        y = leaky_relu(conv(x) + b), series in, series out (wn_conv_forward is the form without activation)
 *   wn_conv_backward_data_series  dx = (W^T dy) * leaky_relu'(act); act = the conv's stored (activated) input, shaped like dx;
 *                                 NULL = no activation (wn_conv_backward_data)
 * The activation is torch's rule v > 0 ? v : v * slope, its derivative act > 0 ? 1 : slope (act == 0 takes the slope): for
 * slope >= 0 the stored leaky_relu(v) has the sign of v, so results are bitwise those of the separate torch passes. */
int wn_skipsum_forward_series(const wn_skipsum_shape* s, const void* packed, const float* const* z, float* out_series,
                              float leaky_slope, wn_stream_t stream);
int wn_conv_forward_series(const wn_conv_shape* s, const void* packed, const float* x, float* y, float leaky_slope,
                           wn_stream_t stream);
int wn_conv_backward_data_series(const wn_conv_shape* s, const void* packed, const float* dy, const float* act,
                                 float leaky_slope, float* dx, wn_stream_t stream);

/* ---- every fp32 weight-pack job of a stack in ONE launch: the fp32 counterpart of wn_hstack_pack_*.
 * The table covers each block's four arrangements (the image wn_block_pack writes), with_skipsum != 0 the long-K skips_sum
 * weights of each group of WN_MAX_STACK_GROUP blocks (the image wn_skipsum_pack writes from the blocks' w_skip;
 * skip_bias_total, [Ms] or NULL, is the bias of group 0) and `convs`, stand-alone convs around the stack (the image
 * wn_conv_pack writes).  Images are byte-identical to those of the per-object entry points and start at
 * packed + block_offsets[l] / skipsum_offsets[g] / conv_offsets[c] (multiples of 256).  wn_stack_pack_table_build is host-only:
 * it fills `table_host` (wn_stack_pack_table_bytes(nblocks, nconvs) bytes), which the caller copies to the device once and
 * keeps; each step wn_stack_pack_run(table_dev, ...) packs into `packed` (*packed_total bytes, may be another allocation every
 * time).  `dynamic` (<= 3 ranges): sources inside one of these address ranges are stored as offsets and each run supplies
 * the ranges' current bases, in the same order.  Rebuild the table when any other pointer or a shape changes. */
typedef struct wn_pack_conv { wn_conv_shape shape; const float* weight /*[Co][Ci][k]*/; const float* bias /*[Co] or NULL*/; } wn_pack_conv;
size_t wn_stack_pack_table_bytes(int nblocks, int nconvs);
int wn_stack_pack_table_build(const wn_block_shape* shapes, const wn_block_params* params, int nblocks, int with_skipsum,
                              const float* skip_bias_total, const wn_pack_conv* convs, int nconvs,
                              const wn_mem_range* dynamic, int ndynamic, void* table_host, size_t table_bytes,
                              size_t* block_offsets, size_t* skipsum_offsets, size_t* conv_offsets, size_t* packed_total,
                              int* njobs, int* launch_blocks);
int wn_stack_pack_run(const void* table_dev, int njobs, int launch_blocks, const void* const* dynamic_bases, int ndynamic,
                      void* packed, wn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* WAVENET_AMD_H */
