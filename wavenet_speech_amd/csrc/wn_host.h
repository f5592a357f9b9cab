// Host-side facilities shared by the translation units of libwavenet_amd.so: the kernel-class table of the profiler, error
// reporting, the timing scope, and the geometry / shape checks of the C ABI.  Internal to the library (the C ABI itself is
// include/wavenet_amd.h); nothing here is device code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdlib>

#include "../../include/wavenet_amd.h"

namespace wn {

// ---- kernel classes: what wn_prof_* books a launch under -------------------------------------------------------------------
// ONE list: the enumerators and the names wn_prof_kernel_name() returns come from it, in this order.  The names are read by the
// tests and the benchmark (which kernel form ran; rocprof symbols), so a new class goes at the end.
#define WN_KERNEL_CLASSES(X)                                   \
    X(KC_PACK, "pack_kernel")                                  \
    X(KC_GATE_GEMM, "series_gemm_kernel<gate>")                \
    X(KC_OUT_GEMM, "series_gemm_kernel<res>")                  \
    X(KC_DZ_GEMM, "series_gemm_kernel<dz,dgate>")              \
    X(KC_DX_GEMM, "series_gemm_kernel<dx>")                    \
    X(KC_WGRAD, "wgrad_kernel")                                \
    X(KC_WGRAD_REDUCE, "wgrad_reduce_kernel")                  \
    X(KC_CONV_FWD, "series_gemm_kernel<conv_fwd>")             \
    X(KC_CONV_BWD_DATA, "series_gemm_kernel<conv_bwd_data>")   \
    X(KC_SKIP_GEMM, "series_gemm_kernel<skips_sum>")           \
    X(KC_HLOAD, "hload_kernel")                                \
    X(KC_HGATE, "hgemm_kernel<gate>")                          \
    X(KC_HRES, "hgemm_kernel<res>")                            \
    X(KC_HDZ, "hgemm_kernel<dz,dgate>")                        \
    X(KC_HDX, "hgemm_kernel<dx>")                              \
    X(KC_HSKIP, "hgemm_kernel<skips_sum>")                     \
    X(KC_HWGRAD, "hwgrad_kernel")                              \
    X(KC_EMBED, "embed_kernel")                                \
    X(KC_SYNTH, "synth_kernel")                                \
    X(KC_CTC, "ctc_kernel")                                    \
    X(KC_HFUSED, "hfused_fwd_kernel")                          \
    X(KC_HCONV_FWD, "hgemm_kernel<conv_fwd>")                  \
    X(KC_HCONV_BWD_DATA, "hgemm_kernel<conv_bwd_data>")        \
    X(KC_HCOL_DZ, "hcol_kernel<dz,dgate>")                     \
    X(KC_HCOL_DX, "hcol_kernel<dx>")                           \
    X(KC_HCOL_DXDZ, "hcol2_kernel<dx+dz>")                     \
    X(KC_HCOL_SKIP, "hcol_kernel<skips_sum>")

enum KernelClass {
#define WN_KC_ENUM(id, name) id,
    WN_KERNEL_CLASSES(WN_KC_ENUM)
#undef WN_KC_ENUM
    KC_COUNT
};
inline constexpr const char* kKernelNames[KC_COUNT] = {
#define WN_KC_NAME(id, name) name,
    WN_KERNEL_CLASSES(WN_KC_NAME)
#undef WN_KC_NAME
};
constexpr KernelClass KC_FRONT = KC_HLOAD;   // the front-end kernels (wn_front.hip) are timed with the layout loads

// ---- error reporting ---------------------------------------------------------------------------------------------------------
// records "what: <HIP error string>" for wn_last_hip_error() and returns WN_ERR_HIP (wn_api.hip)
int hip_fail(hipError_t e, const char* what);
#define WN_HIP(call, what)                                        \
    do {                                                          \
        hipError_t e__ = (call);                                  \
        if (e__ != hipSuccess) return ::wn::hip_fail(e__, what);  \
    } while (0)

// ---- timing scope: HIP events around a launch on its stream while profiling is on (wn_api.hip) ------------------------------
struct ProfRec { int kc; hipEvent_t e0, e1; double flops; };
struct ProfScope {
    ProfScope(int kc, double flops, hipStream_t st);
    ~ProfScope();
    ProfScope(const ProfScope&) = delete;
    ProfScope& operator=(const ProfScope&) = delete;

private:
    bool active = false;
    ProfRec rec{};
    hipStream_t st;
};

// ---- geometry ----------------------------------------------------------------------------------------------------------------
inline int rup(int x, int m) { return (x + m - 1) / m * m; }
inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline int cp8(int c) { return rup(c, 8); }      // channel rows of an fp32 series
inline int cp32(int c) { return rup(c, 32); }    // channels of a half series
inline size_t align256(size_t b) { return (b + 255) / 256 * 256; }
inline bool half_prec(int p) { return p == WN_F16X3 || p == WN_F16 || p == WN_BF16; }
// states of the blank-extended labelling of the CTC loss and the forced alignment, 2 L + 1, in whole waves
inline int ctc_states_padded(int max_label_len) { return (2 * max_label_len + 1 + 63) / 64 * 64; }

// column offsets of the k taps of a dilated conv: tap j reads x[t + off[j]]
inline void tap_offsets(int k, int d, int causal, int* off) {
    const int p = causal ? (k - 1) * d : wn_autopad(k, d);
    for (int j = 0; j < k; ++j) off[j] = j * d - p;
}

// What a residual block's shape and a stand-alone conv's share (a conv passes skip_rows = 1): positive dimensions, the
// WN_MAX_* limits, then the tap offsets and the largest |offset|, which the caller's layout check holds against the halo.
inline int check_taps(int in_channels, int out_channels, int skip_rows, int kernel_width, int dilation, int causal, int* off,
                      int* max_abs_off) {
    if (in_channels <= 0 || out_channels <= 0 || skip_rows <= 0 || dilation <= 0 || kernel_width < 1) return WN_ERR_BAD_SHAPE;
    if (kernel_width > WN_MAX_TAPS) return WN_ERR_UNSUPPORTED;
    if (in_channels > WN_MAX_CHANNELS || out_channels > WN_MAX_CHANNELS || skip_rows > WN_MAX_CHANNELS) return WN_ERR_UNSUPPORTED;
    tap_offsets(kernel_width, dilation, causal, off);
    int mx = 0;
    for (int j = 0; j < kernel_width; ++j) mx = mx > std::abs(off[j]) ? mx : std::abs(off[j]);
    *max_abs_off = mx;
    return WN_OK;
}

// wn_pair_align's limits, which the tools that walk its op strings (quality profile, pileup, evidence, left-alignment) share, and
// the limits of the tables over a reference (pileup, consensus and genotype calls)
constexpr int kPaMaxQuery = 8192, kPaMaxRef = 65535, kPaMaxOps = kPaMaxRef + kPaMaxQuery;
constexpr int kMaxReference = 1 << 26, kMaxIns = 8;

// The reads of a batch as wn_pileup and wn_pileup_evidence take them: PileupArgs and EvidenceArgs begin with one.
struct ReadBatch {
    const unsigned char* ops;           // row b at ops + b * ops_stride
    const int *ops_len, *lo, *ref_len, *strand, *query, *query_len;
    const unsigned char *qual, *keep;   // each or nullptr
    long long ops_stride, query_stride, qual_stride;
    int B, M, max_ops, R, min_qual;
};
// from the arguments of the two entry points, in their order
inline ReadBatch read_batch(const unsigned char* ops, long long ops_stride, const int* ops_len, const int* lo, const int* ref_lengths,
                            const int* strand, const int* query, long long query_stride, const int* query_lengths,
                            const unsigned char* qual, long long qual_stride, const unsigned char* keep, int batch, int max_query_len,
                            int max_ops, int reference_len, int min_qual) {
    return {ops, ops_len, lo, ref_lengths, strand, query, query_lengths, qual, keep, ops_stride, query_stride, qual_stride,
            batch, max_query_len, max_ops, reference_len, min_qual};
}

// What the entry points over op rows and their queries check (wn_gap_left_align; through check_read_batch wn_pileup and
// wn_pileup_evidence), one status class after the other; the caller hands in its own verdict for each class.
inline int check_op_rows(int batch, int max_query_len, int max_ops, long long ops_stride, long long query_stride, bool own_shape_ok,
                         bool own_supported, bool pointers_ok) {
    if (batch < 1 || max_query_len < 1 || max_ops < 1 || ops_stride < 0 || query_stride < 0 || !own_shape_ok) return WN_ERR_BAD_SHAPE;
    if (batch > 65535 || max_query_len > kPaMaxQuery || max_ops > kPaMaxOps || !own_supported) return WN_ERR_UNSUPPORTED;
    return pointers_ok ? WN_OK : WN_ERR_NULL;
}
// the same for a filled-in ReadBatch, with the reference's length, the qual rows and the sign of min_qual (its ceiling, the
// qual rows of the device tables, is the caller's)
inline int check_read_batch(const ReadBatch& r, bool own_shape_ok, bool own_supported, bool own_pointers_ok) {
    return check_op_rows(r.B, r.M, r.max_ops, r.ops_stride, r.query_stride,
                         r.R >= 1 && r.qual_stride >= 0 && r.min_qual >= 0 && own_shape_ok, r.R <= kMaxReference && own_supported,
                         r.ops && r.ops_len && r.lo && r.ref_len && r.strand && r.query && r.query_len && own_pointers_ok);
}
// the affine costs of wn_pair_align and wn_demux_scores: 0 <= gap_extend <= gap_open <= 1024, |match|, |mismatch| <= 1024
inline int check_affine_costs(int match, int mismatch, int gap_open, int gap_extend) {
    const auto in = [](int v) { return v >= -1024 && v <= 1024; };       // no abs: INT_MIN is a possible argument
    return 0 <= gap_extend && gap_extend <= gap_open && gap_open <= 1024 && in(match) && in(mismatch) ? WN_OK : WN_ERR_UNSUPPORTED;
}

}  // namespace wn
