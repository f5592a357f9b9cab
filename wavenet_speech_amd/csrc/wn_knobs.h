// Everything libwavenet_amd.so reads from the environment, and the only getenv of csrc/.  Host code only.
//
// PRODUCT SWITCHES choose between two complete forms of a step; both forms are shipped and the parity tests hold one to the other
// (INTEGRATION.md section 5 lists them with the Python ones).  MEASUREMENT KNOBS are aids of A/B runs: several make results wrong
// on purpose or change the packed-weight layout, so the product library does not read them at all.  They exist only in a build
// with -DWN_MEASURE (`make measure`: ../libwavenet_amd_measure.so, the same kernels by the same per-file flags), which the tools
// that set one load (tools/run_bench_with_lib.py, tools/fused_bench.py).
// A new measurement aid goes through measure_knob(); a new form switch needs a test that compares both forms.
#pragma once
#include <cstdlib>

namespace wn {

// ONE list each: the enumerators (the variable's own name) and the names getenv is asked for come from it.
#define WN_PRODUCT_SWITCHES(X) \
    X(WN_FUSED_FWD)            \
    X(WN_COL_BWD)              \
    X(WN_COL_PAIR)             \
    X(WN_HWGRAD_COMPOSITE)     \
    X(WN_HGEMM16)

#define WN_MEASURE_KNOBS(X) \
    X(WN_FUSED_DBG)         \
    X(WN_COL_DBG)           \
    X(WN_HGEMM_DBG)         \
    X(WN_HGEMM_DBG_EPI)     \
    X(WN_HWGRAD_DBG)        \
    X(WN_FUSED_STAMPS)      \
    X(WN_MT2_MASK)          \
    X(WN_DZ_MT)             \
    X(WN_GEMM_VARIANT)      \
    X(WN_HGEMM16_COLS)      \
    X(WN_HGEMM_OCCUPANCY)

#define WN_KNOB_ENUM(name) name,
#define WN_KNOB_NAME(name) #name,
enum class Switch { WN_PRODUCT_SWITCHES(WN_KNOB_ENUM) };
enum class Knob { WN_MEASURE_KNOBS(WN_KNOB_ENUM) kCount };
inline constexpr const char* kSwitchNames[] = {WN_PRODUCT_SWITCHES(WN_KNOB_NAME)};

// A product switch, read per call (the parity tests compare both forms in one process): on unless the variable reads as 0.
inline bool switch_on(Switch s) {
    const char* e = getenv(kSwitchNames[(int)s]);
    return !(e && atoi(e) == 0);
}
// WN_HGEMM16 alone is an integer and read once per process (HPlan::init): 0 never hgemm8_kernel, 1 where it wins, 2 wherever
// the shape allows (tests, in a child process).
inline int hgemm16_form() {
    static const int v = [] { const char* e = getenv(kSwitchNames[(int)Switch::WN_HGEMM16]); return e ? atoi(e) : 1; }();
    return v;
}

#ifdef WN_MEASURE
inline constexpr bool kMeasureBuild = true;
// the variable's integer value, or dflt where it is not set (a knob that only switches something on is set to 1); the
// environment is read once per process, at the first call
inline int measure_knob(Knob k, int dflt) {
    static const struct Values {
        const char* v[(int)Knob::kCount];
        Values() {
            static constexpr const char* names[] = {WN_MEASURE_KNOBS(WN_KNOB_NAME)};
            for (int i = 0; i < (int)Knob::kCount; ++i) v[i] = getenv(names[i]);
        }
    } values;
    return values.v[(int)k] ? atoi(values.v[(int)k]) : dflt;
}
#else
inline constexpr bool kMeasureBuild = false;
// the product build: the default, at compile time.  No name of a knob reaches the object file.
constexpr int measure_knob(Knob, int dflt) { return dflt; }
#endif
#undef WN_KNOB_ENUM
#undef WN_KNOB_NAME

}  // namespace wn
