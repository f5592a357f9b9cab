// Host program of tests/test_band_cursor.py: the incremental band cursor of csrc/wn_band_dev.h against its closed form.
// For W in {64, 128}, n in 1..200 and every N in 1..3 (n - 1) + 1, at every step i: advance() returns band_lo(i) - band_lo(i - 1),
// lo is band_lo(i) and lo_slot is lo mod W.  Prints the steps and the largest delta it saw; exits 1 at the first mismatch.
#include <cstdio>

#include "../wavenet_speech_amd/csrc/wn_band_dev.h"

int main() {
    long long steps = 0;
    int seen = 0;                                                    // bit d: a step with delta d
    for (int W = 64; W <= 128; W += 64)
        for (int n = 1; n <= 200; ++n)
            for (int N = 1; N <= 3 * (n - 1) + 1; ++N) {
                wn::BandCursor cur(N, n, W);
                if (cur.lo != wn::band_lo(0, N, n, W) || cur.lo_slot != 0) {
                    std::printf("W %d n %d N %d: step 0 starts at lo %d slot %d\n", W, n, N, cur.lo, cur.lo_slot);
                    return 1;
                }
                for (int i = 1; i < n; ++i, ++steps) {
                    const int want = wn::band_lo(i, N, n, W), before = wn::band_lo(i - 1, N, n, W);
                    const int delta = cur.advance();
                    if (delta != want - before || cur.lo != want || cur.lo_slot != want % W || delta < 0 || delta > 3) {
                        std::printf("W %d n %d N %d step %d: delta %d lo %d slot %d, closed form %d after %d\n", W, n, N, i, delta, cur.lo,
                                    cur.lo_slot, want, before);
                        return 1;
                    }
                    seen |= 1 << delta;
                }
            }
    std::printf("steps %lld deltas 0x%x\n", steps, seen);
    return seen == 0xf ? 0 : 1;
}
