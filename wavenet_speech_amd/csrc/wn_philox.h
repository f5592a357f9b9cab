// Counter-based random numbers for the generators (wn_synth.hip, wn_reads.hip): Philox4x32-10, keyed by the caller's seed.
// A draw is a pure function of (seed, stream, index, sub): no state, any thread can produce any element, and a result does
// not depend on the launch shape.  The streams in use (the stream number sits in the counter's top word):
//   0  nucleotides            index = flat element (wn_synth) or (read << 32) | base (wn_reads)
//   1  Gaussian noise         index = flat sample (wn_synth) or (read << 32) | sample (wn_reads)
//   2  read lengths           index = read                                                    (wn_reads)
//   3  dwell times            index = (read << 32) | k-mer, sub = attempt of the rejection sampler (wn_reads)
#pragma once
#include <hip/hip_runtime.h>

namespace wn {

__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

__device__ __forceinline__ void draw_sub(unsigned long long seed, unsigned stream, unsigned long long index, unsigned sub,
                                         unsigned (&c)[4]) {
    c[0] = (unsigned)index; c[1] = (unsigned)(index >> 32); c[2] = sub; c[3] = stream;
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
}

__device__ __forceinline__ void draw(unsigned long long seed, unsigned stream, unsigned long long index, unsigned (&c)[4]) {
    draw_sub(seed, stream, index, 0u, c);
}

// N(0, 1) by Box-Muller from the four words of one draw: two 53-bit uniforms in (0, 1)
__device__ __forceinline__ double philox_normal(const unsigned (&c)[4]) {
    const double u1 = ((double)(((unsigned long long)(c[0] >> 5) << 26) | (c[1] >> 6)) + 0.5) * (1.0 / 9007199254740992.0);
    const double u2 = ((double)(((unsigned long long)(c[2] >> 5) << 26) | (c[3] >> 6)) + 0.5) * (1.0 / 9007199254740992.0);
    return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}

}  // namespace wn
