// Philox-4x32-10 (Salmon et al. 2011): the counter-based generator of the device-side candidate generation (acq.hip) and of
// the SGHMC chains' draws (bnn.hip).
#pragma once
#include "common.h"

namespace robo {

__device__ __forceinline__ void philox_round(unsigned (&c)[4], unsigned k0, unsigned k1) {
    const unsigned long long p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

// the ten rounds on counter c under the 64-bit key `seed` -> two uniforms in [0, 1) of 53 bits each: (c0, c1) and (c2, c3)
__device__ __forceinline__ void philox_uniform2(unsigned (&c)[4], unsigned long long seed, double& ua, double& ub) {
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c, k0, k1);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    const unsigned long long a = ((unsigned long long)c[0] << 32 | c[1]) >> 11;
    const unsigned long long b = ((unsigned long long)c[2] << 32 | c[3]) >> 11;
    ua = (double)a * (1.0 / 9007199254740992.0);
    ub = (double)b * (1.0 / 9007199254740992.0);
}

}  // namespace robo
