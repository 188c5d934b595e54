// Philox4x32-10 (Salmon et al., Random123) and the Box-Muller value the noise planes are made of: one copy for
// gs_img_stack (imgstack.hip) and the intensity chain of the 3-D patch kernels (intensity.hpp).
#pragma once
#include "common.hpp"

constexpr unsigned PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

// first two output words of Philox4x32-10 for the counter (c0, c1, c2, c3) and the key (k0, k1)
__device__ __forceinline__ void philox_r01(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1,
                                           unsigned& r0, unsigned& r1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const unsigned hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  r0 = c0;
  r1 = c1;
}

__device__ __forceinline__ float normal_from(unsigned r0, unsigned r1) {
  const float u1 = ((float)(r0 >> 9) + 0.5f) * 1.1920928955078125e-07f;     // 2^-23: in (0, 1), exact
  const float u2 = (float)(r1 >> 8) * 5.9604644775390625e-08f;              // 2^-24: in [0, 1), exact
  return sqrtf(-2.f * logf(u1)) * cosf(6.283185307179586f * u2);
}
