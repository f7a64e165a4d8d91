// philox.hpp — Philox4x32-10 (Salmon et al., SC'11), the one counter-based generator of the device noise sources: 64-bit counter
// in the low two words, 64-bit key, ten rounds, four 32-bit words out.  What each sampler makes of the words (RBPF's normal_pair,
// MPPI's wide and narrow device_noise) stays with the sampler; tests/noise_restatement.py is the restatement all are held to.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace tbnav {

__device__ __forceinline__ void philox4x32_10(uint64_t ctr, uint64_t key, uint32_t (&out)[4]) {
  uint32_t c0 = (uint32_t)ctr, c1 = (uint32_t)(ctr >> 32), c2 = 0u, c3 = 0u;
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

}  // namespace tbnav
