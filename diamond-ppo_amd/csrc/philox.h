// Philox4x32-10 and the u32 -> (0, 1) map of the rollout samplers (mlp.hip act_kernel,
// gruact.hip gru_act_kernel<G> at every GRU width): one definition, so every sampler draws the documented stream
// (tests restate it in NumPy).
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace dppo {

__device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) {
  return (uint32_t)(((uint64_t)a * b) >> 32);
}

__device__ __forceinline__ void philox4x32(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = mulhi32(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = mulhi32(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// u32 -> uniform in (0, 1): 24 random bits, centred in their interval (never 0 or 1)
__device__ __forceinline__ float u01(uint32_t x) {
  return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f);
}

}  // namespace dppo
