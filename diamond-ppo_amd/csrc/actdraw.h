// The rollout samplers' draw from a sample's actor heads: one definition for the tuned act kernel
// (mlp.hip act_kernel) and the wide one (mbwide.hip wide_act_kernel), so both draw the stream
// dppo_act_f32 documents (tests restate it in NumPy).  Philox4x32-10 keyed by the seed, counter =
// (sample index lo, sample index hi, call counter lo, call counter hi).  Run by the one lane that
// stores the sample; out[] holds the logits / Gaussian means, AMAX >= A its compile-time bound.
#pragma once

#include "philox.h"

namespace dppo {

// What the draw reads from the kernel's argument struct (ARGS): the Philox key and call counter
// {seed_lo, seed_hi, ctr_lo, ctr_hi}, A, and for the Gaussian {env_act, squash, sq_lo[], sq_half[],
// sq_hi[]}.

// Categorical(logits).sample() by inverse CDF on one uniform
template <int AMAX, class ARGS>
__device__ __forceinline__ int draw_categorical(const ARGS& a, const float (&out)[AMAX],
                                                int64_t i) {
  const int A = a.A;
  uint32_t c[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), a.ctr_lo, a.ctr_hi};
  philox4x32(c, a.seed_lo, a.seed_hi);
  float mx = out[0];
#pragma unroll
  for (int k = 1; k < AMAX; ++k)
    if (k < A) mx = fmaxf(mx, out[k]);
  float e[AMAX], se = 0.0f;
#pragma unroll
  for (int k = 0; k < AMAX; ++k) {
    e[k] = k < A ? __expf(out[k] - mx) : 0.0f;
    se += e[k];
  }
  // the first k whose cumulative mass exceeds u * sum (the last action takes the remainder)
  const float target = u01(c[0]) * se;
  int pick = A - 1;
  float cum = 0.0f;
#pragma unroll
  for (int k = 0; k < AMAX; ++k) {
    if (k < A - 1) {
      cum += e[k];
      if (pick == A - 1 && target < cum) pick = k;
    }
  }
  return pick;
}

// Normal(mean, exp(log_std)).sample(): Box-Muller pairs from Philox (4 uniforms per call), the
// block of four action dims k0 xor-ed into the counter's high sample word.  act: this sample's A
// draws u.  a.env_act (or null): the [n][A] environment actions, tanh(u) (squash 1) or
// sq_lo + (tanh(u) + 1) * sq_half (squash 2) -- the squashed env action (SURVEY 8 f2 extension;
// the reference samples the raw Gaussian, continuous_ppo.py:83-93): accurate tanhf, not the MLP's
// fast form.  Capped at sq_hi: where tanhf returns 1, low + 2 * ((high - low) / 2) can round one
// ulp above high, outside the action space.
template <int AMAX, class ARGS>
__device__ __forceinline__ void draw_gaussian(const ARGS& a, const float (&out)[AMAX],
                                              const float* ls, int64_t i, float* act) {
  const int A = a.A;
#pragma unroll
  for (int k0 = 0; k0 < AMAX; k0 += 4) {
    if (k0 < A) {
      uint32_t c[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32) ^ (uint32_t)(k0 << 24),
                       a.ctr_lo, a.ctr_hi};
      philox4x32(c, a.seed_lo, a.seed_hi);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const float r = sqrtf(-2.0f * __logf(u01(c[2 * p])));
        float sn, cs;
        __sincosf(6.28318530717958647692f * u01(c[2 * p + 1]), &sn, &cs);
        const int k = k0 + 2 * p;
        const float u0 = k < AMAX ? out[k] + __expf(ls[k]) * (r * cs) : 0.f;
        const float u1 = k + 1 < AMAX ? out[k + 1] + __expf(ls[k + 1]) * (r * sn) : 0.f;
        if (k < A) act[k] = u0;
        if (k + 1 < A) act[k + 1] = u1;
        if (a.env_act) {
          float* env = a.env_act + i * A;
          if (k < A) {
            const float t0 = tanhf(u0);
            const float e0 = fminf(a.sq_lo[k] + (t0 + 1.0f) * a.sq_half[k], a.sq_hi[k]);
            env[k] = a.squash == 2 ? e0 : t0;
          }
          if (k + 1 < A) {
            const float t1 = tanhf(u1);
            const float e1 = fminf(a.sq_lo[k + 1] + (t1 + 1.0f) * a.sq_half[k + 1], a.sq_hi[k + 1]);
            env[k + 1] = a.squash == 2 ? e1 : t1;
          }
        }
      }
    }
  }
}

}  // namespace dppo
