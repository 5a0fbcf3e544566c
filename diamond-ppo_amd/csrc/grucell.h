// What the RecurrentPPO GRU kernels share (gru.hip, gruact.hip, grugrad.hip, gruseq.hip): the
// network family's constants, the supported hidden widths and their dispatch, and -- for the two
// kernels that run whole sequences, grugrad.hip (phases B and D) and gruseq.hip (the scans) -- the
// staging of Whh and the one forward and one backward recurrence.
//
// The recurrences are written for "lane j of an env, all T steps": G lanes per env, lane j =
// hidden unit j, an env inside one wave (G <= 64).  The per-step exchange of the hidden state
// (forward) and of the 3G gate deltas (backward) goes through the env's LDS buffer with no
// workgroup barrier in the time loop: a wave issues its LDS writes and reads in program order.
// Whh sits in LDS with a row stride of G + 1 (stage_whh): lane j's k-th read of its rows
// ((gG + j)(G + 1) + k, forward) and its column reads (g (G + 1) + j, backward) both fall on
// distinct consecutive banks.  Where a kernel keeps its operands is its operand policy's business
// (below); every floating-point expression is here, once, so the kernels agree bit for bit.  Every
// sum runs over k in a fixed order inside one lane: no atomics, the same bits on every call.
// gruact.hip's single step sums in another order (dot4 pairs, weights from global memory) and
// takes only the constants and the dispatch.
#pragma once

#include <type_traits>

#include "common.h"

namespace dppo {

constexpr int kH = 64;     // MLP hidden
constexpr int kAPad = 16;  // action dims padded

// The supported gru_hidden widths, once: f(std::integral_constant<int, G>{}) for G = 16, 32 or
// 64; false (f not called) for any other width.
template <class F>
bool dispatch_gru_width(int G, F&& f) {
  switch (G) {
    case 16: f(std::integral_constant<int, 16>{}); return true;
    case 32: f(std::integral_constant<int, 32>{}); return true;
    case 64: f(std::integral_constant<int, 64>{}); return true;
    default: return false;
  }
}
inline bool gru_width_ok(int G) {
  return dispatch_gru_width(G, [](auto) {});
}

// Whh [3G][G] (16-byte aligned) into LDS with a row stride of G + 1, by kThreads threads
template <int G, int kThreads>
__device__ __forceinline__ void stage_whh(float* dst, const float* __restrict__ src, int tid) {
  static_assert(G % 4 == 0, "a 16-byte load stays inside a row");
  for (int k4 = tid; k4 < 3 * G * G / 4; k4 += kThreads) {
    const f32x4 v = ((const f32x4*)src)[k4];
    const int k = 4 * k4;
    float* d = dst + (k / G) * (G + 1) + (k % G);
    d[0] = v[0];
    d[1] = v[1];
    d[2] = v[2];
    d[3] = v[3];
  }
}

// One step's operands that do not depend on the carried state; the recurrences load them a step
// ahead.
struct GruFwdIn {
  float gir, giz, gin;  // lane j's gate inputs gi = Wih x + b_ih, rows j, G + j, 2G + j
  bool done;            // the hidden state is zeroed before the step
};
struct GruBwdIn {
  float dout;  // dL/dh' of the step from outside the recurrence
  float r, z, n, ghn;
  float hin;   // the hidden state the step started from, after the reset
  bool done;
};

// Forward over t = 0 .. T - 1 from h.  W: Whh in LDS (stage_whh), bhh: b_hh [3G], hb: the env's
// G floats of LDS.  Ops: in(t) -> GruFwdIn; store(t, h_in, r, z, n, gh_n, h_out).
template <int G, class Idx, class Ops>
__device__ __forceinline__ void gru_seq_fwd(const float* W, const float* bhh, float* hb, int j,
                                            float h, Idx T, const Ops& op) {
  constexpr int kWs = G + 1;
  const float* wr = W + j * kWs;
  const float* wz = W + (G + j) * kWs;
  const float* wn = W + (2 * G + j) * kWs;
  const float br = bhh[j], bz = bhh[G + j], bn = bhh[2 * G + j];
  GruFwdIn nx = op.in(Idx(0));
  for (Idx t = 0; t < T; ++t) {
    const GruFwdIn cur = nx;
    nx = op.in(t + 1 < T ? t + 1 : T - 1);
    if (cur.done) h = 0.0f;  // hx[:, dones[t]] = 0 (recurrent_ppo.py:84)
    hb[j] = h;
    float ghr = br, ghz = bz, ghn = bn;
#pragma unroll
    for (int q = 0; q < G / 4; ++q) {
      const f32x4 x = *(const f32x4*)(hb + 4 * q);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        ghr += wr[4 * q + u] * x[u];
        ghz += wz[4 * q + u] * x[u];
        ghn += wn[4 * q + u] * x[u];
      }
    }
    const float r = sigm(cur.gir + ghr), z = sigm(cur.giz + ghz);
    const float nn = tanh_acc(cur.gin + r * ghn);
    const float hn = (1.0f - z) * nn + z * h;
    op.store(t, h, r, z, nn, ghn, hn);
    h = hn;
  }
}

// BPTT over t = T - 1 .. 0 from the carry dL/dh_T; returns dL/dh_0 (before step 0's reset is
// undone: zero where the env starts on a reset).  W as above, gb: the env's 3G floats of LDS.
// Ops: in(t) -> GruBwdIn; dgi(t), dgh(t) -> the step's [3G] output rows.
template <int G, class Idx, class Ops>
__device__ __forceinline__ float gru_seq_bwd(const float* W, float* gb, int j, float carry, Idx T,
                                             const Ops& op) {
  constexpr int G3 = 3 * G, kWs = G + 1;
  const float* wc = W + j;  // column j
  GruBwdIn nx = op.in(T - 1);
  for (Idx t = T - 1; t >= 0; --t) {
    const GruBwdIn cur = nx;
    nx = op.in(t > 0 ? t - 1 : 0);
    const float dh = cur.dout + carry;
    const float r = cur.r, z = cur.z, nn = cur.n;
    const float dn = dh * (1.0f - z);
    const float dz = dh * (cur.hin - nn);
    const float dan = dn * (1.0f - nn * nn);
    const float dghn = dan * r;
    const float dar = dan * cur.ghn * r * (1.0f - r);
    const float daz = dz * z * (1.0f - z);
    float* dgi = op.dgi(t);
    float* dgh = op.dgh(t);
    dgi[j] = dar;
    dgi[G + j] = daz;
    dgi[2 * G + j] = dan;
    dgh[j] = dar;
    dgh[G + j] = daz;
    dgh[2 * G + j] = dghn;
    gb[j] = dar;
    gb[G + j] = daz;
    gb[2 * G + j] = dghn;
    float dhin = dh * z;
#pragma unroll
    for (int q = 0; q < G3 / 4; ++q) {
      const f32x4 x = *(const f32x4*)(gb + 4 * q);
      dhin += wc[(4 * q) * kWs] * x[0] + wc[(4 * q + 1) * kWs] * x[1] +
              wc[(4 * q + 2) * kWs] * x[2] + wc[(4 * q + 3) * kWs] * x[3];
    }
    // h_in = h_prev * keep  =>  dh_prev = dh_in * keep
    carry = cur.done ? 0.0f : dhin;
  }
  return carry;
}

}  // namespace dppo
