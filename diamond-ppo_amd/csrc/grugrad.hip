// RecurrentPPO minibatch gradient, fused: the full [T x N] GRU sequence recomputed from the stored
// initial hidden state (intended semantics of reference diamond/recurrent_ppo.py:301-367: every
// minibatch re-runs the sequence, :337, and slices its samples, :340-341), the PPO loss on the
// minibatch's samples, and the analytic backward through heads, GRU (BPTT with the per-step hidden
// resets, :82-87) and base layer -- one launch per minibatch instead of torch's hundreds.  The
// reference itself cannot run (GRUCore.forward evaluates `hx or ...` on a tensor, :78), so the
// yardstick is torch's own nn.GRU cell on the same semantics (tests/test_gpu_gru.py).
//
// Network (recurrent_ppo.py:94-149 as restated in diamond/recurrent_ppo.py): x1 = tanh(Wb obs + bb)
// [64]; torch GRU cell, hidden G: r = s(Wir x1 + bir + Whr h + bhr), z = s(Wiz x1 + biz + Whz h +
// bhz), n = tanh(Win x1 + bin + r (Whn h + bhn)), h' = (1 - z) n + z h, with h zeroed where the
// step's prev_done is set; actor Linear(G, 64) tanh Linear(64, A); critic Linear(G, 64) tanh
// Linear(64, 1).
//
// gru_grad_kernel<G> is the one kernel source for G = 16, 32 and 64.  One workgroup = 256 / G envs
// over all T steps (256 threads): 16 envs at G = 16, 8 at 32, 4 at 64, one gradient slab each.
// Phases, separated by workgroup barriers, exchanging per-sample vectors through a global scratch
// (SoA, one row per sample, rows sized by G):
//  A  per sample (thread per sample): x1, then gi = Wih x1 + bih in blocks of 48 gate rows
//     (G = 16: the one block beside x1);
//  B  per env, serial in t: G lanes per env (lane j = hidden unit j, all in one wave), the
//     recurrent half gh = Whh h + bhh and the cell; Whh read from LDS, h exchanged through LDS;
//  C  per minibatch sample: heads, loss (ppo.py:264-280 terms), head backward -> dL/dh' (h and
//     dh' as G registers);
//  D  per env, serial in reverse: BPTT through the cell, column j of Whh read from LDS;
//  E  per sample: dx1 = (Wih^T dgi)(1 - x1^2), 64 accumulators, dgi streamed 4 rows at a time;
//  F  weight gradients = sums over the workgroup's samples of outer products, on
//     v_mfma_f32_16x16x4_f32 (k = sample) in a fixed order, bias sums on VALU, one slab per
//     workgroup (optim.hip's slab reduction sums them in a fixed order: bit-reproducible).
// No per-thread array is ever indexed by a run-time value (that would put it in scratch memory).
// gru_grad_kernel<G, true> is the form for observations of 33 to 128 floats: phase A's base layer
// walks the observation row in blocks of 32 columns (base8_wide); everything else is the same
// code, already written in D and D16.
// gru_grad_kernel<G, WIDE_OBS, true> is the Gaussian head (RecurrentContinuousPPO; the loss of
// continuous_ppo.py:276-292 on the GRU features): phase C's loss and its derivative, and one more
// bias column in phase F (the state-independent log_std), differ; A, B, D and E are the same code.
//
// LDS holds the biases for the whole launch and, in one region restaged between the phases' own
// barriers, only the weights the current phase reads: A Wb + Wih | B, D Whh | C Wa1 Wc1 Wa2 |
// E Wih.  The recurrences of B and D, and Whh's LDS image with its row stride of G + 1 floats, are
// grucell.h's, shared with the scan kernels of gruseq.hip.
#include "grucell.h"

namespace dppo {
namespace {

constexpr int kThr = 256;
constexpr int kGiBlk = 48; // gate rows per register block of phase A

// LDS (floats): the phase's weights at W, then the biases, then the exchange buffers
struct GruLds {
  int W, bb, bih, bhh, ba1, ba2, bc1, Wc2, bc2, hbuf, gbuf, red, total;
};
__host__ __device__ constexpr int imax(int a, int b) { return a > b ? a : b; }
__host__ __device__ constexpr GruLds gru_lds(int D, int G) {
  GruLds L{};
  int o = 0;
  L.W = o;
  o += imax(imax(kH * D + 3 * G * kH, 3 * G * (G + 1)), 2 * kH * G + kAPad * kH);
  o = (o + 3) & ~3;
  L.bb = o; o += kH;
  L.bih = o; o += 3 * G;
  L.bhh = o; o += 3 * G;
  L.ba1 = o; o += kH;
  L.ba2 = o; o += kAPad;
  L.bc1 = o; o += kH;
  L.Wc2 = o; o += kH;
  L.bc2 = o; o += 4;
  L.hbuf = o; o += kThr;      // envs x G
  L.gbuf = o; o += 3 * kThr;  // envs x 3 G
  L.red = o; o += 3 * kThr;
  L.total = o;
  return L;
}

// n floats (a multiple of 4; both pointers 16-byte aligned) from global memory into LDS
__device__ __forceinline__ void stage4(float* dst, const float* __restrict__ src, int n, int tid) {
  for (int k = tid; k < n / 4; k += kThr) ((f32x4*)dst)[k] = ((const f32x4*)src)[k];
}

// Phases B and D for lane j of env n: where grucell.h's recurrences find their operands, the SoA
// scratch rows of sample i = t N + n.
template <int G>
struct GradFwdOps {
  const GruScratch& sc;
  const uint8_t* dones;
  int N, n, j;
  __device__ __forceinline__ GruFwdIn in(int t) const {
    const int64_t i = (int64_t)t * N + n;
    const float* gi = sc.gi + i * (3 * G);
    return GruFwdIn{gi[j], gi[G + j], gi[2 * G + j], dones[i] != 0};
  }
  __device__ __forceinline__ void store(int t, float hin, float r, float z, float nn, float ghn,
                                        float hout) const {
    const int64_t i = (int64_t)t * N + n;
    sc.hi[i * G + j] = hin;
    sc.r[i * G + j] = r;
    sc.z[i * G + j] = z;
    sc.n[i * G + j] = nn;
    sc.ghn[i * G + j] = ghn;
    sc.ho[i * G + j] = hout;
  }
};
template <int G>
struct GradBwdOps {
  const GruScratch& sc;
  const uint8_t* dones;
  int N, n, j;
  __device__ __forceinline__ GruBwdIn in(int t) const {
    const int64_t i = (int64_t)t * N + n;
    return GruBwdIn{sc.dho[i * G + j], sc.r[i * G + j], sc.z[i * G + j], sc.n[i * G + j],
                    sc.ghn[i * G + j], sc.hi[i * G + j], dones[i] != 0};
  }
  __device__ __forceinline__ int64_t row(int t) const { return ((int64_t)t * N + n) * (3 * G); }
  __device__ __forceinline__ float* dgi(int t) const { return sc.dgi + row(t); }
  __device__ __forceinline__ float* dgh(int t) const { return sc.dgh + row(t); }
};

// Sum over k = samples of A[s][m] B[s][n] for one 16 x 16 output tile: rows mt*16.., cols nt*16..
// of arrays with row strides lda / ldb (floats).  Lane (q, r) supplies A[s_{4kk+q}][16mt + r] and
// B[s_{4kk+q}][16nt + r]; the result D[4q + v][r] lands in register v.  s_k enumerates the
// workgroup's samples (t, e) as t * N + n0 + e, e < ne, in t-major order.
// The loads of kSumAhead k-steps are issued together (the loop is bound by their latency), the
// MFMAs still chain in k order: the same bits as one step at a time.  NE > 0: ne == NE, a
// compile-time divisor for the full workgroups.
constexpr int kSumAhead = 8;
template <int NE>
__device__ __forceinline__ f32x4 tile_sum(const float* __restrict__ A, int lda, int mt,
                                          const float* __restrict__ B, int ldb, int nt, int S,
                                          int ne_, int N, int n0, int q, int r) {
  const int ne = NE ? NE : ne_;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  int k0 = 0;
  for (; k0 + 4 * kSumAhead <= S; k0 += 4 * kSumAhead) {
    float av[kSumAhead], bv[kSumAhead];
#pragma unroll
    for (int u = 0; u < kSumAhead; ++u) {
      const int s = k0 + 4 * u + q;
      const int t = s / ne, e = s - t * ne;
      const int64_t i = (int64_t)t * N + n0 + e;
      av[u] = A[i * lda + 16 * mt + r];
      bv[u] = B[i * ldb + 16 * nt + r];
    }
#pragma unroll
    for (int u = 0; u < kSumAhead; ++u)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
  }
  for (; k0 < S; k0 += 4) {
    const int s = k0 + q;
    const bool ok = s < S;
    const int ss = ok ? s : S - 1;
    const int t = ss / ne, e = ss - t * ne;
    const int64_t i = (int64_t)t * N + n0 + e;
    const float a = ok ? A[i * lda + 16 * mt + r] : 0.0f;
    const float b = B[i * ldb + 16 * nt + r];
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }
  return acc;
}

// Phase A's base layer at 33 <= D <= 128, eight features of one sample:
// z[u] = bb[u] + sum_c Wb8[u][c] ob[c], c ascending as at D <= 32.  The observation row is
// re-read from the sample's scratch copy ob16 (D16 floats, zeros from D on, 16-byte aligned) 32
// columns at a time, so the registers that hold it are indexed at compile time only; the block
// that holds column D - 1, where it is not a full one, checks c < D.  Wb8: rows of D floats in LDS.
__device__ __forceinline__ void base8_wide(float (&z)[8], const float* bb, const float* Wb8, int D,
                                           int D16, const float* ob16) {
#pragma unroll
  for (int u = 0; u < 8; ++u) z[u] = bb[u];
  int c0 = 0;
#pragma unroll 1
  for (; c0 + 32 <= D; c0 += 32) {
    float ob[32];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const f32x4 v = *(const f32x4*)(ob16 + c0 + 4 * q);
      ob[4 * q] = v[0];
      ob[4 * q + 1] = v[1];
      ob[4 * q + 2] = v[2];
      ob[4 * q + 3] = v[3];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
#pragma unroll
      for (int k = 0; k < 32; ++k) z[u] += Wb8[u * D + c0 + k] * ob[k];
    }
  }
  if (c0 < D) {
    float ob[32];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (c0 + 4 * q < D16) v = *(const f32x4*)(ob16 + c0 + 4 * q);
      ob[4 * q] = v[0];
      ob[4 * q + 1] = v[1];
      ob[4 * q + 2] = v[2];
      ob[4 * q + 3] = v[3];
    }
#pragma unroll
    for (int k = 0; k < 32; ++k) {
      if (c0 + k < D) {
#pragma unroll
        for (int u = 0; u < 8; ++u) z[u] += Wb8[u * D + c0 + k] * ob[k];
      }
    }
  }
}

// The Gaussian form's arguments: the categorical kernel's, then where log_std sits in the flat
// layout and the per-sample rows [B][kAPad] of its gradient.  b.actions is float [T][N][A] here.
struct GruGaussArgs : GruArgs {
  int64_t ls_off;
  float* dls;
};
constexpr int kGaussLds = 2 * kAPad;  // exp(-log_std) | log_std, behind the categorical image

// WIDE_OBS: the form for 33 <= D <= 128 (dppo_gru_dims.wide_obs); phase A's base layer alone
// differs.  GAUSS: the Normal(mean, exp(log_std)) head; phase C's loss and phase F's log_std
// column alone differ.
template <int G, bool WIDE_OBS = false, bool GAUSS = false>
__global__ __launch_bounds__(kThr) void gru_grad_kernel(
    std::conditional_t<GAUSS, GruGaussArgs, GruArgs> a) {
  constexpr int kEnvs = kThr / G, G3 = 3 * G;
  static_assert(G3 % kGiBlk == 0 && G3 <= kThr && G % 16 == 0, "gate blocking");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const GruLds L = gru_lds(a.D, G);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n0 = blockIdx.x * kEnvs;
  const int ne = min(kEnvs, a.N - n0);
  const int T = a.T, N = a.N, D = a.D, A = a.A;
  const int S = T * ne;
  const float* P = a.params;
  const GruOffsets& po = a.po;
  const GruScratch& sc = a.sc;
  float* W = lds + L.W;

  // ---- biases (and the critic's output row) for the whole launch; phase A's weights
  if (tid < kH) {
    lds[L.bb + tid] = P[po.bb + tid];
    lds[L.ba1 + tid] = P[po.ba1 + tid];
    lds[L.bc1 + tid] = P[po.bc1 + tid];
    lds[L.Wc2 + tid] = P[po.Wc2 + tid];
  }
  if (tid < G3) {
    lds[L.bih + tid] = P[po.bih + tid];
    lds[L.bhh + tid] = P[po.bhh + tid];
  }
  if (tid < kAPad) lds[L.ba2 + tid] = tid < A ? P[po.ba2 + tid] : 0.f;
  if (tid == 0) lds[L.bc2] = P[po.bc2];
  if constexpr (GAUSS) {
    // 1 / sigma and log_std once per workgroup, zeros past A
    if (tid < kAPad) {
      const float ls = tid < A ? P[a.ls_off + tid] : 0.f;
      lds[L.total + tid] = tid < A ? expf(-ls) : 0.f;
      lds[L.total + kAPad + tid] = ls;
    }
  }
  float* Wb = W;
  float* Wih = W + kH * D;
  stage4(Wb, P + po.Wb, kH * D, tid);
  stage4(Wih, P + po.Wih, G3 * kH, tid);
  __syncthreads();

  // ---- A: x1 (8 features at a time), then gi in blocks of kGiBlk gate rows with x1 re-read
  // from the scratch row this thread just wrote.  At G = 16 the gates are one block, which
  // accumulates beside x1 instead (x1 still in registers): the form this width has always had,
  // kept because the compiler pairs the products of a re-read x1 for its packed instructions
  // the other way round and so contracts the other product of a pair -- not the same bits.
  // (The two forms share no helper: passing x1 as eight scalars changes how the blocks of the
  // wider instantiations are compiled.)
  constexpr bool kOneBlk = G3 == kGiBlk;
  for (int s = tid; s < S; s += kThr) {
    const int t = s / ne, e = s - t * ne;
    const int64_t i = (int64_t)t * N + n0 + e;
    {
      [[maybe_unused]] float ob[32];
      float* ob16 = sc.obs + i * a.D16;
      if constexpr (WIDE_OBS) {
        // the row goes to its D16-wide scratch row first; base8_wide re-reads it from there
#pragma unroll 1
        for (int c = 0; c < a.D16; c += 4) {
          f32x4 v;
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = c + k < D ? a.b.obs[i * D + c + k] : 0.f;
          *(f32x4*)(ob16 + c) = v;
        }
      } else {
#pragma unroll
        for (int c = 0; c < 32; ++c) ob[c] = c < D ? a.b.obs[i * D + c] : 0.f;
#pragma unroll
        for (int c = 0; c < 32; ++c)
          if (c < a.D16) ob16[c] = ob[c];
      }
      [[maybe_unused]] float gi[kOneBlk ? kGiBlk : 1];
      if constexpr (kOneBlk) {
#pragma unroll
        for (int g = 0; g < kGiBlk; ++g) gi[g] = lds[L.bih + g];
      }
#pragma unroll 1
      for (int o0 = 0; o0 < kH; o0 += 8) {
        float x[8];
        if constexpr (WIDE_OBS) base8_wide(x, lds + L.bb + o0, Wb + o0 * D, D, a.D16, ob16);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          float z;
          if constexpr (WIDE_OBS) {
            z = x[u];
          } else {
            z = lds[L.bb + o0 + u];
#pragma unroll
            for (int c = 0; c < 32; ++c)
              if (c < D) z += Wb[(o0 + u) * D + c] * ob[c];
          }
          x[u] = tanh_acc(z);
        }
        f32x4* xo = (f32x4*)(sc.x1 + i * kH + o0);
        xo[0] = (f32x4){x[0], x[1], x[2], x[3]};
        xo[1] = (f32x4){x[4], x[5], x[6], x[7]};
        if constexpr (kOneBlk) {
#pragma unroll
          for (int g = 0; g < kGiBlk; ++g) {
            const f32x4 w0 = *(const f32x4*)(Wih + g * kH + o0);
            const f32x4 w1 = *(const f32x4*)(Wih + g * kH + o0 + 4);
            gi[g] += ((w0[0] * x[0] + w0[1] * x[1]) + (w0[2] * x[2] + w0[3] * x[3])) +
                     ((w1[0] * x[4] + w1[1] * x[5]) + (w1[2] * x[6] + w1[3] * x[7]));
          }
        }
      }
      if constexpr (kOneBlk) {
        f32x4* go = (f32x4*)(sc.gi + i * G3);
#pragma unroll
        for (int g = 0; g < kGiBlk / 4; ++g)
          go[g] = (f32x4){gi[4 * g], gi[4 * g + 1], gi[4 * g + 2], gi[4 * g + 3]};
      }
    }
    if constexpr (!kOneBlk) {
#pragma unroll 1
      for (int g0 = 0; g0 < G3; g0 += kGiBlk) {
        float gi[kGiBlk];
#pragma unroll
        for (int g = 0; g < kGiBlk; ++g) gi[g] = lds[L.bih + g0 + g];
        const float* wrow = Wih + g0 * kH;
#pragma unroll 1
        for (int o0 = 0; o0 < kH; o0 += 8) {
          const f32x4 xa = *(const f32x4*)(sc.x1 + i * kH + o0);
          const f32x4 xb = *(const f32x4*)(sc.x1 + i * kH + o0 + 4);
#pragma unroll
          for (int g = 0; g < kGiBlk; ++g) {
            const f32x4 w0 = *(const f32x4*)(wrow + g * kH + o0);
            const f32x4 w1 = *(const f32x4*)(wrow + g * kH + o0 + 4);
            gi[g] += ((w0[0] * xa[0] + w0[1] * xa[1]) + (w0[2] * xa[2] + w0[3] * xa[3])) +
                     ((w1[0] * xb[0] + w1[1] * xb[1]) + (w1[2] * xb[2] + w1[3] * xb[3]));
          }
        }
        f32x4* go = (f32x4*)(sc.gi + i * G3 + g0);
#pragma unroll
        for (int g = 0; g < kGiBlk / 4; ++g)
          go[g] = (f32x4){gi[4 * g], gi[4 * g + 1], gi[4 * g + 2], gi[4 * g + 3]};
      }
    }
  }
  __syncthreads();
  // 16-byte loads, as stage4's: params is 16-byte aligned (checked at the C ABI) and every
  // offset of the layout is a multiple of 16 floats (gru_layout)
  stage_whh<G, kThr>(W, P + po.Whh, tid);
  __syncthreads();

  // ---- B: forward recurrence (grucell.h), lane j of env e = hidden unit j (G lanes of one wave
  // per env)
  const int e = tid / G, j = tid % G;
  const bool env_ok = e < ne;
  const int n = n0 + e;
  if (env_ok)
    gru_seq_fwd<G>(W, lds + L.bhh, lds + L.hbuf + e * G, j, a.b.hx0[(int64_t)n * G + j], T,
                   GradFwdOps<G>{sc, a.b.prev_dones, N, n, j});
  __syncthreads();
  float* Wa1 = W;
  float* Wc1 = W + kH * G;
  float* Wa2 = W + 2 * kH * G;
  stage4(Wa1, P + po.Wa1, kH * G, tid);
  stage4(Wc1, P + po.Wc1, kH * G, tid);
  for (int k = tid; k < kAPad * kH; k += kThr) Wa2[k] = (k >> 6) < A ? P[po.Wa2 + k] : 0.f;
  __syncthreads();

  // ---- C: heads, loss and head backward per sample (ppo.py:264-280 with the GRU features).
  // Forward 8 head features at a time (stored, and folded into the logits / value at once);
  // backward the same blocks re-read from the scratch rows this thread just wrote.
  float s_pi = 0.f, s_v = 0.f, s_ent = 0.f;
  for (int s = tid; s < S; s += kThr) {
    const int t = s / ne, ee = s - t * ne;
    const int64_t i = (int64_t)t * N + n0 + ee;
    const float w = a.wmask[i];
    float dl[kAPad];
    float dv = 0.f;
#pragma unroll
    for (int k = 0; k < kAPad; ++k) dl[k] = 0.f;
    float* yar = sc.ya + i * kH;
    float* ycr = sc.yc + i * kH;
    float* dyar = sc.dya + i * kH;
    float* dycr = sc.dyc + i * kH;
    f32x4* dhor = (f32x4*)(sc.dho + i * G);
    if (w != 0.f) {
      float out[kAPad];
#pragma unroll
      for (int k = 0; k < kAPad; ++k) out[k] = lds[L.ba2 + k];
      float val = lds[L.bc2];
      {
        float hv[G];
#pragma unroll
        for (int q = 0; q < G / 4; ++q) {
          const f32x4 x = ((const f32x4*)(sc.ho + i * G))[q];
          hv[4 * q] = x[0];
          hv[4 * q + 1] = x[1];
          hv[4 * q + 2] = x[2];
          hv[4 * q + 3] = x[3];
        }
#pragma unroll 1
        for (int o0 = 0; o0 < kH; o0 += 8) {
          float ya[8], yc[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            float za = lds[L.ba1 + o0 + u], zc = lds[L.bc1 + o0 + u];
#pragma unroll
            for (int q = 0; q < G / 4; ++q) {
              const f32x4 wa = *(const f32x4*)(Wa1 + (o0 + u) * G + 4 * q);
              const f32x4 wc = *(const f32x4*)(Wc1 + (o0 + u) * G + 4 * q);
              za += (wa[0] * hv[4 * q] + wa[1] * hv[4 * q + 1]) + (wa[2] * hv[4 * q + 2] + wa[3] * hv[4 * q + 3]);
              zc += (wc[0] * hv[4 * q] + wc[1] * hv[4 * q + 1]) + (wc[2] * hv[4 * q + 2] + wc[3] * hv[4 * q + 3]);
            }
            ya[u] = tanh_acc(za);
            yc[u] = tanh_acc(zc);
          }
          ((f32x4*)(yar + o0))[0] = (f32x4){ya[0], ya[1], ya[2], ya[3]};
          ((f32x4*)(yar + o0))[1] = (f32x4){ya[4], ya[5], ya[6], ya[7]};
          ((f32x4*)(ycr + o0))[0] = (f32x4){yc[0], yc[1], yc[2], yc[3]};
          ((f32x4*)(ycr + o0))[1] = (f32x4){yc[4], yc[5], yc[6], yc[7]};
#pragma unroll
          for (int k = 0; k < kAPad; ++k) {
            if (k < A) {
              const f32x4 w0 = *(const f32x4*)(Wa2 + k * kH + o0);
              const f32x4 w1 = *(const f32x4*)(Wa2 + k * kH + o0 + 4);
              out[k] += ((w0[0] * ya[0] + w0[1] * ya[1]) + (w0[2] * ya[2] + w0[3] * ya[3])) +
                        ((w1[0] * ya[4] + w1[1] * ya[5]) + (w1[2] * ya[6] + w1[3] * ya[7]));
            }
          }
          const f32x4 v0 = *(const f32x4*)(lds + L.Wc2 + o0);
          const f32x4 v1 = *(const f32x4*)(lds + L.Wc2 + o0 + 4);
          val += ((v0[0] * yc[0] + v0[1] * yc[1]) + (v0[2] * yc[2] + v0[3] * yc[3])) +
                 ((v1[0] * yc[4] + v1[1] * yc[5]) + (v1[2] * yc[6] + v1[3] * yc[7]));
        }
      }
      [[maybe_unused]] int act = 0;
      float ent = 0.f, logp = 0.f;
      if constexpr (GAUSS) {
        // JointNormal(mean, exp(log_std)) (continuous_ppo.py:41-47, :276-277): out[] holds the
        // means; z_k = (a_k - mean_k) / sigma_k replaces them
        const float* av = (const float*)a.b.actions + i * A;
#pragma unroll
        for (int k = 0; k < kAPad; ++k) {
          const float ls = lds[L.total + kAPad + k];
          const float z = k < A ? (av[k] - out[k]) * lds[L.total + k] : 0.f;
          if (k < A) {
            logp += -0.5f * z * z - ls - 0.91893853320467274178f;
            ent += 1.41893853320467274178f + ls;
          }
          out[k] = z;
        }
      } else {
      act = a.b.actions[i];
      float mx = out[0];
#pragma unroll
      for (int k = 1; k < kAPad; ++k)
        if (k < A) mx = fmaxf(mx, out[k]);
      float se = 0.f;
#pragma unroll
      for (int k = 0; k < kAPad; ++k)
        if (k < A) se += __expf(out[k] - mx);
      const float lse = mx + __logf(se);
#pragma unroll
      for (int k = 0; k < kAPad; ++k) {
        const float lpk = out[k] - lse;
        const float pk = k < A ? __expf(lpk) : 0.f;
        ent -= pk * lpk;
        logp = k == act ? lpk : logp;
        out[k] = lpk;  // log-probabilities from here on
      }
      }
      const float adv = a.b.advantages[i], ret = a.b.returns[i];
      const float ratio = __expf(logp - a.b.old_log_probs[i]);                 // ppo.py:266
      const float rcl = fminf(fmaxf(ratio, 1.0f - a.clip_eps), 1.0f + a.clip_eps);
      const float u = -adv * ratio, wv = -adv * rcl;                            // ppo.py:267-269
      const float inr = (ratio >= 1.0f - a.clip_eps && ratio <= 1.0f + a.clip_eps) ? 1.f : 0.f;
      const float gu = u > wv ? 1.f : (u == wv ? 0.5f : 0.f);  // torch.max splits ties
      const float gw = wv > u ? 1.f : (u == wv ? 0.5f : 0.f);
      const float vm = w * a.inv_m;
      const float dlogp = (gu * -adv + gw * -adv * inr) * vm * ratio;
      dv = a.vf * (val - ret) * vm;                                            // ppo.py:272
      s_pi += fmaxf(u, wv);
      s_v += 0.5f * (val - ret) * (val - ret);
      s_ent += ent;
      if constexpr (GAUSS) {
        // d logp / d mean_k = z_k / sigma_k, d logp / d log_std_k = z_k^2 - 1; the entropy's
        // log_std derivative (1 per dimension) rides in the sample's row, so the ranks' slabs
        // sum to the union minibatch's -ent once
        float* dlsr = a.dls + i * kAPad;
#pragma unroll
        for (int k = 0; k < kAPad; ++k) {
          const float z = out[k];
          dl[k] = k < A ? dlogp * z * lds[L.total + k] : 0.f;
          out[k] = k < A ? dlogp * (z * z - 1.0f) - a.ent * vm : 0.f;
        }
#pragma unroll
        for (int k = 0; k < kAPad / 4; ++k)
          ((f32x4*)dlsr)[k] = (f32x4){out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]};
      } else {
#pragma unroll
      for (int k = 0; k < kAPad; ++k) {
        const float pk = k < A ? __expf(out[k]) : 0.f;
        dl[k] = k < A ? dlogp * ((k == act ? 1.f : 0.f) - pk) + a.ent * vm * pk * (out[k] + ent)
                      : 0.f;
      }
      }
      // head backward: dya = (Wa2^T dl)(1 - ya^2), dyc = Wc2 dv (1 - yc^2),
      // dh' = Wa1^T dya + Wc1^T dyc
      float dho[G];
#pragma unroll
      for (int k = 0; k < G; ++k) dho[k] = 0.f;
#pragma unroll 1
      for (int o0 = 0; o0 < kH; o0 += 4) {
        const f32x4 ya = *(const f32x4*)(yar + o0);
        const f32x4 yc = *(const f32x4*)(ycr + o0);
        f32x4 da = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < kAPad; ++k)
          if (k < A) da += *(const f32x4*)(Wa2 + k * kH + o0) * dl[k];
        const f32x4 dya = da * (1.0f - ya * ya);
        const f32x4 dyc = *(const f32x4*)(lds + L.Wc2 + o0) * dv * (1.0f - yc * yc);
        *(f32x4*)(dyar + o0) = dya;
        *(f32x4*)(dycr + o0) = dyc;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
          for (int q = 0; q < G / 4; ++q) {
            const f32x4 wa = *(const f32x4*)(Wa1 + (o0 + u) * G + 4 * q);
            const f32x4 wc = *(const f32x4*)(Wc1 + (o0 + u) * G + 4 * q);
#pragma unroll
            for (int x = 0; x < 4; ++x) dho[4 * q + x] += wa[x] * dya[u] + wc[x] * dyc[u];
          }
        }
      }
#pragma unroll
      for (int k = 0; k < G / 4; ++k)
        dhor[k] = (f32x4){dho[4 * k], dho[4 * k + 1], dho[4 * k + 2], dho[4 * k + 3]};
    } else {
      const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int o = 0; o < kH / 4; ++o) {
        ((f32x4*)yar)[o] = zero;
        ((f32x4*)ycr)[o] = zero;
        ((f32x4*)dyar)[o] = zero;
        ((f32x4*)dycr)[o] = zero;
      }
#pragma unroll
      for (int k = 0; k < G / 4; ++k) dhor[k] = zero;
      if constexpr (GAUSS) {
#pragma unroll
        for (int k = 0; k < kAPad / 4; ++k) ((f32x4*)(a.dls + i * kAPad))[k] = zero;
      }
    }
#pragma unroll
    for (int k = 0; k < kAPad / 4; ++k)
      ((f32x4*)(sc.dl + i * kAPad))[k] = (f32x4){dl[4 * k], dl[4 * k + 1], dl[4 * k + 2], dl[4 * k + 3]};
    ((f32x4*)(sc.dv + i * kAPad))[0] = (f32x4){dv, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 1; k < kAPad / 4; ++k) ((f32x4*)(sc.dv + i * kAPad))[k] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  __syncthreads();
  stage_whh<G, kThr>(W, P + po.Whh, tid);
  __syncthreads();

  // ---- D: BPTT, reverse in t (lane j of env e reads column j of Whh)
  if (env_ok)
    gru_seq_bwd<G>(W, lds + L.gbuf + e * G3, j, 0.0f, T,
                   GradBwdOps<G>{sc, a.b.prev_dones, N, n, j});
  __syncthreads();
  stage4(W, P + po.Wih, G3 * kH, tid);
  __syncthreads();

  // ---- E: dx1 = (Wih^T dgi)(1 - x1^2) per sample: all 64 features accumulate in registers
  // while the sample's dgi streams through four gate rows at a time
  for (int s = tid; s < S; s += kThr) {
    const int t = s / ne, ee = s - t * ne;
    const int64_t i = (int64_t)t * N + n0 + ee;
    f32x4 d[kH / 4];
#pragma unroll
    for (int c = 0; c < kH / 4; ++c) d[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const f32x4* dgr = (const f32x4*)(sc.dgi + i * G3);
#pragma unroll 1
    for (int g0 = 0; g0 < G3; g0 += 4) {
      const f32x4 dg = dgr[g0 / 4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int c = 0; c < kH / 4; ++c) d[c] += *(const f32x4*)(W + (g0 + u) * kH + 4 * c) * dg[u];
      }
    }
    const f32x4* x1 = (const f32x4*)(sc.x1 + i * kH);
    f32x4* dx = (f32x4*)(sc.dx1 + i * kH);
#pragma unroll
    for (int c = 0; c < kH / 4; ++c) {
      const f32x4 x = x1[c];
      dx[c] = d[c] * (1.0f - x * x);
    }
  }
  __syncthreads();

  // ---- F: weight gradients (MFMA over samples), biases and loss sums into this workgroup's slab
  float* slab = a.slabs + (int64_t)blockIdx.x * a.slab_stride;
  {
    const int q = lane >> 4, r = lane & 15;
    const int nD = a.D16 / 16;
    constexpr int nG = G / 16, nG3 = G3 / 16;
    // tiles: Wb 4 x nD | Wih 3G/16 x 4 | Whh 3G/16 x G/16 | Wa1 4 x G/16 | Wc1 4 x G/16 |
    //        Wa2 1 x 4 | Wc2 1 x 4
    const int nt_b = 4 * nD, nt_ih = nG3 * 4, nt_hh = nG3 * nG, nt_a1 = 4 * nG, nt_c1 = 4 * nG,
              nt_a2 = 4, nt_c2 = 4;
    const int ntiles = nt_b + nt_ih + nt_hh + nt_a1 + nt_c1 + nt_a2 + nt_c2;
    for (int tl = wave; tl < ntiles; tl += kThr / 64) {
      int k = tl;
      const float *Aa, *Bb;
      int lda, ldb, mt, nt, rows, cols, ldo;
      int64_t off;
      if (k < nt_b) {
        Aa = sc.dx1; lda = kH; Bb = sc.obs; ldb = a.D16; mt = k / nD; nt = k % nD;
        off = po.Wb; rows = kH; cols = D; ldo = D;
      } else if ((k -= nt_b) < nt_ih) {
        Aa = sc.dgi; lda = G3; Bb = sc.x1; ldb = kH; mt = k / 4; nt = k % 4;
        off = po.Wih; rows = G3; cols = kH; ldo = kH;
      } else if ((k -= nt_ih) < nt_hh) {
        Aa = sc.dgh; lda = G3; Bb = sc.hi; ldb = G; mt = k / nG; nt = k % nG;
        off = po.Whh; rows = G3; cols = G; ldo = G;
      } else if ((k -= nt_hh) < nt_a1) {
        Aa = sc.dya; lda = kH; Bb = sc.ho; ldb = G; mt = k / nG; nt = k % nG;
        off = po.Wa1; rows = kH; cols = G; ldo = G;
      } else if ((k -= nt_a1) < nt_c1) {
        Aa = sc.dyc; lda = kH; Bb = sc.ho; ldb = G; mt = k / nG; nt = k % nG;
        off = po.Wc1; rows = kH; cols = G; ldo = G;
      } else if ((k -= nt_c1) < nt_a2) {
        Aa = sc.dl; lda = kAPad; Bb = sc.ya; ldb = kH; mt = 0; nt = k;
        off = po.Wa2; rows = A; cols = kH; ldo = kH;
      } else {
        k -= nt_a2;
        Aa = sc.dv; lda = kAPad; Bb = sc.yc; ldb = kH; mt = 0; nt = k;
        off = po.Wc2; rows = 1; cols = kH; ldo = kH;
      }
      const f32x4 acc = ne == kEnvs ? tile_sum<kEnvs>(Aa, lda, mt, Bb, ldb, nt, S, ne, N, n0, q, r)
                                    : tile_sum<0>(Aa, lda, mt, Bb, ldb, nt, S, ne, N, n0, q, r);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int row = 16 * mt + 4 * q + v, col = 16 * nt + r;
        if (row < rows && col < cols) slab[off + (int64_t)row * ldo + col] = acc[v];
      }
    }
  }
  {
    // bias columns: bb 64 | bih 3G | bhh 3G | ba1 64 | bc1 64 | ba2 A | bc2 1 | (GAUSS) log_std A
    const int nb = kH + G3 + G3 + kH + kH + A + 1 + (GAUSS ? A : 0);
    for (int c = tid; c < nb; c += kThr) {
      const float* src;
      int ld, col;
      int64_t off;
      int k = c;
      if (k < kH) { src = sc.dx1; ld = kH; col = k; off = po.bb + k; }
      else if ((k -= kH) < G3) { src = sc.dgi; ld = G3; col = k; off = po.bih + k; }
      else if ((k -= G3) < G3) { src = sc.dgh; ld = G3; col = k; off = po.bhh + k; }
      else if ((k -= G3) < kH) { src = sc.dya; ld = kH; col = k; off = po.ba1 + k; }
      else if ((k -= kH) < kH) { src = sc.dyc; ld = kH; col = k; off = po.bc1 + k; }
      else if ((k -= kH) < A) { src = sc.dl; ld = kAPad; col = k; off = po.ba2 + k; }
      else {
        src = sc.dv; ld = kAPad; col = 0; off = po.bc2;
        if constexpr (GAUSS) {
          if ((k -= A) > 0) { src = a.dls; col = k - 1; off = a.ls_off + k - 1; }
        }
      }
      // sample order s = 0, 1, ...; the loads of kSumAhead samples in flight together
      float sum = 0.f;
      int s = 0;
      for (; s + kSumAhead <= S; s += kSumAhead) {
        float v[kSumAhead];
#pragma unroll
        for (int u = 0; u < kSumAhead; ++u) {
          const int t = (s + u) / ne, ee = (s + u) - t * ne;
          v[u] = src[((int64_t)t * N + n0 + ee) * ld + col];
        }
#pragma unroll
        for (int u = 0; u < kSumAhead; ++u) sum += v[u];
      }
      for (; s < S; ++s) {
        const int t = s / ne, ee = s - t * ne;
        sum += src[((int64_t)t * N + n0 + ee) * ld + col];
      }
      slab[off] = sum;
    }
  }
  // loss sums {policy, value, entropy} in a fixed order
  float* red = lds + L.red;
  red[tid] = s_pi;
  red[kThr + tid] = s_v;
  red[2 * kThr + tid] = s_ent;
  __syncthreads();
  if (tid < 3) {
    float sum = 0.f;
    for (int k = 0; k < kThr; ++k) sum += red[tid * kThr + k];
    slab[a.p_total + tid] = sum;
  }
}

__global__ void mask_kernel(const int32_t* __restrict__ idx, int m, float* __restrict__ wmask) {
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < m; k += gridDim.x * blockDim.x)
    wmask[idx[k]] = 1.0f;
}

template <int G>
int launch_g(const GruArgs& a, hipStream_t s) {
  static const bool attr = [] {
    raise_dyn_lds((const void*)gru_grad_kernel<G>);
    raise_dyn_lds((const void*)gru_grad_kernel<G, true>);
    return true;
  }();
  (void)attr;
  const dim3 grid(gru_grid(a.N, G));
  if (a.D > 32)
    DPPO_LAUNCH((gru_grad_kernel<G, true>), grid, dim3(kThr), gru_lds_bytes(a.D, G), s, a);
  else
    DPPO_LAUNCH(gru_grad_kernel<G>, grid, dim3(kThr), gru_lds_bytes(a.D, G), s, a);
  DPPO_LAUNCH_CHECK();
  return DPPO_OK;
}

template <int G>
int launch_g_gauss(const GruGaussArgs& a, hipStream_t s) {
  static const bool attr = [] {
    raise_dyn_lds((const void*)gru_grad_kernel<G, false, true>);
    raise_dyn_lds((const void*)gru_grad_kernel<G, true, true>);
    return true;
  }();
  (void)attr;
  const dim3 grid(gru_grid(a.N, G));
  const size_t lds = gru_gauss_lds_bytes(a.D, G);
  if (a.D > 32)
    DPPO_LAUNCH((gru_grad_kernel<G, true, true>), grid, dim3(kThr), lds, s, a);
  else
    DPPO_LAUNCH((gru_grad_kernel<G, false, true>), grid, dim3(kThr), lds, s, a);
  DPPO_LAUNCH_CHECK();
  return DPPO_OK;
}

}  // namespace

int gru_envs(int G) { return kThr / G; }

int gru_grid(int N, int G) { return (N + gru_envs(G) - 1) / gru_envs(G); }

size_t gru_lds_bytes(int D, int G) { return (size_t)gru_lds(D, G).total * sizeof(float); }

size_t gru_gauss_lds_bytes(int D, int G) {
  return (size_t)(gru_lds(D, G).total + kGaussLds) * sizeof(float);
}

namespace {

int build_mask(const int32_t* idx, int32_t m, float* wmask, int64_t B, hipStream_t s) {
  DPPO_HIP_CHECK(hipMemsetAsync(wmask, 0, (size_t)B * sizeof(float), s));
  if (m > 0) {
    int g = (m + 255) / 256;
    if (g > 1024) g = 1024;
    DPPO_LAUNCH(mask_kernel, dim3(g), dim3(256), 0, s, idx, m, wmask);
    DPPO_LAUNCH_CHECK();
  }
  return DPPO_OK;
}

}  // namespace

int launch_gru_gauss_grad(int G, const GruOffsets& po, int64_t ls_off, const float* params,
                          const dppo_gru_gauss_batch& b, const int32_t* idx, int32_t m,
                          float* wmask, int64_t B, int T, int N, int D, int A, float inv_m,
                          float clip_eps, float vf, float ent, const GruScratch& sc, float* dls,
                          float* slabs, int64_t slab_stride, int64_t p_total, hipStream_t s) {
  int rc = build_mask(idx, m, wmask, B, s);
  if (rc != DPPO_OK) return rc;
  GruGaussArgs a{};
  a.po = po;
  a.params = params;
  // the two batch structs differ in the element type behind `actions` alone
  a.b = dppo_gru_batch{b.obs, (const int32_t*)(const void*)b.actions, b.old_log_probs,
                       b.advantages, b.returns, b.prev_dones, b.hx0};
  a.wmask = wmask;
  a.T = T;
  a.N = N;
  a.D = D;
  a.D16 = (D + 15) / 16 * 16;
  a.A = A;
  a.inv_m = inv_m;
  a.clip_eps = clip_eps;
  a.vf = vf;
  a.ent = ent;
  a.sc = sc;
  a.slabs = slabs;
  a.slab_stride = slab_stride;
  a.p_total = p_total;
  a.ls_off = ls_off;
  a.dls = dls;
  if (!dispatch_gru_width(G, [&](auto g) { rc = launch_g_gauss<decltype(g)::value>(a, s); })) {
    set_error("no GRU gradient kernel for gru_hidden=%d", G);
    return DPPO_EUNSUPPORTED;
  }
  return rc;
}

int launch_gru_grad(int G, const GruOffsets& po, const float* params, const dppo_gru_batch& b,
                    const int32_t* idx, int32_t m, float* wmask, int64_t B, int T, int N, int D,
                    int A, float inv_m, float clip_eps, float vf, float ent, const GruScratch& sc,
                    float* slabs, int64_t slab_stride, int64_t p_total, hipStream_t s) {
  int rc = build_mask(idx, m, wmask, B, s);
  if (rc != DPPO_OK) return rc;
  GruArgs a{};
  a.po = po;
  a.params = params;
  a.b = b;
  a.wmask = wmask;
  a.T = T;
  a.N = N;
  a.D = D;
  a.D16 = (D + 15) / 16 * 16;
  a.A = A;
  a.inv_m = inv_m;
  a.clip_eps = clip_eps;
  a.vf = vf;
  a.ent = ent;
  a.sc = sc;
  a.slabs = slabs;
  a.slab_stride = slab_stride;
  a.p_total = p_total;
  if (!dispatch_gru_width(G, [&](auto g) { rc = launch_g<decltype(g)::value>(a, s); })) {
    set_error("no GRU gradient kernel for gru_hidden=%d", G);
    return DPPO_EUNSUPPORTED;
  }
  return rc;
}

}  // namespace dppo
