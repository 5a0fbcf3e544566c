// RecurrentPPO rollout step, fused (intended semantics of reference diamond/recurrent_ppo.py:214-245
// with the network of :94-149 and the hidden reset of :82-87; restated for T = 1 in
// oracle/gru_torch.py::sequence): what rollout() ran under torch as several dozen launches per env
// step is one launch for the policy step (gru_act_kernel: base, GRU cell, both heads, Categorical
// draw, log-prob) and one for V(next_obs) (gru_value_kernel: base, GRU cell, critic head).
//
// Mapping: 16 lanes per env (lane j = hidden unit j, gru.hip's phase-B mapping), 4 envs per
// wave, one wave per workgroup.  Lane j computes base features j, j+16, j+32, j+48, the three
// gate rows j, the head features j + 16q, and logit j; per-env vectors pass between the steps
// through 768 B of LDS per env.  The ~36 KB of parameters are read straight from global memory
// (L2-resident after the first workgroup; a row is read by the four envs of a wave at once):
// staging them in LDS would cost every workgroup a full 36 KB copy, which the 8 workgroups of
// num_envs = 32 could not amortise, and at n = 8192 the 2048 one-wave workgroups spread 8 waves
// over every CU without it.
//
// Every sum runs in a fixed order inside the env's own 16 lanes (the value's 16 partials through
// row-local DPP), so a sample's outputs are the same bits at any n, at any position in the batch
// and on any grid.  Lanes past n clamp to env n - 1 (valid addresses) and store nothing.
#include "common.h"
#include "philox.h"

namespace dppo {
namespace {

constexpr int kG = 16;         // GRU hidden
constexpr int kH = 64;         // MLP hidden
constexpr int kEnvsPerWg = 4;  // one wave
constexpr int kThr = kEnvsPerWg * kG;

struct GruStepArgs {
  GruOffsets po;
  const float* params;
  const float* obs;
  const uint8_t* dones;  // null: no reset
  const float* hx;
  float* hx_out;
  int32_t* actions;
  float* log_probs;
  float* values;
  float* logits;
  int64_t n;
  int D, A;
  uint32_t seed_lo, seed_hi, ctr_lo, ctr_hi;
};

// per-env LDS vectors (floats)
struct EnvLds {
  float obs[32];
  float x1[kH];
  float h[kG];
  float ya[kH];
  float lg[kG];
};

__device__ __forceinline__ float dot4(f32x4 w, f32x4 x) {
  return (w[0] * x[0] + w[1] * x[1]) + (w[2] * x[2] + w[3] * x[3]);
}

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float x) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}

// Sum over the 16 lanes of a DPP row (= one env), the same bits in every lane: xor 1, xor 2,
// half-row mirror, row mirror.
__device__ __forceinline__ float row_sum(float x) {
  x += dpp_f32<0xB1>(x);   // quad_perm [1,0,3,2]
  x += dpp_f32<0x4E>(x);   // quad_perm [2,3,0,1]
  x += dpp_f32<0x141>(x);  // row_half_mirror
  x += dpp_f32<0x140>(x);  // row_mirror
  return x;
}

// tanh(W1 v + b1) for head features j + 16q, q < 4; W1 [64][16], v [16] in LDS
__device__ __forceinline__ void head_hidden(const float* __restrict__ W1,
                                            const float* __restrict__ b1, const float* v, int j,
                                            float (&y)[4]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int o = j + 16 * q;
    const f32x4* w = (const f32x4*)(W1 + o * kG);
    float z = b1[o];
#pragma unroll
    for (int k = 0; k < kG / 4; ++k) z += dot4(w[k], ((const f32x4*)v)[k]);
    y[q] = tanh_acc(z);
  }
}

// Base layer, hidden reset and one GRU step for env slot `e` of the workgroup; on return E.h
// holds the new hidden state (all 16 lanes of the env see it) and the return value is lane j's
// own element.
__device__ __forceinline__ float gru_forward(const GruStepArgs& a, EnvLds& E, int64_t ic, int j) {
  const float* P = a.params;
  const GruOffsets& po = a.po;
  const int D = a.D;
  for (int c = j; c < D; c += kG) E.obs[c] = a.obs[ic * D + c];
  const bool reset = a.dones && a.dones[ic];
  const float h = reset ? 0.0f : a.hx[ic * kG + j];  // hx[:, dones] = 0 (recurrent_ppo.py:84)
  E.h[j] = h;
  __syncthreads();
  // x1 = tanh(Wb obs + bb), features j + 16q
  {
    float z[4];
    const float* w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      z[q] = P[po.bb + j + 16 * q];
      w[q] = P + po.Wb + (int64_t)(j + 16 * q) * D;
    }
#pragma unroll 4
    for (int c = 0; c < D; ++c) {
      const float o = E.obs[c];
#pragma unroll
      for (int q = 0; q < 4; ++q) z[q] += w[q][c] * o;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) E.x1[j + 16 * q] = tanh_acc(z[q]);
  }
  __syncthreads();
  // gates: gi = Wih x1 + bih, gh = Whh h + bhh, rows j (r), 16 + j (z), 32 + j (n)
  float gi[3], gh[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    const int row = g * kG + j;
    const f32x4* wi = (const f32x4*)(P + po.Wih + row * kH);
    const f32x4* wh = (const f32x4*)(P + po.Whh + row * kG);
    float si = P[po.bih + row], sh = P[po.bhh + row];
#pragma unroll
    for (int k = 0; k < kH / 4; ++k) si += dot4(wi[k], ((const f32x4*)E.x1)[k]);
#pragma unroll
    for (int k = 0; k < kG / 4; ++k) sh += dot4(wh[k], ((const f32x4*)E.h)[k]);
    gi[g] = si;
    gh[g] = sh;
  }
  const float r = sigm(gi[0] + gh[0]), z = sigm(gi[1] + gh[1]);
  const float nn = tanh_acc(gi[2] + r * gh[2]);
  const float hn = (1.0f - z) * nn + z * h;
  __syncthreads();  // every lane has read E.h
  E.h[j] = hn;
  __syncthreads();
  return hn;
}

// critic head on E.h: Linear(16, 64) tanh Linear(64, 1)
__device__ __forceinline__ float critic_value(const GruStepArgs& a, const EnvLds& E, int j) {
  const float* P = a.params;
  float yc[4];
  head_hidden(P + a.po.Wc1, P + a.po.bc1, E.h, j, yc);
  float part = 0.0f;
#pragma unroll
  for (int q = 0; q < 4; ++q) part += P[a.po.Wc2 + j + 16 * q] * yc[q];
  return P[a.po.bc2] + row_sum(part);
}

__global__ __launch_bounds__(kThr) void gru_act_kernel(GruStepArgs a) {
  __shared__ __attribute__((aligned(16))) EnvLds lds[kEnvsPerWg];
  const int e = threadIdx.x >> 4, j = threadIdx.x & 15;
  const int64_t i = (int64_t)blockIdx.x * kEnvsPerWg + e;
  const bool valid = i < a.n;
  const int64_t ic = valid ? i : a.n - 1;
  EnvLds& E = lds[e];
  const float* P = a.params;
  const int A = a.A;

  const float hn = gru_forward(a, E, ic, j);
  if (valid) a.hx_out[i * kG + j] = hn;
  const float value = critic_value(a, E, j);

  // actor head: Linear(16, 64) tanh Linear(64, A); lane k < A computes logit k
  float ya[4];
  head_hidden(P + a.po.Wa1, P + a.po.ba1, E.h, j, ya);
#pragma unroll
  for (int q = 0; q < 4; ++q) E.ya[j + 16 * q] = ya[q];
  __syncthreads();
  {
    const int k = j < A ? j : A - 1;
    const f32x4* w = (const f32x4*)(P + a.po.Wa2 + k * kH);
    float lg = P[a.po.ba2 + k];
#pragma unroll
    for (int q = 0; q < kH / 4; ++q) lg += dot4(w[q], ((const f32x4*)E.ya)[q]);
    E.lg[j] = lg;
    if (valid && a.logits && j < A) a.logits[i * A + j] = lg;
  }
  __syncthreads();
  if (!valid || j != 0) return;

  // Categorical(logits).sample() by inverse CDF on one uniform (as mlp.hip act_kernel), and the
  // log-prob of the draw with accurate expf / logf
  float out[kG];
#pragma unroll
  for (int q = 0; q < kG / 4; ++q) {
    const f32x4 x = ((const f32x4*)E.lg)[q];
    out[4 * q] = x[0];
    out[4 * q + 1] = x[1];
    out[4 * q + 2] = x[2];
    out[4 * q + 3] = x[3];
  }
  float mx = out[0];
#pragma unroll
  for (int k = 1; k < kG; ++k)
    if (k < A) mx = fmaxf(mx, out[k]);
  float ex[kG], se = 0.0f;
#pragma unroll
  for (int k = 0; k < kG; ++k) {
    ex[k] = k < A ? expf(out[k] - mx) : 0.0f;
    se += ex[k];
  }
  uint32_t c[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), a.ctr_lo, a.ctr_hi};
  philox4x32(c, a.seed_lo, a.seed_hi);
  // the first k whose cumulative mass exceeds u * sum (the last action takes the remainder)
  const float target = u01(c[0]) * se;
  int pick = A - 1;
  float cum = 0.0f;
#pragma unroll
  for (int k = 0; k < kG; ++k) {
    if (k < A - 1) {
      cum += ex[k];
      if (pick == A - 1 && target < cum) pick = k;
    }
  }
  float lp = out[0];
#pragma unroll
  for (int k = 1; k < kG; ++k) lp = k == pick ? out[k] : lp;
  a.actions[i] = pick;
  a.log_probs[i] = lp - (mx + logf(se));
  a.values[i] = value;
}

__global__ __launch_bounds__(kThr) void gru_value_kernel(GruStepArgs a) {
  __shared__ __attribute__((aligned(16))) EnvLds lds[kEnvsPerWg];
  const int e = threadIdx.x >> 4, j = threadIdx.x & 15;
  const int64_t i = (int64_t)blockIdx.x * kEnvsPerWg + e;
  const bool valid = i < a.n;
  EnvLds& E = lds[e];
  gru_forward(a, E, valid ? i : a.n - 1, j);
  const float value = critic_value(a, E, j);
  if (valid && j == 0) a.values[i] = value;
}

int grid_for_envs(int64_t n, unsigned* grid) {
  const int64_t g = (n + kEnvsPerWg - 1) / kEnvsPerWg;
  if (g > 0x7FFFFFFF) {
    set_error("n = %lld is too large for one launch", (long long)n);
    return DPPO_EINVAL;
  }
  *grid = (unsigned)g;
  return DPPO_OK;
}

}  // namespace

int launch_gru_act(const GruOffsets& po, const float* params, const dppo_gru_step& st, int64_t n,
                   int D, int A, uint64_t seed, uint64_t counter, hipStream_t s) {
  unsigned grid = 0;
  const int rc = grid_for_envs(n, &grid);
  if (rc != DPPO_OK) return rc;
  GruStepArgs a{};
  a.po = po;
  a.params = params;
  a.obs = st.obs;
  a.dones = st.prev_dones;
  a.hx = st.hx;
  a.hx_out = st.hx_out;
  a.actions = st.actions;
  a.log_probs = st.log_probs;
  a.values = st.values;
  a.logits = st.logits;
  a.n = n;
  a.D = D;
  a.A = A;
  a.seed_lo = (uint32_t)seed;
  a.seed_hi = (uint32_t)(seed >> 32);
  a.ctr_lo = (uint32_t)counter;
  a.ctr_hi = (uint32_t)(counter >> 32);
  DPPO_LAUNCH(gru_act_kernel, dim3(grid), dim3(kThr), 0, s, a);
  DPPO_LAUNCH_CHECK();
  return DPPO_OK;
}

int launch_gru_value(const GruOffsets& po, const float* params, const float* obs, const float* hx,
                     const uint8_t* dones, int64_t n, int D, float* values, hipStream_t s) {
  unsigned grid = 0;
  const int rc = grid_for_envs(n, &grid);
  if (rc != DPPO_OK) return rc;
  GruStepArgs a{};
  a.po = po;
  a.params = params;
  a.obs = obs;
  a.dones = dones;
  a.hx = hx;
  a.values = values;
  a.n = n;
  a.D = D;
  DPPO_LAUNCH(gru_value_kernel, dim3(grid), dim3(kThr), 0, s, a);
  DPPO_LAUNCH_CHECK();
  return DPPO_OK;
}

}  // namespace dppo
