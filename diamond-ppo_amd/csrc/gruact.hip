// RecurrentPPO rollout step, fused (intended semantics of reference diamond/recurrent_ppo.py:214-245
// with the network of :94-149 and the hidden reset of :82-87; restated for T = 1 in
// oracle/gru_torch.py::sequence): what rollout() ran under torch as several dozen launches per env
// step is one launch for the policy step (gru_act_kernel: base, GRU cell, both heads, Categorical
// draw, log-prob) and one for V(next_obs) (gru_value_kernel: base, GRU cell, critic head).  Both
// kernels are templates on the GRU hidden width G, instantiated for 16, 32 and 64, and on the
// per-env observation capacity of their LDS: 32 floats, or 128 for the observations of 33 to 128
// floats that dppo_gru_dims.wide_obs admits (another 384 B per env, nothing else differs).
//
// Mapping: G lanes per env (lane j = hidden unit j, grugrad.hip's phase-B mapping), 4 envs per
// workgroup (4 G threads: one wave at G = 16, 2 at G = 32, 4 at G = 64); an env never straddles a
// wave.  Lane j computes base features j + G q and head features j + G q (q < 64 / G), the three
// gate rows j, and logit j (A <= 16 <= G); per-env vectors pass between the steps through LDS
// (768 / 832 / 960 B per env at G = 16 / 32 / 64).  The ~36 KB of parameters (G = 16) are read
// straight from global memory (L2-resident after the first workgroup; a row is read by all the
// envs of a workgroup at once): staging them in LDS would cost every workgroup a full 36 KB copy,
// which the 8 workgroups of num_envs = 32 could not amortise, and at n = 8192 the 2048 one-wave
// workgroups spread 8 waves over every CU without it.
//
// Every sum runs in a fixed order inside the env's own G lanes (the value's partials through
// row-local DPP, then at G >= 32 the 2 or 4 row sums by xor-16 / xor-32 lane exchanges, which
// stay inside the env's G lanes), so a sample's outputs are the same bits at any n, at any
// position in the batch and on any grid.  Lanes past n clamp to env n - 1 (valid addresses) and
// store nothing.  The Philox key, counter and per-env counter layout are the same at every width:
// the stream does not depend on G.
//
// gru_act_kernel<G, OBS, true> is the Gaussian policy step (RecurrentContinuousPPO): lane k < A
// computes mean k where it computed logit k, lane 0 draws with actdraw.h's draw_gaussian (the
// stream dppo_act_f32 documents) and takes the log-prob from the float32 action it stores, so a
// learn() at unchanged parameters recomputes a ratio of 1 to rounding.
#include "actdraw.h"
#include "grucell.h"
#include "philox.h"

namespace dppo {
namespace {

constexpr int kEnvsPerWg = 4;

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

// The Gaussian step's arguments: `actions` points at float [n][A], `logits` at the optional
// means, and log_std sits at ls_off of the flat layout.
struct GruGaussStepArgs : GruStepArgs {
  int64_t ls_off;
};

// What draw_gaussian reads (actdraw.h): no environment copy, no squash.
struct GaussDraw {
  int A;
  uint32_t seed_lo, seed_hi, ctr_lo, ctr_hi;
  float* env_act;
  int squash;
  const float *sq_lo, *sq_half, *sq_hi;
};

// per-env LDS vectors (floats); OBS = the observation capacity, 32 or (wide_obs) 128
template <int G, int OBS>
struct EnvLds {
  float obs[OBS];
  float x1[kH];
  float h[G];
  float ya[kH];
  float lg[kAPad];
};

__device__ __forceinline__ float dot4(f32x4 w, f32x4 x) {
  return (w[0] * x[0] + w[1] * x[1]) + (w[2] * x[2] + w[3] * x[3]);
}

template <int CTRL>
__device__ __forceinline__ float dpp_f32(float x) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, false));
}

// Sum over the G lanes of an env, the same bits in every lane: inside each 16-lane DPP row xor 1,
// xor 2, half-row mirror, row mirror; then the rows pairwise.
template <int G>
__device__ __forceinline__ float env_sum(float x) {
  x += dpp_f32<0xB1>(x);   // quad_perm [1,0,3,2]
  x += dpp_f32<0x4E>(x);   // quad_perm [2,3,0,1]
  x += dpp_f32<0x141>(x);  // row_half_mirror
  x += dpp_f32<0x140>(x);  // row_mirror
  if (G >= 32) x += __shfl_xor(x, 16);
  if (G == 64) x += __shfl_xor(x, 32);
  return x;
}

// tanh(W1 v + b1) for head features j + G q, q < 64 / G; W1 [64][G], v [G] in LDS
template <int G>
__device__ __forceinline__ void head_hidden(const float* __restrict__ W1,
                                            const float* __restrict__ b1, const float* v, int j,
                                            float (&y)[kH / G]) {
#pragma unroll
  for (int q = 0; q < kH / G; ++q) {
    const int o = j + G * q;
    const f32x4* w = (const f32x4*)(W1 + o * G);
    float z = b1[o];
#pragma unroll
    for (int k = 0; k < G / 4; ++k) z += dot4(w[k], ((const f32x4*)v)[k]);
    y[q] = tanh_acc(z);
  }
}

// Base layer, hidden reset and one GRU step for one env slot of the workgroup; on return E.h
// holds the new hidden state (all G lanes of the env see it) and the return value is lane j's own
// element.
template <int G, int OBS>
__device__ __forceinline__ float gru_forward(const GruStepArgs& a, EnvLds<G, OBS>& E, int64_t ic,
                                             int j) {
  constexpr int Q = kH / G;
  const float* P = a.params;
  const GruOffsets& po = a.po;
  const int D = a.D;
  for (int c = j; c < D; c += G) E.obs[c] = a.obs[ic * D + c];
  const bool reset = a.dones && a.dones[ic];
  const float h = reset ? 0.0f : a.hx[ic * G + j];  // hx[:, dones] = 0 (recurrent_ppo.py:84)
  E.h[j] = h;
  __syncthreads();
  // x1 = tanh(Wb obs + bb), features j + G q
  {
    float z[Q];
    const float* w[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      z[q] = P[po.bb + j + G * q];
      w[q] = P + po.Wb + (int64_t)(j + G * q) * D;
    }
#pragma unroll 4
    for (int c = 0; c < D; ++c) {
      const float o = E.obs[c];
#pragma unroll
      for (int q = 0; q < Q; ++q) z[q] += w[q][c] * o;
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) E.x1[j + G * q] = tanh_acc(z[q]);
  }
  __syncthreads();
  // gates: gi = Wih x1 + bih, gh = Whh h + bhh, rows j (r), G + j (z), 2G + j (n)
  float gi[3], gh[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    const int row = g * G + j;
    const f32x4* wi = (const f32x4*)(P + po.Wih + row * kH);
    const f32x4* wh = (const f32x4*)(P + po.Whh + row * G);
    float si = P[po.bih + row], sh = P[po.bhh + row];
#pragma unroll
    for (int k = 0; k < kH / 4; ++k) si += dot4(wi[k], ((const f32x4*)E.x1)[k]);
#pragma unroll
    for (int k = 0; k < G / 4; ++k) sh += dot4(wh[k], ((const f32x4*)E.h)[k]);
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

// critic head on E.h: Linear(G, 64) tanh Linear(64, 1)
template <int G, int OBS>
__device__ __forceinline__ float critic_value(const GruStepArgs& a, const EnvLds<G, OBS>& E,
                                              int j) {
  const float* P = a.params;
  float yc[kH / G];
  head_hidden<G>(P + a.po.Wc1, P + a.po.bc1, E.h, j, yc);
  float part = 0.0f;
#pragma unroll
  for (int q = 0; q < kH / G; ++q) part += P[a.po.Wc2 + j + G * q] * yc[q];
  return P[a.po.bc2] + env_sum<G>(part);
}

template <int G, int OBS = 32, bool GAUSS = false>
__global__ __launch_bounds__(kEnvsPerWg* G) void gru_act_kernel(
    std::conditional_t<GAUSS, GruGaussStepArgs, GruStepArgs> a) {
  __shared__ __attribute__((aligned(16))) EnvLds<G, OBS> lds[kEnvsPerWg];
  const int e = threadIdx.x / G, j = threadIdx.x % G;
  const int64_t i = (int64_t)blockIdx.x * kEnvsPerWg + e;
  const bool valid = i < a.n;
  const int64_t ic = valid ? i : a.n - 1;
  EnvLds<G, OBS>& E = lds[e];
  const float* P = a.params;
  const int A = a.A;

  const float hn = gru_forward<G, OBS>(a, E, ic, j);
  if (valid) a.hx_out[i * G + j] = hn;
  const float value = critic_value<G, OBS>(a, E, j);

  // actor head: Linear(G, 64) tanh Linear(64, A); lane k < A computes logit k
  float ya[kH / G];
  head_hidden<G>(P + a.po.Wa1, P + a.po.ba1, E.h, j, ya);
#pragma unroll
  for (int q = 0; q < kH / G; ++q) E.ya[j + G * q] = ya[q];
  __syncthreads();
  if (j < kAPad) {
    const int k = j < A ? j : A - 1;
    const f32x4* w = (const f32x4*)(P + a.po.Wa2 + k * kH);
    float lg = P[a.po.ba2 + k];
#pragma unroll
    for (int q = 0; q < kH / 4; ++q) lg += dot4(w[q], ((const f32x4*)E.ya)[q]);
    E.lg[j] = lg;
    if (valid && a.logits && j < A) a.logits[i * A + j] = lg;
  }
  __syncthreads();
  if constexpr (GAUSS) {
    // log_std for the workgroup, zeros past A (draw_gaussian reads kAPad of them)
    __shared__ float ls_s[kAPad];
    if (threadIdx.x < kAPad) ls_s[threadIdx.x] = (int)threadIdx.x < A ? P[a.ls_off + threadIdx.x] : 0.0f;
    __syncthreads();
    if (!valid || j != 0) return;
    float mean[kAPad], u[kAPad];
#pragma unroll
    for (int q = 0; q < kAPad / 4; ++q) {
      const f32x4 x = ((const f32x4*)E.lg)[q];
      mean[4 * q] = x[0];
      mean[4 * q + 1] = x[1];
      mean[4 * q + 2] = x[2];
      mean[4 * q + 3] = x[3];
    }
#pragma unroll
    for (int k = 0; k < kAPad; ++k) u[k] = 0.0f;
    const GaussDraw dr{A, a.seed_lo, a.seed_hi, a.ctr_lo, a.ctr_hi, nullptr, 0, nullptr, nullptr,
                       nullptr};
    draw_gaussian<kAPad>(dr, mean, ls_s, i, u);
    // log N(u; mean, exp(log_std)) summed over the action dims (continuous_ppo.py:41-43), from
    // the float32 action as stored; accurate expf
    float lp = 0.0f;
    float* act = (float*)(void*)a.actions + i * A;
#pragma unroll
    for (int k = 0; k < kAPad; ++k) {
      if (k < A) {
        const float ls = ls_s[k];
        const float z = (u[k] - mean[k]) * expf(-ls);
        lp += -0.5f * z * z - ls - 0.91893853320467274178f;
        act[k] = u[k];
      }
    }
    a.log_probs[i] = lp;
    a.values[i] = value;
    return;
  }
  if (!valid || j != 0) return;

  // Categorical(logits).sample() by inverse CDF on one uniform (as mlp.hip act_kernel), and the
  // log-prob of the draw with accurate expf / logf
  float out[kAPad];
#pragma unroll
  for (int q = 0; q < kAPad / 4; ++q) {
    const f32x4 x = ((const f32x4*)E.lg)[q];
    out[4 * q] = x[0];
    out[4 * q + 1] = x[1];
    out[4 * q + 2] = x[2];
    out[4 * q + 3] = x[3];
  }
  float mx = out[0];
#pragma unroll
  for (int k = 1; k < kAPad; ++k)
    if (k < A) mx = fmaxf(mx, out[k]);
  float ex[kAPad], se = 0.0f;
#pragma unroll
  for (int k = 0; k < kAPad; ++k) {
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
  for (int k = 0; k < kAPad; ++k) {
    if (k < A - 1) {
      cum += ex[k];
      if (pick == A - 1 && target < cum) pick = k;
    }
  }
  float lp = out[0];
#pragma unroll
  for (int k = 1; k < kAPad; ++k) lp = k == pick ? out[k] : lp;
  a.actions[i] = pick;
  a.log_probs[i] = lp - (mx + logf(se));
  a.values[i] = value;
}

template <int G, int OBS = 32>
__global__ __launch_bounds__(kEnvsPerWg* G) void gru_value_kernel(GruStepArgs a) {
  __shared__ __attribute__((aligned(16))) EnvLds<G, OBS> lds[kEnvsPerWg];
  const int e = threadIdx.x / G, j = threadIdx.x % G;
  const int64_t i = (int64_t)blockIdx.x * kEnvsPerWg + e;
  const bool valid = i < a.n;
  EnvLds<G, OBS>& E = lds[e];
  gru_forward<G, OBS>(a, E, valid ? i : a.n - 1, j);
  const float value = critic_value<G, OBS>(a, E, j);
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

constexpr int kWideObs = 128;  // observation capacity of the wide_obs instantiations

template <int G>
void launch_width_gauss(unsigned grid, const GruGaussStepArgs& a, hipStream_t s) {
  const dim3 block(kEnvsPerWg * G);
  if (a.D > 32)
    DPPO_LAUNCH((gru_act_kernel<G, kWideObs, true>), dim3(grid), block, 0, s, a);
  else
    DPPO_LAUNCH((gru_act_kernel<G, 32, true>), dim3(grid), block, 0, s, a);
}

template <int G>
void launch_width(bool act, unsigned grid, const GruStepArgs& a, hipStream_t s) {
  const dim3 block(kEnvsPerWg * G);
  if (a.D > 32) {
    if (act)
      DPPO_LAUNCH((gru_act_kernel<G, kWideObs>), dim3(grid), block, 0, s, a);
    else
      DPPO_LAUNCH((gru_value_kernel<G, kWideObs>), dim3(grid), block, 0, s, a);
  } else if (act) {
    DPPO_LAUNCH(gru_act_kernel<G>, dim3(grid), block, 0, s, a);
  } else {
    DPPO_LAUNCH(gru_value_kernel<G>, dim3(grid), block, 0, s, a);
  }
}

// The one fill of the kernel arguments and the one dispatch on G: the policy step (act) or the
// value step, which reads st.obs / prev_dones / hx and writes st.values alone.
int launch_step(int G, bool act, const GruOffsets& po, const float* params,
                const dppo_gru_step& st, int64_t n, int D, int A, uint64_t seed, uint64_t counter,
                hipStream_t s) {
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
  if (!dispatch_gru_width(G, [&](auto g) { launch_width<decltype(g)::value>(act, grid, a, s); })) {
    set_error("no wide GRU rollout kernel for gru_hidden=%d", G);
    return DPPO_EUNSUPPORTED;
  }
  DPPO_LAUNCH_CHECK();
  return DPPO_OK;
}

}  // namespace

int gru_act_envs() { return kEnvsPerWg; }

int launch_gru_act(int G, const GruOffsets& po, const float* params, const dppo_gru_step& st,
                   int64_t n, int D, int A, uint64_t seed, uint64_t counter, hipStream_t s) {
  return launch_step(G, true, po, params, st, n, D, A, seed, counter, s);
}

int launch_gru_gauss_act(int G, const GruOffsets& po, int64_t ls_off, const float* params,
                         const dppo_gru_gauss_step& st, int64_t n, int D, int A, uint64_t seed,
                         uint64_t counter, hipStream_t s) {
  unsigned grid = 0;
  const int rc = grid_for_envs(n, &grid);
  if (rc != DPPO_OK) return rc;
  GruGaussStepArgs a{};
  a.po = po;
  a.params = params;
  a.obs = st.obs;
  a.dones = st.prev_dones;
  a.hx = st.hx;
  a.hx_out = st.hx_out;
  a.actions = (int32_t*)(void*)st.actions;  // float [n][A] in the Gaussian kernel
  a.log_probs = st.log_probs;
  a.values = st.values;
  a.logits = st.means;
  a.n = n;
  a.D = D;
  a.A = A;
  a.seed_lo = (uint32_t)seed;
  a.seed_hi = (uint32_t)(seed >> 32);
  a.ctr_lo = (uint32_t)counter;
  a.ctr_hi = (uint32_t)(counter >> 32);
  a.ls_off = ls_off;
  if (!dispatch_gru_width(G, [&](auto g) { launch_width_gauss<decltype(g)::value>(grid, a, s); })) {
    set_error("no GRU rollout kernel for gru_hidden=%d", G);
    return DPPO_EUNSUPPORTED;
  }
  DPPO_LAUNCH_CHECK();
  return DPPO_OK;
}

int launch_gru_value(int G, const GruOffsets& po, const float* params, const float* obs,
                     const float* hx, const uint8_t* dones, int64_t n, int D, float* values,
                     hipStream_t s) {
  dppo_gru_step st{};
  st.obs = obs;
  st.prev_dones = dones;
  st.hx = hx;
  st.values = values;
  return launch_step(G, false, po, params, st, n, D, 0, 0, 0, s);
}

}  // namespace dppo
