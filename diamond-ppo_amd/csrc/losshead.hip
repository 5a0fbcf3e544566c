// PPO loss head on gfx950: clipped surrogate + value + entropy loss of one minibatch, forward and
// the closed-form backward in one pass over the network's outputs.
//
// Replaces, for a network that runs under torch autograd (custom network_cls, shapes outside the
// fused classes), the eager op chain of the reference's minibatch loss (ppo.py:264-280:
// Categorical(logits), log_prob, ratio, clamp, max, mse_loss, entropy, three means;
// continuous_ppo.py:276-292 with JointNormal, continuous_ppo.py:39-47) together with the four
// index gathers in front of it and autograd's backward of all of them; and, forward only, the
// old-policy log-probabilities (ppo.py:235-237, continuous_ppo.py:247-249).
//
// Layout.  A sample's row of A logits (or Gaussian means) sits on a group of G lanes, G a power
// of two <= 64; every lane holds kSlots = 4 elements of it in registers:
//   * scalar form: G >= min(A, 64), slot j of lane l is column l + j*G (consecutive lanes read
//     consecutive floats; rows wider than 64 take the further slots: the in-group loop);
//   * 16-byte form (A % 4 == 0 and every [.][A] array 16-byte aligned, checked on the host):
//     G >= A/4, slot j of lane l is column 4l + j, one dwordx4 load and store per array.
// So A <= 4 * 64 = kLossMaxA = 256, and each row is read once and its gradient written once.  Row
// maxima and sums are butterflies over the group's lanes (ds_bpermute); the per-sample scalars
// (action, old log-prob, advantage, return) are gathered through idx.  The grid is capped at
// kMaxGrid blocks and grid-strided; each block leaves the partials of the sums {policy, value,
// entropy, clip count} in the caller's workspace and a one-block second launch adds them
// in a fixed order, in double: no floating-point atomics, the same bits on every call.
//
// The log-probability is ONE function (row_logp, contraction off) for both kernels, so the old
// and the new log-probability of an unchanged network are the same bits and ratio == 1.0f.
#include "common.h"

#include <cmath>

namespace dppo {
namespace {

constexpr int kSlots = 4;
constexpr int kLossMaxA = kSlots * kWave;  // 256
constexpr int kLossThreads = 256;
constexpr int kLossWaves = kLossThreads / kWave;
constexpr int kMaxGrid = 1024;
constexpr int kPartStride = 8;  // floats per block in the workspace (4 used)
constexpr int kSums = 4;     // policy, value, entropy, clip count

struct LossGeom {
  int A;
  int G;          // lanes per row
  int log_std_stride;
  int64_t m;
  int64_t B;      // length of the rollout-flat arrays idx points into
};

struct LossScalars {
  float lo, hi;   // 1 - eps, 1 + eps as torch.clamp receives them
  float vf, beta;
  float w;        // scale / m
  float scale;
  float inv_m;
};

__device__ __forceinline__ float group_sum(float v, int G) {
  for (int off = G >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ float group_max(float v, int G) {
  for (int off = G >> 1; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}

template <bool VEC>
__device__ __forceinline__ int slot_col(int lig, int G, int j) {
  return VEC ? 4 * lig + j : lig + j * G;
}

// One row's kSlots elements of this lane; `row` may be null (lane without a sample): fill.
template <bool VEC>
__device__ __forceinline__ void load_row(const float* __restrict__ row, int A, int lig, int G,
                                         float fill, float (&x)[kSlots]) {
  if (VEC) {
    if (row && 4 * lig < A) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(row + 4 * lig);
#pragma unroll
      for (int j = 0; j < kSlots; ++j) x[j] = v[j];
    } else {
#pragma unroll
      for (int j = 0; j < kSlots; ++j) x[j] = fill;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
      const int c = lig + j * G;
      x[j] = (row && c < A) ? row[c] : fill;
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void store_row(float* __restrict__ row, int A, int lig, int G,
                                          const float (&x)[kSlots]) {
  if (VEC) {
    if (4 * lig < A) {
      f32x4 v;
#pragma unroll
      for (int j = 0; j < kSlots; ++j) v[j] = x[j];
      *reinterpret_cast<f32x4*>(row + 4 * lig) = v;
    }
  } else {
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
      const int c = lig + j * G;
      if (c < A) row[c] = x[j];
    }
  }
}

// What the backward needs of a row beside its log-probability.
struct RowStats {
  float lse;   // categorical: log sum exp
  float rse;   // categorical: 1 / sum exp(x - max)
  float mx;    // categorical: row maximum
};

constexpr float kHalfLog2Pi = 0.91893853320467274178f;

// log pi(a | row): categorical log-softmax with the row maximum subtracted, gathered at `act`
// (torch Categorical.log_prob), or the JointNormal log-density summed over the action dims
// (x = means, ls = log-std, av = the action).  Every lane of the group returns the same value.
template <bool CONT, bool VEC>
__device__ __forceinline__ float row_logp(const float (&x)[kSlots], const float (&ls)[kSlots],
                                          const float (&av)[kSlots], int act, int A, int lig,
                                          int G, RowStats& st) {
#pragma clang fp contract(off)
  if (CONT) {
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
      if (slot_col<VEC>(lig, G, j) < A) {
        const float z = (av[j] - x[j]) * expf(-ls[j]);
        s += (-0.5f * (z * z) - ls[j]) - kHalfLog2Pi;
      }
    }
    st.lse = st.rse = st.mx = 0.0f;
    return group_sum(s, G);
  } else {
    float mx = x[0];  // slots past A hold -inf
#pragma unroll
    for (int j = 1; j < kSlots; ++j) mx = fmaxf(mx, x[j]);
    mx = group_max(mx, G);
    float se = 0.0f, xa = 0.0f;
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
      const int c = slot_col<VEC>(lig, G, j);
      if (c < A) {
        se += expf(x[j] - mx);
        if (c == act) xa = x[j];
      }
    }
    se = group_sum(se, G);
    xa = group_sum(xa, G);
    st.mx = mx;
    st.lse = mx + logf(se);
    st.rse = 1.0f / se;
    return xa - st.lse;
  }
}

// The row pointers and gathered index of this lane's sample.
struct Sample {
  int64_t s;    // minibatch position, < m
  int64_t i;    // rollout-flat index
  bool ok;      // s < m and 0 <= i < B
};

__device__ __forceinline__ Sample pick(int64_t s, const LossGeom& g,
                                       const int64_t* __restrict__ idx) {
  Sample p;
  p.s = s;
  p.i = 0;
  p.ok = s < g.m;
  if (p.ok) {
    p.i = idx ? idx[s] : s;
    // an index outside the rollout is never dereferenced: the sample's result is NaN
    if (p.i < 0 || p.i >= g.B) p.ok = false;
  }
  return p;
}

template <bool CONT, bool VEC>
__device__ __forceinline__ float sample_logp(const Sample& p, const LossGeom& g, int lig,
                                             const float* __restrict__ logits,
                                             const float* __restrict__ log_std,
                                             const void* __restrict__ actions,
                                             float (&x)[kSlots], float (&ls)[kSlots],
                                             float (&av)[kSlots], int& act, RowStats& st) {
  const float* row = p.ok ? logits + p.s * g.A : nullptr;
  load_row<VEC>(row, g.A, lig, g.G, CONT ? 0.0f : -INFINITY, x);
  act = -1;
  if (CONT) {
    load_row<VEC>(p.ok ? log_std + p.s * g.log_std_stride : nullptr, g.A, lig, g.G, 0.0f, ls);
    load_row<VEC>(p.ok ? (const float*)actions + p.i * g.A : nullptr, g.A, lig, g.G, 0.0f, av);
  } else {
#pragma unroll
    for (int j = 0; j < kSlots; ++j) ls[j] = av[j] = 0.0f;
    if (p.ok) act = ((const int32_t*)actions)[p.i];
  }
  return row_logp<CONT, VEC>(x, ls, av, act, g.A, lig, g.G, st);
}

template <bool CONT, bool VEC>
__global__ __launch_bounds__(kLossThreads) void policy_logp_kernel(
    LossGeom g, const float* __restrict__ logits, const float* __restrict__ log_std,
    const int64_t* __restrict__ idx, const void* __restrict__ actions, float* __restrict__ logp) {
  const int lig = threadIdx.x & (g.G - 1);
  const int64_t per_pass = (int64_t)gridDim.x * (kLossThreads / g.G);
  const int64_t first = ((int64_t)blockIdx.x * kLossThreads + threadIdx.x) / g.G;
  // the trip count is the same for every lane: the group butterflies need whole waves
  for (int64_t base = 0; base < g.m; base += per_pass) {
    const int64_t s = base + first;
    const Sample p = pick(s, g, idx);
    float x[kSlots], ls[kSlots], av[kSlots];
    int act;
    RowStats st;
    const float lp = sample_logp<CONT, VEC>(p, g, lig, logits, log_std, actions, x, ls, av, act, st);
    if (lig == 0 && s < g.m) logp[s] = p.ok ? lp : NAN;
  }
}

template <bool CONT, bool VEC>
__global__ __launch_bounds__(kLossThreads) void ppo_loss_kernel(
    LossGeom g, LossScalars c, const float* __restrict__ logits, const float* __restrict__ log_std,
    const float* __restrict__ values, const int64_t* __restrict__ idx,
    const void* __restrict__ actions, const float* __restrict__ old_logp,
    const float* __restrict__ adv, const float* __restrict__ ret, float* __restrict__ d_logits,
    float* __restrict__ d_log_std, float* __restrict__ d_values, float* __restrict__ partials) {
  __shared__ double part[kLossWaves][kSums];
  const int lig = threadIdx.x & (g.G - 1);
  const int64_t per_pass = (int64_t)gridDim.x * (kLossThreads / g.G);
  const int64_t first = ((int64_t)blockIdx.x * kLossThreads + threadIdx.x) / g.G;
  double acc[kSums] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t base = 0; base < g.m; base += per_pass) {
    const int64_t s = base + first;
    const Sample p = pick(s, g, idx);
    float x[kSlots], ls[kSlots], av[kSlots];
    int act;
    RowStats st;
    const float lp = sample_logp<CONT, VEC>(p, g, lig, logits, log_std, actions, x, ls, av, act, st);
    float a = 0.0f, old = 0.0f, R = 0.0f, v = 0.0f;
    if (p.ok) {
      a = adv[p.i];
      old = old_logp[p.i];
      R = ret[p.i];
      v = values[p.s];
    }
    // ratio, clipped surrogate and its derivative with torch's conventions: maximum halves the
    // gradient at a tie, clamp passes it on the closed interval [lo, hi]
    const float r = expf(lp - old);
    const float rc = fminf(fmaxf(r, c.lo), c.hi);
    const float t1 = -a * r, t2 = -a * rc;
    const float l_pi = fmaxf(t1, t2);
    const float g1 = t1 > t2 ? 1.0f : (t1 == t2 ? 0.5f : 0.0f);
    const float pass = (r >= c.lo && r <= c.hi) ? 1.0f : 0.0f;
    const float dlp = (g1 * -a + (1.0f - g1) * pass * -a) * r;  // d l_pi / d logp
    const float dv = v - R;
    float H;
    float dx[kSlots], dls[kSlots];
    if (CONT) {
      float h = 0.0f;
#pragma unroll
      for (int j = 0; j < kSlots; ++j) {
        dx[j] = dls[j] = 0.0f;
        if (slot_col<VEC>(lig, g.G, j) < g.A) {
          h += (0.5f + kHalfLog2Pi) + ls[j];
          const float is = expf(-ls[j]);
          const float z = (av[j] - x[j]) * is;
          dx[j] = c.w * (dlp * (z * is));
          // d(-beta H)/d log_std = -beta for every sample and dim
          dls[j] = c.w * (dlp * (z * z - 1.0f) - c.beta);
        }
      }
      H = group_sum(h, g.G);
    } else {
      float pl[kSlots], lpk[kSlots];
      float h = 0.0f;
#pragma unroll
      for (int j = 0; j < kSlots; ++j) {
        pl[j] = lpk[j] = 0.0f;
        if (slot_col<VEC>(lig, g.G, j) < g.A) {
          lpk[j] = x[j] - st.lse;
          pl[j] = expf(x[j] - st.mx) * st.rse;
          // torch clamps log p at the smallest float before p * log p, so p == 0 gives 0
          h -= pl[j] == 0.0f ? 0.0f : pl[j] * lpk[j];
        }
      }
      H = group_sum(h, g.G);
#pragma unroll
      for (int j = 0; j < kSlots; ++j) {
        const int col = slot_col<VEC>(lig, g.G, j);
        const float onehot = col == act ? 1.0f : 0.0f;
        const float dent = pl[j] == 0.0f ? 0.0f : pl[j] * (lpk[j] + H);
        dx[j] = c.w * (dlp * (onehot - pl[j]) + c.beta * dent);
      }
    }
    if (s < g.m) {
      if (!p.ok) {  // index outside the rollout: poison this sample's outputs
#pragma unroll
        for (int j = 0; j < kSlots; ++j) dx[j] = dls[j] = NAN;
      }
      store_row<VEC>(d_logits + s * g.A, g.A, lig, g.G, dx);
      if (CONT) store_row<VEC>(d_log_std + s * g.A, g.A, lig, g.G, dls);
      if (lig == 0) {
        d_values[s] = p.ok ? c.w * c.vf * dv : NAN;
        acc[0] += p.ok ? (double)l_pi : (double)NAN;
        acc[1] += 0.5 * (double)dv * (double)dv;
        acc[2] += (double)H;
        acc[3] += (r < c.lo || r > c.hi) ? 1.0 : 0.0;
      }
    }
  }
  // block partials in a fixed order: wave butterfly, then the waves in order
#pragma unroll
  for (int k = 0; k < kSums; ++k)
    for (int off = 32; off >= 1; off >>= 1) acc[k] += __shfl_xor(acc[k], off);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kSums; ++k) part[wave][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < kSums) {
    double t = 0.0;
    for (int w = 0; w < kLossWaves; ++w) t += part[w][threadIdx.x];
    partials[(int64_t)blockIdx.x * kPartStride + threadIdx.x] = (float)t;
  }
}

// One block, one thread per block partial (blocks <= kMaxGrid = 1024 threads, so every partial is
// in flight in one memory round trip): out[8] = {loss, policy, value, entropy, clip fraction, 0,
// 0, 0}.  Fixed order: wave butterfly, then the waves in order, in double.
__global__ __launch_bounds__(kMaxGrid) void ppo_loss_finish_kernel(
    const float* __restrict__ partials, int blocks, LossScalars c, float* __restrict__ out) {
  __shared__ double part[kMaxGrid / kWave][kSums];
  double t[kSums];
#pragma unroll
  for (int k = 0; k < kSums; ++k)
    t[k] = (int)threadIdx.x < blocks
               ? (double)partials[(int64_t)threadIdx.x * kPartStride + k] : 0.0;
#pragma unroll
  for (int k = 0; k < kSums; ++k)
    for (int off = 32; off >= 1; off >>= 1) t[k] += __shfl_xor(t[k], off);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kSums; ++k) part[wave][k] = t[k];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int waves = (int)(blockDim.x >> 6);
    double u[kSums] = {0.0, 0.0, 0.0, 0.0};
    for (int w = 0; w < waves; ++w) {
#pragma unroll
      for (int k = 0; k < kSums; ++k) u[k] += part[w][k];
    }
    const double inv = (double)c.inv_m;
    const double lpi = u[0] * inv, lv = u[1] * inv, ent = u[2] * inv;
    out[0] = (float)((double)c.scale * (lpi + (double)c.vf * lv - (double)c.beta * ent));
    out[1] = (float)lpi;
    out[2] = (float)lv;
    out[3] = (float)ent;
    out[4] = (float)(u[3] * inv);
    out[5] = out[6] = out[7] = 0.0f;
  }
}

int pow2_at_least(int n) {
  int g = 1;
  while (g < n) g <<= 1;
  return g;
}

// lanes per row and blocks for m rows of A in the scalar or the 16-byte form
void loss_geometry(int64_t m, int A, bool vec, int* G, int* grid) {
  int need = vec ? A / 4 : A;
  if (need > kWave) need = kWave;
  *G = pow2_at_least(need);
  const int64_t per_block = kLossThreads / *G;
  int64_t blocks = (m + per_block - 1) / per_block;
  if (blocks > kMaxGrid) blocks = kMaxGrid;
  if (blocks < 1) blocks = 1;
  *grid = (int)blocks;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

int loss_plan(int64_t m, int A, int64_t* workspace_floats, int* grid) {
  // the form is chosen from the pointers' alignment at launch: size for the larger grid
  int Gs, gs, Gv = 0, gv = 0;
  loss_geometry(m, A, false, &Gs, &gs);
  if (A % 4 == 0) loss_geometry(m, A, true, &Gv, &gv);
  *grid = gs;  // the scalar form's: rows of 256 / pow2(min(A, 64)) samples per block
  *workspace_floats = (int64_t)(gs > gv ? gs : gv) * kPartStride;
  return DPPO_OK;
}

int launch_policy_logp(const float* logits, const float* log_std, int log_std_stride,
                       const int64_t* idx, const void* actions, int64_t m, int64_t B, int A,
                       bool continuous, float* logp, hipStream_t s) {
  const bool vec = A % 4 == 0 && aligned16(logits) &&
                   (!continuous || (aligned16(log_std) && aligned16(actions)));
  LossGeom g{};
  int grid;
  loss_geometry(m, A, vec, &g.G, &grid);
  g.A = A;
  g.log_std_stride = log_std_stride;
  g.m = m;
  g.B = B;
#define DPPO_LOGP(C, V)                                                                          \
  DPPO_LAUNCH((policy_logp_kernel<C, V>), dim3((unsigned)grid), dim3(kLossThreads), 0, s, g,     \
              logits, log_std, idx, actions, logp)
  if (continuous) {
    if (vec) DPPO_LOGP(true, true); else DPPO_LOGP(true, false);
  } else {
    if (vec) DPPO_LOGP(false, true); else DPPO_LOGP(false, false);
  }
#undef DPPO_LOGP
  DPPO_LAUNCH_CHECK();
  return DPPO_OK;
}

int launch_ppo_loss(const dppo_loss_args& a, hipStream_t s) {
  const bool cont = a.continuous != 0;
  const bool vec = a.act_dim % 4 == 0 && aligned16(a.logits) && aligned16(a.d_logits) &&
                   (!cont || (aligned16(a.log_std) && aligned16(a.actions) &&
                              aligned16(a.d_log_std)));
  LossGeom g{};
  int grid;
  loss_geometry(a.m, a.act_dim, vec, &g.G, &grid);
  g.A = a.act_dim;
  g.log_std_stride = a.log_std_stride;
  g.m = a.m;
  g.B = a.rollout_len;
  LossScalars c{};
  // torch.clamp(ratio, 1.0 - clip, 1.0 + clip): Python doubles, rounded to the tensor's float
  c.lo = (float)(1.0 - a.ppo_clip);
  c.hi = (float)(1.0 + a.ppo_clip);
  c.vf = a.value_loss_weight;
  c.beta = a.entropy_beta;
  c.scale = a.scale;
  c.inv_m = (float)(1.0 / (double)a.m);
  c.w = (float)((double)a.scale / (double)a.m);
#define DPPO_LOSS(C, V)                                                                          \
  DPPO_LAUNCH((ppo_loss_kernel<C, V>), dim3((unsigned)grid), dim3(kLossThreads), 0, s, g, c,     \
              a.logits, a.log_std, a.values, a.idx, a.actions, a.old_log_probs, a.advantages,    \
              a.returns, a.d_logits, a.d_log_std, a.d_values, a.workspace)
  if (cont) {
    if (vec) DPPO_LOSS(true, true); else DPPO_LOSS(true, false);
  } else {
    if (vec) DPPO_LOSS(false, true); else DPPO_LOSS(false, false);
  }
#undef DPPO_LOSS
  DPPO_LAUNCH_CHECK();
  DPPO_LAUNCH(ppo_loss_finish_kernel, dim3(1), dim3((unsigned)((grid + kWave - 1) / kWave * kWave)), 0,
              s, a.workspace, grid, c, a.out);
  DPPO_LAUNCH_CHECK();
  return DPPO_OK;
}

bool bad_shape(const char* fn, int64_t m, int A, int cont, int ls_stride) {
  if (m < 1) {
    set_error("%s: m = %lld, need at least one sample", fn, (long long)m);
    return true;
  }
  if (A < 1 || A > kLossMaxA) {
    set_error("%s: act_dim %d outside 1..%d", fn, A, kLossMaxA);
    return true;
  }
  if (cont && ls_stride != 0 && ls_stride != A) {
    set_error("%s: log_std_stride %d, must be 0 (one broadcast row) or act_dim %d", fn, ls_stride,
              A);
    return true;
  }
  return false;
}

}  // namespace
}  // namespace dppo

using namespace dppo;

extern "C" {

int dppo_ppo_loss_plan(int64_t m, int32_t act_dim, int32_t continuous, int64_t* workspace_floats,
                       int32_t* grid, int32_t* max_A) {
  (void)continuous;
  if (max_A) *max_A = kLossMaxA;
  if (bad_shape("dppo_ppo_loss_plan", m, act_dim, 0, 0)) return DPPO_EINVAL;
  int64_t ws;
  int g;
  loss_plan(m, act_dim, &ws, &g);
  if (workspace_floats) *workspace_floats = ws;
  if (grid) *grid = g;
  return DPPO_OK;
}

int dppo_ppo_loss_f32(const dppo_loss_args* a, void* stream) {
  if (!a) {
    set_error("dppo_ppo_loss_f32: args is NULL");
    return DPPO_EINVAL;
  }
  if (!a->logits || !a->values || !a->actions || !a->old_log_probs || !a->advantages ||
      !a->returns || !a->d_logits || !a->d_values || !a->out || !a->workspace ||
      (a->continuous && (!a->log_std || !a->d_log_std))) {
    set_error("dppo_ppo_loss_f32: a required pointer is NULL");
    return DPPO_EINVAL;
  }
  if (bad_shape("dppo_ppo_loss_f32", a->m, a->act_dim, a->continuous, a->log_std_stride))
    return DPPO_EINVAL;
  if (a->rollout_len < 1) {
    set_error("dppo_ppo_loss_f32: rollout_len = %lld", (long long)a->rollout_len);
    return DPPO_EINVAL;
  }
  int64_t ws;
  int g;
  loss_plan(a->m, a->act_dim, &ws, &g);
  if (a->workspace_floats < ws) {
    set_error("dppo_ppo_loss_f32: workspace of %lld floats, the plan needs %lld",
              (long long)a->workspace_floats, (long long)ws);
    return DPPO_EINVAL;
  }
  return launch_ppo_loss(*a, static_cast<hipStream_t>(stream));
}

int dppo_policy_logp_f32(const float* logits, const float* log_std, int32_t log_std_stride,
                         const int64_t* idx, const void* actions, int64_t m, int64_t rollout_len,
                         int32_t act_dim, int32_t continuous, float* logp, void* stream) {
  if (!logits || !actions || !logp || (continuous && !log_std)) {
    set_error("dppo_policy_logp_f32: a required pointer is NULL");
    return DPPO_EINVAL;
  }
  if (bad_shape("dppo_policy_logp_f32", m, act_dim, continuous, log_std_stride)) return DPPO_EINVAL;
  if (rollout_len < 1) {
    set_error("dppo_policy_logp_f32: rollout_len = %lld", (long long)rollout_len);
    return DPPO_EINVAL;
  }
  return launch_policy_logp(logits, log_std, log_std_stride, idx, actions, m, rollout_len, act_dim,
                            continuous != 0, logp, static_cast<hipStream_t>(stream));
}

}  // extern "C"
