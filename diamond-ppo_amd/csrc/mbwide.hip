// Wide kernel family: the fused PPO minibatch step, the old-policy evaluation and the rollout's
// action sampling of the default actor-critic MLP at hidden 128 (1 <= D <= 128) and at hidden 64 with 33 <= D <= 128, where the
// tuned kernels (mbwave.hip / mbstep.hip / mlp.hip: hidden 64, D <= 32) do not apply.  Hidden 64
// goes on to "large heads" (dispatch.cpp wide_large_shape): D <= 384 and A <= 32, the second
// block of 16 actions a compile-time choice (AB below) so that the A <= 16 kernels keep their code.
//
// Reference: loss and backward of one minibatch, diamond/ppo.py:261-283 (continuous:
// continuous_ppo.py:273-295), default networks ppo.py:53-71 / continuous_ppo.py:63-81.
//
// ---- Decomposition ----------------------------------------------------------------------------
// A workgroup = H/16 waves (8 at H = 128, 4 at H = 64), one workgroup per CU.  The minibatch is
// cut into tiles of S = 32 samples; workgroup b runs tiles b, b + G, ... and writes ONE gradient
// slab at the end.  Wave q owns output features [16q, 16q+16) of every hidden layer:
//   * forward  Y[16q.., s]  = W[16q.., :] X[:, s]       A = 16 rows of W, 16-B loads from L2/L1,
//   * backward dX[16q.., s] = W[:, 16q..]^T dZ[:, s]    A = 16 columns of W, 4-B loads,
//   * dW[16q.., :] += dZ[16q.., s] X[:, s]^T            accumulators in registers for the whole
//     launch: 16 rows x (3 H + 128) columns = 128 registers per lane at H = 128,
// all with v_mfma_f32_16x16x4_f32 (exact fp32).  At H = 128 the three hidden matrices are 192 KB:
// they do not fit the LDS beside the activations, so the A operands are read from global memory
// (every CU reads the same ~270 KB: L2 hits) and each is used for both 16-sample halves of a tile.
// Activations and deltas pass between the waves through LDS images [S][H + 4] with workgroup
// barriers between the layers (ten per tile); deltas overwrite the activation they belong to once
// every wave has read it.  The K order of the forward and backward products is permuted so that a
// lane's four consecutive k-steps are 16 contiguous bytes of the B image (one ds_read_b128).
// Heads (logits / Gaussian mean, value), the per-sample loss and the head back-propagation run on
// VALU, H/8 lanes per sample and 8 hidden features per lane; the head weight gradient dWo is an
// MFMA product over the sample axis (wave q: columns [16q, 16q+16)).
//
// Every sum has a fixed order (MFMA accumulation over tiles in tile order, xor butterflies, fixed
// LDS reductions); there are no floating-point atomics: two launches on the same inputs give the
// same bits.
#include "actdraw.h"
#include "common.h"

namespace dppo {
namespace {

constexpr int S = 32;     // samples per tile
// Head-delta image of AB blocks of 16 actions: per sample [0, 16 AB) dout, [16 AB, 32 AB) d log_std
// terms, stride 32 AB + 4
constexpr int sdo_of(int AB) { return 32 * AB + 4; }
constexpr int kMinTiles = 2;  // tiles per workgroup before another workgroup (slab) is added
constexpr float kLogSqrt2Pi = 0.91893853320467274178f;
constexpr float kHalfLog2PiPlusHalf = 1.41893853320467274178f;

struct WLds {  // offsets (floats)
  int X0, H1, H2, HA, HC, DZA, DOUT, WO, WV, BO, LS, IDX;
  int SX;  // X0 stride
  int total;
};

WLds make_wlds(int H, int D16, int AB) {
  WLds L{};
  const int SH = H + 4;
  int o = 0;
  L.SX = D16 + 4;
  L.X0 = o; o += S * L.SX;
  L.H1 = o; o += S * SH;
  L.H2 = o; o += S * SH;
  L.HA = o; o += S * SH;
  L.HC = o; o += S * SH;
  L.DZA = o; o += S * SH;
  L.DOUT = o; o += S * sdo_of(AB);
  L.WO = o; o += 16 * AB * H;
  L.WV = o; o += H;
  L.BO = o; o += 16 * AB;
  L.LS = o; o += 16 * AB;
  L.IDX = o; o += S;
  L.total = o;
  return L;
}

struct WArgs {
  WLds L;
  ParamOffsets po;
  const float* params;
  // minibatch kernel
  const float* rec;
  const int32_t* idx;
  int m;
  float inv_m, clip_eps, vf, ent;
  float* slabs;
  int64_t slab_stride, p_total;
  // evaluation kernel
  const float* obs;       // [n][D]
  const void* actions;    // int32 [n] or float [n][A]; null: values only
  float* logp;
  float* values;
  int64_t n;
  int D, D8, D16, A, R;
  // minibatch kernel, SEG form (last: the fields above keep their kernel-argument offsets)
  const int32_t* seg;  // global-minibatch DP: {start, end} of this minibatch in idx (device)
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ f32x4 tanh4(f32x4 x) {
  const f32x2 a = tanh2((f32x2){x[0], x[1]});
  const f32x2 b = tanh2((f32x2){x[2], x[3]});
  return {a[0], a[1], b[0], b[1]};
}

// acc[h] += W[16q.., 0..K) X[16h.., 0..K)^T for both sample halves; W rows of `ldw` floats in
// global memory.  ALIGNED: K and ldw are multiples of 16 and 4 (16-B A loads); otherwise 4-B
// loads guarded by k < kreal (layer 1: W1 is [H][D] with no padding).
template <bool ALIGNED>
__device__ __forceinline__ void fwd_mm(const float* __restrict__ W, int ldw, int K, int kreal,
                                       const float* X, int sx, int q, int lane, f32x4 acc[2]) {
  const int r = lane & 15, g = lane >> 4;
  const float* wrow = W + (int64_t)(16 * q + r) * ldw + 4 * g;
  const float* x0 = X + r * sx + 4 * g;
  const float* x1 = x0 + 16 * sx;
  for (int j = 0; j < K; j += 16) {
    f32x4 a;
    if (ALIGNED) {
      a = *(const f32x4*)(wrow + j);
    } else {
      const int k = j + 4 * g;
#pragma unroll
      for (int i = 0; i < 4; ++i) a[i] = k + i < kreal ? wrow[j + i] : 0.0f;
    }
    const f32x4 b0 = *(const f32x4*)(x0 + j);
    const f32x4 b1 = *(const f32x4*)(x1 + j);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[0] = mfma4(a[i], b0[i], acc[0]);
      acc[1] = mfma4(a[i], b1[i], acc[1]);
    }
  }
}

// acc[h] += W[:, 16q..]^T DZ[16h.., :]^T: the delta of the layer's input features [16q, 16q+16)
template <int H>
__device__ __forceinline__ void bwd_mm(const float* __restrict__ W, const float* DZ, int q,
                                       int lane, f32x4 acc[2]) {
  constexpr int SH = H + 4;
  const int r = lane & 15, g = lane >> 4;
  const float* wcol = W + (4 * g) * H + 16 * q + r;
  const float* z0 = DZ + r * SH + 4 * g;
  const float* z1 = z0 + 16 * SH;
#pragma unroll 2
  for (int j = 0; j < H; j += 16) {
    f32x4 a;
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = wcol[(j + i) * H];
    const f32x4 b0 = *(const f32x4*)(z0 + j);
    const f32x4 b1 = *(const f32x4*)(z1 + j);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      acc[0] = mfma4(a[i], b0[i], acc[0]);
      acc[1] = mfma4(a[i], b1[i], acc[1]);
    }
  }
}

// acc[cb] += DZ[:, 16q..]^T X[:, 16cb..] over the tile's 32 samples, cb < ncb; bsum += this
// lane's share of the bias gradient (samples = lane group mod 4)
template <int NCB>
__device__ __forceinline__ void wgrad_mm(const float* DZ, int sz, const float* X, int sx, int ncb,
                                         int q, int lane, f32x4 (&acc)[NCB], float& bsum) {
  const int r = lane & 15, g = lane >> 4;
  const float* z = DZ + g * sz + 16 * q + r;
  const float* x = X + g * sx + r;
#pragma unroll 2
  for (int t = 0; t < S / 4; ++t) {
    const float a = z[4 * t * sz];
    bsum += a;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
      if (cb < ncb) acc[cb] = mfma4(a, x[4 * t * sx + 16 * cb], acc[cb]);
  }
}

// bias + tanh of a forward product, into image Y: lane register v = feature 16q + 4g + v of
// sample 16h + r
template <int H>
__device__ __forceinline__ void act_store(const f32x4 acc[2], const float* __restrict__ bias,
                                          float* Y, int q, int lane) {
  constexpr int SH = H + 4;
  const int r = lane & 15, g = lane >> 4;
  const f32x4 b = *(const f32x4*)(bias + 16 * q + 4 * g);
  *(f32x4*)(Y + r * SH + 16 * q + 4 * g) = tanh4(acc[0] + b);
  *(f32x4*)(Y + (16 + r) * SH + 16 * q + 4 * g) = tanh4(acc[1] + b);
}

// delta through tanh, in place: Y <- dY * (1 - Y^2) on this lane's own elements
template <int H>
__device__ __forceinline__ void delta_store(const f32x4 acc[2], float* Y, int q, int lane) {
  constexpr int SH = H + 4;
  const int r = lane & 15, g = lane >> 4;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    f32x4* p = (f32x4*)(Y + (16 * h + r) * SH + 16 * q + 4 * g);
    const f32x4 y = *p;
    *p = acc[h] * (1.0f - y * y);
  }
}

template <int LPS>
__device__ __forceinline__ float sample_sum(float x) {
#pragma unroll
  for (int mask = 1; mask < LPS; mask <<= 1) x += __shfl_xor(x, mask);
  return x;
}

// sum over the four 16-lane groups in a fixed order, valid in every lane
__device__ __forceinline__ float group_sum(float x, int r) {
  const float a = __shfl(x, r), b = __shfl(x, r + 16), c = __shfl(x, r + 32),
              d = __shfl(x, r + 48);
  return (a + b) + (c + d);
}

// head weights into LDS: Wo rows >= A zero (NA = 16 AB rows)
template <int H, int NA = 16>
__device__ __forceinline__ void stage_heads(const WArgs& a, float* lds, bool cont) {
  constexpr int kThreads = H * 4;
  const int tid = threadIdx.x;
  const float* P = a.params;
  for (int e = tid; e < NA * H; e += kThreads)
    lds[a.L.WO + e] = e < a.A * H ? P[a.po.Wo + e] : 0.0f;
  for (int e = tid; e < H; e += kThreads) lds[a.L.WV + e] = P[a.po.Wv + e];
  if (tid < NA) {
    lds[a.L.BO + tid] = tid < a.A ? P[a.po.bo + tid] : 0.0f;
    lds[a.L.LS + tid] = cont && tid < a.A ? P[a.po.ls + tid] : 0.0f;
  }
}

// hidden layers of one tile, X0 -> H1 -> H2 -> (HA), HC; ends behind a barrier.  CRITIC false (the
// rollout sampler): HC is not computed
template <int H, bool CRITIC = true>
__device__ __forceinline__ void forward_tile(const WArgs& a, float* lds, int q, int lane,
                                             bool actor) {
  constexpr int SH = H + 4;
  const float* P = a.params;
  {
    f32x4 acc[2] = {};
    fwd_mm<false>(P + a.po.W1, a.D, a.D16, a.D, lds + a.L.X0, a.L.SX, q, lane, acc);
    act_store<H>(acc, P + a.po.b1, lds + a.L.H1, q, lane);
  }
  __syncthreads();
  {
    f32x4 acc[2] = {};
    fwd_mm<true>(P + a.po.W2, H, H, H, lds + a.L.H1, SH, q, lane, acc);
    act_store<H>(acc, P + a.po.b2, lds + a.L.H2, q, lane);
  }
  __syncthreads();
  if (actor) {
    f32x4 acc[2] = {};
    fwd_mm<true>(P + a.po.Wa, H, H, H, lds + a.L.H2, SH, q, lane, acc);
    act_store<H>(acc, P + a.po.ba, lds + a.L.HA, q, lane);
  }
  if (CRITIC) {
    f32x4 acc[2] = {};
    fwd_mm<true>(P + a.po.Wc, H, H, H, lds + a.L.H2, SH, q, lane, acc);
    act_store<H>(acc, P + a.po.bc, lds + a.L.HC, q, lane);
  }
  __syncthreads();
}

// Actor head of one sample on its H/8 lanes (8 hidden features each): out[NA] (logits or Gaussian
// mean; entries >= A are bo's zero padding), identical in every lane of the sample.
template <int H, int NA>
__device__ __forceinline__ void heads_actor(const WArgs& a, const float* lds, const float (&ha)[8],
                                            int k0, bool actor, float (&out)[NA]) {
  constexpr int LPS = H / 8;
#pragma unroll
  for (int c = 0; c < NA; ++c) {
    out[c] = 0.0f;
    if (actor && c < a.A) {
      const float* w = lds + a.L.WO + c * H + k0;
      float p = 0.0f;
#pragma unroll
      for (int j = 0; j < 8; ++j) p += ha[j] * w[j];
      out[c] = sample_sum<LPS>(p) + lds[a.L.BO + c];
    }
  }
}

// Both heads of one sample: the value (identical in every lane of the sample), then heads_actor
template <int H, int NA>
__device__ __forceinline__ void heads_fwd(const WArgs& a, const float* lds, const float (&ha)[8],
                                          const float (&hc)[8], int k0, bool actor,
                                          float (&out)[NA], float& v) {
  constexpr int LPS = H / 8;
  float pv = 0.0f;
#pragma unroll
  for (int j = 0; j < 8; ++j) pv += hc[j] * lds[a.L.WV + k0 + j];
  v = sample_sum<LPS>(pv) + a.params[a.po.bv];
  heads_actor<H>(a, lds, ha, k0, actor, out);
}

// log-probability and entropy of one sample; discrete: p[], lp[] of the softmax; continuous:
// the per-action (x - mu) / var and z^2 - 1 left in p[], lp[]
template <bool CONT, int NA>
__device__ __forceinline__ void policy_terms(const WArgs& a, const float* lds,
                                             const float (&out)[NA], int action,
                                             const float* __restrict__ xact, float (&p)[NA],
                                             float (&lp)[NA], float& logp, float& ent) {
  if (CONT) {
    logp = 0.0f;
    ent = 0.0f;
#pragma unroll
    for (int c = 0; c < NA; ++c) {
      p[c] = 0.0f;
      lp[c] = 0.0f;
      if (c < a.A) {
        const float ls = lds[a.L.LS + c];
        const float sigma = expf(ls);
        const float var = sigma * sigma;
        const float log_scale = logf(sigma);
        const float d = xact[c] - out[c];
        logp += -(d * d) / (2.0f * var) - log_scale - kLogSqrt2Pi;
        ent += kHalfLog2PiPlusHalf + log_scale;
        const float z = d / sigma;
        p[c] = d / var;
        lp[c] = z * z - 1.0f;
      }
    }
  } else {
    float mx = out[0];
#pragma unroll
    for (int c = 1; c < NA; ++c)
      if (c < a.A) mx = fmaxf(mx, out[c]);
    float se = 0.0f;
#pragma unroll
    for (int c = 0; c < NA; ++c)
      if (c < a.A) se += expf(out[c] - mx);
    const float lse = mx + logf(se);
    logp = 0.0f;
    ent = 0.0f;
#pragma unroll
    for (int c = 0; c < NA; ++c) {
      p[c] = 0.0f;
      lp[c] = 0.0f;
      if (c < a.A) {
        lp[c] = out[c] - lse;
        p[c] = expf(lp[c]);
        if (c == action) logp = lp[c];
        ent -= fmaxf(lp[c], -3.402823466e+38f) * p[c];
      }
    }
  }
}

// NB1: 16-column blocks of dW1 held in registers (>= D16 / 16: 2, 4 or 8).  SEG: the minibatch is
// idx[seg[0], seg[1]), a rank's share of a global minibatch.  A template parameter and not a
// run-time branch: the H = 128 kernels are short of scalar registers, and the two values a branch
// keeps live cost the categorical ones 4-16 B of scratch per lane; this way the !SEG kernels are
// instruction for instruction what they were before segments existed.  AB: blocks of 16 actions (1,
// or 2 for 16 < A <= 32: twice the head registers, a second dWo accumulator); NA = 16 AB.
template <int H, bool CONT, int NB1, bool SEG, int AB = 1>
__global__ __launch_bounds__(H * 4, 1) void wide_mb_kernel(WArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int SH = H + 4;
  constexpr int NA = 16 * AB;
  constexpr int SDO = sdo_of(AB);
  constexpr int NCB = H / 16;  // 16-column blocks of an H-wide matrix
  constexpr int LPS = H / 8;   // lanes per sample in the gather and head phases
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int hs = tid / LPS, li = tid % LPS, k0 = 8 * li;
  const WLds& L = a.L;
  const float* P = a.params;
  const int ncb1 = a.D16 / 16;

  f32x4 aW1[NB1] = {}, aW2[NCB] = {}, aWa[NCB] = {}, aWc[NCB] = {};
  f32x4 aWo[AB] = {};
  float sb1 = 0.0f, sb2 = 0.0f, sba = 0.0f, sbc = 0.0f, sbo[AB] = {}, sls[AB] = {};
  float gWv[8] = {};
  float s_pi = 0.0f, s_v = 0.0f, s_h = 0.0f, s_bv = 0.0f;

  stage_heads<H, NA>(a, lds, CONT);
  int* sidx = (int*)(lds + L.IDX);
  int mm = a.m;
  const int32_t* idxp = a.idx;
  if constexpr (SEG) {  // this rank's share of a global minibatch is known only on the device
    const int s0 = a.seg[0];
    mm = a.seg[1] - s0;
    idxp += s0;
  }
  // A workgroup past the share's last tile (the grid is sized for a whole global minibatch; an
  // empty share has no tile at all) skips the loop: its accumulators are still zero and the
  // epilogue writes them, so its slab is a complete zero slab.
  const int ntiles = (mm + S - 1) / S;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    // ---- gather: the samples' observation rows into X0 (zero past D and for samples past m)
    {
      const int i = tile * S + hs;
      const bool valid = i < mm;
      const int id = valid ? idxp[i] : -1;
      if (li == 0) sidx[hs] = id;
      const f32x4* src = (const f32x4*)(a.rec + (int64_t)(valid ? id : 0) * a.R);
      for (int c = li; c < a.D16 / 4; c += LPS) {
        f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (valid && 4 * c < a.D8) v = src[c];
        *(f32x4*)(lds + L.X0 + hs * L.SX + 4 * c) = v;
      }
    }
    __syncthreads();
    forward_tile<H>(a, lds, q, lane, true);

    // ---- heads, per-sample loss, head back-propagation (VALU)
    {
      const int id = sidx[hs];
      const bool valid = id >= 0;
      float ha[8], hc[8];
      *(f32x4*)&ha[0] = *(const f32x4*)(lds + L.HA + hs * SH + k0);
      *(f32x4*)&ha[4] = *(const f32x4*)(lds + L.HA + hs * SH + k0 + 4);
      *(f32x4*)&hc[0] = *(const f32x4*)(lds + L.HC + hs * SH + k0);
      *(f32x4*)&hc[4] = *(const f32x4*)(lds + L.HC + hs * SH + k0 + 4);
      float out[NA], v;
      heads_fwd<H>(a, lds, ha, hc, k0, true, out, v);
      const float* sc = a.rec + (int64_t)(valid ? id : 0) * a.R + a.D8;
      const f32x4 s4 = *(const f32x4*)sc;  // {action bits, old log-prob, advantage, return}
      float p[NA], lp[NA], logp, ent;
      policy_terms<CONT>(a, lds, out, __float_as_int(s4[0]), sc + 4, p, lp, logp, ent);
      // clipped surrogate (ppo.py:266-270) and its derivative: maximum splits ties, clamp passes
      // the gradient on the closed interval
      const float adv = s4[2];
      const float ratio = expf(logp - s4[1]);
      const float lo = 1.0f - a.clip_eps, hi = 1.0f + a.clip_eps;
      const float rc = fminf(fmaxf(ratio, lo), hi);
      const float u = -adv * ratio, w = -adv * rc;
      const float inr = (ratio >= lo && ratio <= hi) ? 1.0f : 0.0f;
      const float gu = u > w ? 1.0f : (u == w ? 0.5f : 0.0f);
      const float gw = w > u ? 1.0f : (u == w ? 0.5f : 0.0f);
      const float dratio = (gu * -adv + gw * -adv * inr) * a.inv_m;
      const float dlogp = valid ? dratio * ratio : 0.0f;
      const float verr = v - s4[3];
      const float dv = valid ? a.vf * verr * a.inv_m : 0.0f;
      const float entc = valid ? a.ent * a.inv_m : 0.0f;
      if (li == 0 && valid) {
        s_pi += fmaxf(u, w);
        s_v += 0.5f * verr * verr;
        s_h += ent;
        s_bv += dv;
      }
      float dout[NA];
#pragma unroll
      for (int c = 0; c < NA; ++c) {
        if (CONT) {
          dout[c] = dlogp * p[c];
          lp[c] = dlogp * lp[c];  // d log_std term
        } else {
          const float oh = (c == __float_as_int(s4[0])) ? 1.0f : 0.0f;
          dout[c] = c < a.A ? dlogp * (oh - p[c]) + entc * p[c] * (lp[c] + ent) : 0.0f;
          lp[c] = 0.0f;
        }
      }
      if (li == 0) {
        float* d = lds + L.DOUT + hs * SDO;
#pragma unroll
        for (int c = 0; c < NA; c += 4) {
          *(f32x4*)(d + c) = (f32x4){dout[c], dout[c + 1], dout[c + 2], dout[c + 3]};
          *(f32x4*)(d + NA + c) = (f32x4){lp[c], lp[c + 1], lp[c + 2], lp[c + 3]};
        }
      }
      float dza[8], dzc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        dza[j] = 0.0f;
        gWv[j] += dv * hc[j];
        dzc[j] = dv * lds[L.WV + k0 + j] * (1.0f - hc[j] * hc[j]);
      }
#pragma unroll
      for (int c = 0; c < NA; ++c) {
        if (c < a.A) {
          const float* wo = lds + L.WO + c * H + k0;
#pragma unroll
          for (int j = 0; j < 8; ++j) dza[j] += dout[c] * wo[j];
        }
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) dza[j] *= 1.0f - ha[j] * ha[j];
      *(f32x4*)(lds + L.DZA + hs * SH + k0) = *(const f32x4*)&dza[0];
      *(f32x4*)(lds + L.DZA + hs * SH + k0 + 4) = *(const f32x4*)&dza[4];
      *(f32x4*)(lds + L.HC + hs * SH + k0) = *(const f32x4*)&dzc[0];  // HC <- dZc
      *(f32x4*)(lds + L.HC + hs * SH + k0 + 4) = *(const f32x4*)&dzc[4];
    }
    __syncthreads();

    // ---- head layers: weight gradients of Wa, Wc, Wo and the delta of H2
    f32x4 dh[2] = {};
    wgrad_mm<NCB>(lds + L.DZA, SH, lds + L.H2, SH, NCB, q, lane, aWa, sba);
    wgrad_mm<NCB>(lds + L.HC, SH, lds + L.H2, SH, NCB, q, lane, aWc, sbc);
    {
      // dWo[a, 16q..] += dout[s, a] HA[s, 16q..]; the same A operand sums to d bo
      const float* z = lds + L.DOUT + g * SDO + r;
      const float* x = lds + L.HA + g * SH + 16 * q + r;
#pragma unroll 2
      for (int t = 0; t < S / 4; ++t) {
        const float xv = x[4 * t * SH];
#pragma unroll
        for (int ab = 0; ab < AB; ++ab) {
          const float av = z[4 * t * SDO + 16 * ab];
          sbo[ab] += av;
          if (CONT) sls[ab] += z[4 * t * SDO + NA + 16 * ab];
          aWo[ab] = mfma4(av, xv, aWo[ab]);
        }
      }
    }
    bwd_mm<H>(P + a.po.Wa, lds + L.DZA, q, lane, dh);
    bwd_mm<H>(P + a.po.Wc, lds + L.HC, q, lane, dh);
    __syncthreads();
    delta_store<H>(dh, lds + L.H2, q, lane);  // H2 <- dZ2
    __syncthreads();
    // ---- layer 2
    dh[0] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    dh[1] = dh[0];
    wgrad_mm<NCB>(lds + L.H2, SH, lds + L.H1, SH, NCB, q, lane, aW2, sb2);
    bwd_mm<H>(P + a.po.W2, lds + L.H2, q, lane, dh);
    __syncthreads();
    delta_store<H>(dh, lds + L.H1, q, lane);  // H1 <- dZ1
    __syncthreads();
    // ---- layer 1
    wgrad_mm<NB1>(lds + L.H1, SH, lds + L.X0, L.SX, ncb1, q, lane, aW1, sb1);
    __syncthreads();
  }

  // ---- this workgroup's slab: every real parameter written once, padding left as it is (zero)
  float* slab = a.slabs + (int64_t)blockIdx.x * a.slab_stride;
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int o = (16 * q + 4 * g + v) * H + 16 * cb + r;
      slab[a.po.W2 + o] = aW2[cb][v];
      slab[a.po.Wa + o] = aWa[cb][v];
      slab[a.po.Wc + o] = aWc[cb][v];
    }
  }
#pragma unroll
  for (int cb = 0; cb < NB1; ++cb) {
    const int k = 16 * cb + r;
    if (k < a.D) {
#pragma unroll
      for (int v = 0; v < 4; ++v) slab[a.po.W1 + (16 * q + 4 * g + v) * a.D + k] = aW1[cb][v];
    }
  }
#pragma unroll
  for (int ab = 0; ab < AB; ++ab) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int c = 16 * ab + 4 * g + v;
      if (c < a.A) slab[a.po.Wo + c * H + 16 * q + r] = aWo[ab][v];
    }
  }
  {
    const float t1 = group_sum(sb1, r), t2 = group_sum(sb2, r), ta = group_sum(sba, r),
                tc = group_sum(sbc, r);
    float to[AB], tl[AB];
#pragma unroll
    for (int ab = 0; ab < AB; ++ab) {
      to[ab] = group_sum(sbo[ab], r);
      tl[ab] = group_sum(sls[ab], r);
    }
    if (g == 0) {
      slab[a.po.b1 + 16 * q + r] = t1;
      slab[a.po.b2 + 16 * q + r] = t2;
      slab[a.po.ba + 16 * q + r] = ta;
      slab[a.po.bc + 16 * q + r] = tc;
#pragma unroll
      for (int ab = 0; ab < AB; ++ab) {
        if (q == 0 && 16 * ab + r < a.A) {
          slab[a.po.bo + 16 * ab + r] = to[ab];
          if (CONT) slab[a.po.ls + 16 * ab + r] = tl[ab];
        }
      }
    }
  }
  // critic output layer and the loss sums: per-thread partials over this thread's sample slot,
  // summed over the 32 slots in slot order
  float* red = lds + L.H1;        // [S][H]
  float* red4 = lds + L.X0;       // [S][4]
#pragma unroll
  for (int j = 0; j < 8; ++j) red[hs * H + k0 + j] = gWv[j];
  if (li == 0) *(f32x4*)(red4 + 4 * hs) = (f32x4){s_pi, s_v, s_h, s_bv};
  __syncthreads();
  if (tid < H) {
    float t = 0.0f;
    for (int s = 0; s < S; ++s) t += red[s * H + tid];
    slab[a.po.Wv + tid] = t;
  }
  if (tid >= 64 && tid < 72) {
    const int c = tid - 64;
    float t = 0.0f;
    if (c < 4)
      for (int s = 0; s < S; ++s) t += red4[4 * s + c];
    if (c == 3) {
      slab[a.po.bv] = t;
      t = 0.0f;
    }
    slab[a.p_total + c] = t;  // {sum l_pi, sum l_v, sum H, 0, ...}
  }
}

// Old-policy evaluation, one pass: log-probs (actions given) and values of obs[n][D]
template <int H, bool CONT, int AB = 1>
__global__ __launch_bounds__(H * 4, 1) void wide_eval_kernel(WArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int SH = H + 4;
  constexpr int NA = 16 * AB;
  constexpr int LPS = H / 8;
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int hs = tid / LPS, li = tid % LPS, k0 = 8 * li;
  const WLds& L = a.L;
  const bool actor = a.actions != nullptr;
  stage_heads<H, NA>(a, lds, CONT);
  const int64_t ntiles = (a.n + S - 1) / S;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t i = tile * S + hs;
    const bool valid = i < a.n;
    {
      const float* src = a.obs + (valid ? i : 0) * a.D;
      for (int k = li; k < a.D16; k += LPS)
        lds[L.X0 + hs * L.SX + k] = (valid && k < a.D) ? src[k] : 0.0f;
    }
    __syncthreads();
    forward_tile<H>(a, lds, q, lane, actor);
    float ha[8] = {}, hc[8];
    if (actor) {
      *(f32x4*)&ha[0] = *(const f32x4*)(lds + L.HA + hs * SH + k0);
      *(f32x4*)&ha[4] = *(const f32x4*)(lds + L.HA + hs * SH + k0 + 4);
    }
    *(f32x4*)&hc[0] = *(const f32x4*)(lds + L.HC + hs * SH + k0);
    *(f32x4*)&hc[4] = *(const f32x4*)(lds + L.HC + hs * SH + k0 + 4);
    float out[NA], v;
    heads_fwd<H>(a, lds, ha, hc, k0, actor, out, v);
    if (valid && li == 0) a.values[i] = v;
    if (actor) {
      float p[NA], lp[NA], logp, ent;
      float xa[NA] = {};
      int action = 0;
      if (CONT) {
        const float* ac = (const float*)a.actions + (valid ? i : 0) * a.A;
#pragma unroll
        for (int c = 0; c < NA; ++c)
          if (c < a.A) xa[c] = ac[c];
      } else {
        action = ((const int32_t*)a.actions)[valid ? i : 0];
      }
      policy_terms<CONT>(a, lds, out, action, xa, p, lp, logp, ent);
      if (valid && li == 0) a.logp[i] = logp;
    }
    __syncthreads();
  }
}

// Action sampling for the rollout (get_actions, ppo.py:73-82 / continuous_ppo.py:83-93) at wide
// shapes: the actor half of wide_eval_kernel (X0 -> H1 -> H2 -> HA -> heads; no critic layer, no
// value), then the draw of actdraw.h on lane li == 0 of each valid sample -- the stream of
// mlp.hip's act_kernel.  Optional outputs: heads [n][A], actions (int32 [n] or float [n][A]) and,
// with them, the squashed environment actions.
struct WActArgs {
  WArgs w;
  float* heads;
  void* actions;
  float* env_act;
  int squash;  // 1: tanh(u), 2: sq_lo + (tanh(u) + 1) * sq_half
  float sq_lo[32], sq_half[32], sq_hi[32];
  uint32_t seed_lo, seed_hi, ctr_lo, ctr_hi;
  int A;
};

template <int H, bool CONT, int AB = 1>
__global__ __launch_bounds__(H * 4, 1) void wide_act_kernel(WActArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int SH = H + 4;
  constexpr int NA = 16 * AB;
  constexpr int LPS = H / 8;
  const int tid = threadIdx.x, lane = tid & 63, q = tid >> 6;
  const int hs = tid / LPS, li = tid % LPS, k0 = 8 * li;
  const WArgs& w = a.w;
  const WLds& L = w.L;
  stage_heads<H, NA>(w, lds, CONT);
  const int64_t ntiles = (w.n + S - 1) / S;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t i = tile * S + hs;
    const bool valid = i < w.n;
    {
      const float* src = w.obs + (valid ? i : 0) * w.D;
      for (int k = li; k < w.D16; k += LPS)
        lds[L.X0 + hs * L.SX + k] = (valid && k < w.D) ? src[k] : 0.0f;
    }
    __syncthreads();
    forward_tile<H, false>(w, lds, q, lane, true);
    float ha[8];
    *(f32x4*)&ha[0] = *(const f32x4*)(lds + L.HA + hs * SH + k0);
    *(f32x4*)&ha[4] = *(const f32x4*)(lds + L.HA + hs * SH + k0 + 4);
    float out[NA];
    heads_actor<H>(w, lds, ha, k0, true, out);
    if (valid && li == 0) {
      if (a.heads) {
#pragma unroll
        for (int c = 0; c < NA; ++c)
          if (c < a.A) a.heads[i * a.A + c] = out[c];
      }
      if (a.actions) {
        if (CONT) {
          draw_gaussian<NA>(a, out, lds + L.LS, i, (float*)a.actions + i * a.A);
        } else {
          ((int32_t*)a.actions)[i] = draw_categorical<NA>(a, out, i);
        }
      }
    }
    __syncthreads();
  }
}

// Sample records for the wide minibatch gather, in pack_kernel's layout (gae.hip): one thread per
// 16-B piece of a record; the advantage statistics come finalised in mean_std.
struct WPackArgs {
  PackArgs p;
  const float* mean_std;
};

__global__ __launch_bounds__(256) void wide_pack_kernel(WPackArgs w) {
  const PackArgs& a = w.p;
  const int R4 = a.R / 4;
  const int64_t total = a.B * R4;
  float mean = 0.0f, denom = 1.0f;
  if (a.advantage_norm) {
    mean = w.mean_std[0];
    denom = w.mean_std[1] + 1e-6f;
  }
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = e / R4;
    const int k = (int)(e - i * R4) * 4;
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (k < a.D8) {
      const float* o = a.obs + i * a.D;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (k + j < a.D) v[j] = o[k + j];
    } else if (k == a.D8) {
      float adv = a.adv[i];
      if (a.advantage_norm) adv = (adv - mean) / denom;  // ppo.py:243, fp32 as the reference
      if (a.adv_out) a.adv_out[i] = adv;
      v = (f32x4){a.continuous ? 0.0f : __int_as_float(((const int32_t*)a.actions)[i]), a.logp[i],
                  adv, a.ret[i]};
    } else {
      const int c = k - a.D8 - 4;
      const float* sa = (const float*)a.actions + i * a.A;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c + j < a.A) v[j] = sa[c + j];
    }
    *(f32x4*)(a.rec + i * a.R + k) = v;
  }
}

inline int cus_of(const MlpShape& sh) { return sh.cus > 0 ? sh.cus : 256; }

inline int ab_of(const MlpShape& sh) { return sh.A > 16 ? 2 : 1; }  // blocks of 16 actions

WArgs base_args(const MlpShape& sh, const ParamOffsets& po, const float* params) {
  WArgs k{};
  const int D16 = (sh.D + 15) / 16 * 16;
  k.L = make_wlds(sh.H, D16, ab_of(sh));
  k.po = po;
  k.params = params;
  k.D = sh.D;
  k.D8 = sh.D8;
  k.D16 = D16;
  k.A = sh.A;
  k.R = sh.R;
  return k;
}

void raise_wide_lds() {
  static const bool attr = [] {
#define DPPO_WSET3(H_, C_, G_)                                  \
  raise_dyn_lds((const void*)wide_mb_kernel<H_, C_, 2, G_>);    \
  raise_dyn_lds((const void*)wide_mb_kernel<H_, C_, 4, G_>);    \
  raise_dyn_lds((const void*)wide_mb_kernel<H_, C_, 8, G_>);
#define DPPO_WSET(H_, C_) DPPO_WSET3(H_, C_, false) DPPO_WSET3(H_, C_, true)
    DPPO_WSET(64, false) DPPO_WSET(64, true) DPPO_WSET(128, false) DPPO_WSET(128, true)
#undef DPPO_WSET
#undef DPPO_WSET3
    // large heads: hidden 64, no segments; one action block only where D16 > 128
#define DPPO_WSETL(C_)                                                \
  raise_dyn_lds((const void*)wide_mb_kernel<64, C_, 2, false, 2>);    \
  raise_dyn_lds((const void*)wide_mb_kernel<64, C_, 4, false, 2>);    \
  raise_dyn_lds((const void*)wide_mb_kernel<64, C_, 8, false, 2>);    \
  raise_dyn_lds((const void*)wide_mb_kernel<64, C_, 12, false, 1>);   \
  raise_dyn_lds((const void*)wide_mb_kernel<64, C_, 12, false, 2>);   \
  raise_dyn_lds((const void*)wide_mb_kernel<64, C_, 16, false, 1>);   \
  raise_dyn_lds((const void*)wide_mb_kernel<64, C_, 16, false, 2>);   \
  raise_dyn_lds((const void*)wide_mb_kernel<64, C_, 24, false, 1>);   \
  raise_dyn_lds((const void*)wide_mb_kernel<64, C_, 24, false, 2>);   \
  raise_dyn_lds((const void*)wide_eval_kernel<64, C_, 2>);            \
  raise_dyn_lds((const void*)wide_act_kernel<64, C_, 2>);
    DPPO_WSETL(false) DPPO_WSETL(true)
#undef DPPO_WSETL
    raise_dyn_lds((const void*)wide_eval_kernel<64, false>);
    raise_dyn_lds((const void*)wide_eval_kernel<64, true>);
    raise_dyn_lds((const void*)wide_eval_kernel<128, false>);
    raise_dyn_lds((const void*)wide_eval_kernel<128, true>);
    raise_dyn_lds((const void*)wide_act_kernel<64, false>);
    raise_dyn_lds((const void*)wide_act_kernel<64, true>);
    raise_dyn_lds((const void*)wide_act_kernel<128, false>);
    raise_dyn_lds((const void*)wide_act_kernel<128, true>);
    return true;
  }();
  (void)attr;
}

}  // namespace

size_t wide_lds_bytes(const MlpShape& sh) {
  return (size_t)make_wlds(sh.H, (sh.D + 15) / 16 * 16, ab_of(sh)).total * sizeof(float);
}

int wide_tile() { return S; }

int wide_grid(const MlpShape& sh, int32_t m) {
  const int ntiles = (m + S - 1) / S;
  int g = ntiles / kMinTiles;
  const int cus = cus_of(sh);
  if (g > cus) g = cus;
  if (g < 1) g = 1;
  return g;
}

int launch_wide_mb(const MlpShape& sh, const ParamOffsets& po, const GradArgs& ga, int G,
                   hipStream_t s) {
  if (!wide_shape(sh)) {
    set_error("wide minibatch kernel: unsupported shape");
    return DPPO_EUNSUPPORTED;
  }
  if (wide_large_shape(sh) && ga.seg) {
    set_error("wide minibatch kernel: large heads (obs_dim > 128 or act_dim > 16) run on one rank");
    return DPPO_EUNSUPPORTED;
  }
  WArgs k = base_args(sh, po, ga.params);
  k.rec = ga.rec;
  k.idx = ga.idx;
  k.seg = ga.seg;  // with segments G is the handle's grid, sized for a whole global minibatch
  k.m = ga.m;
  k.inv_m = ga.inv_m;
  k.clip_eps = ga.clip_eps;
  k.vf = ga.vf_coef;
  k.ent = ga.ent_coef;
  k.slabs = ga.slabs;
  k.slab_stride = ga.slab_stride;
  k.p_total = ga.p_total;
  const size_t lds = (size_t)k.L.total * sizeof(float);
  raise_wide_lds();
  const dim3 grid((unsigned)(G < 1 ? 1 : G)), block((unsigned)(sh.H * 4));
  const bool c = sh.continuous != 0;
  const int nb1 = k.D16 / 16;
#define DPPO_WLAUNCH3(H_, C_, G_)                                                            \
  do {                                                                                       \
    if (nb1 <= 2) DPPO_LAUNCH((wide_mb_kernel<H_, C_, 2, G_>), grid, block, lds, s, k);      \
    else if (nb1 <= 4) DPPO_LAUNCH((wide_mb_kernel<H_, C_, 4, G_>), grid, block, lds, s, k); \
    else DPPO_LAUNCH((wide_mb_kernel<H_, C_, 8, G_>), grid, block, lds, s, k);               \
  } while (0)
#define DPPO_WLAUNCH(H_, C_)                    \
  do {                                          \
    if (k.seg) DPPO_WLAUNCH3(H_, C_, true);     \
    else DPPO_WLAUNCH3(H_, C_, false);          \
  } while (0)
  // large heads (hidden 64, no segments): NB1 12 / 16 / 24 past D16 = 128, AB_ blocks of 16 actions
#define DPPO_WLAUNCHL(C_, AB_)                                                                   \
  do {                                                                                           \
    if (nb1 <= 2) DPPO_LAUNCH((wide_mb_kernel<64, C_, 2, false, AB_>), grid, block, lds, s, k);  \
    else if (nb1 <= 4)                                                                           \
      DPPO_LAUNCH((wide_mb_kernel<64, C_, 4, false, AB_>), grid, block, lds, s, k);              \
    else if (nb1 <= 8)                                                                           \
      DPPO_LAUNCH((wide_mb_kernel<64, C_, 8, false, AB_>), grid, block, lds, s, k);              \
    else if (nb1 <= 12)                                                                          \
      DPPO_LAUNCH((wide_mb_kernel<64, C_, 12, false, AB_>), grid, block, lds, s, k);             \
    else if (nb1 <= 16)                                                                          \
      DPPO_LAUNCH((wide_mb_kernel<64, C_, 16, false, AB_>), grid, block, lds, s, k);             \
    else DPPO_LAUNCH((wide_mb_kernel<64, C_, 24, false, AB_>), grid, block, lds, s, k);          \
  } while (0)
  if (wide_large_shape(sh)) {
    if (sh.A > 16) {
      if (c) DPPO_WLAUNCHL(true, 2);
      else DPPO_WLAUNCHL(false, 2);
    } else {
      if (c) DPPO_WLAUNCHL(true, 1);
      else DPPO_WLAUNCHL(false, 1);
    }
  } else if (sh.H == 128) {
    if (c) DPPO_WLAUNCH(128, true);
    else DPPO_WLAUNCH(128, false);
  } else {
    if (c) DPPO_WLAUNCH(64, true);
    else DPPO_WLAUNCH(64, false);
  }
#undef DPPO_WLAUNCHL
#undef DPPO_WLAUNCH
#undef DPPO_WLAUNCH3
  DPPO_LAUNCH_CHECK();
  return DPPO_OK;
}

int launch_wide_eval(const MlpShape& sh, const ParamOffsets& po, const float* params,
                     const float* obs, const void* actions, const float* next_obs, float* logp,
                     float* values, float* next_values, int64_t n, hipStream_t s) {
  if (!wide_shape(sh)) {
    set_error("wide evaluation kernel: unsupported shape");
    return DPPO_EUNSUPPORTED;
  }
  if (n <= 0) return DPPO_OK;
  raise_wide_lds();
  const bool c = sh.continuous != 0;
  const int64_t ntiles = (n + S - 1) / S;
  const int cus = cus_of(sh);
  const dim3 grid((unsigned)(ntiles < cus ? ntiles : cus)), block((unsigned)(sh.H * 4));
  for (int pass = 0; pass < 2; ++pass) {
    WArgs k = base_args(sh, po, params);
    k.obs = pass == 0 ? obs : next_obs;
    k.actions = pass == 0 ? actions : nullptr;
    k.logp = logp;
    k.values = pass == 0 ? values : next_values;
    k.n = n;
    const size_t lds = (size_t)k.L.total * sizeof(float);
    if (sh.A > 16) {  // hidden 64: wide_shape
      if (c) DPPO_LAUNCH((wide_eval_kernel<64, true, 2>), grid, block, lds, s, k);
      else DPPO_LAUNCH((wide_eval_kernel<64, false, 2>), grid, block, lds, s, k);
    } else if (sh.H == 128) {
      if (c) DPPO_LAUNCH((wide_eval_kernel<128, true>), grid, block, lds, s, k);
      else DPPO_LAUNCH((wide_eval_kernel<128, false>), grid, block, lds, s, k);
    } else {
      if (c) DPPO_LAUNCH((wide_eval_kernel<64, true>), grid, block, lds, s, k);
      else DPPO_LAUNCH((wide_eval_kernel<64, false>), grid, block, lds, s, k);
    }
    DPPO_LAUNCH_CHECK();
  }
  return DPPO_OK;
}

int launch_wide_act(const MlpShape& sh, const ParamOffsets& po, const float* params,
                    const float* obs, void* actions, int64_t n, uint64_t seed, uint64_t counter,
                    hipStream_t s, float* heads, const ActSquash* squash) {
  if (!wide_shape(sh)) {
    set_error("wide actor kernel: unsupported shape");
    return DPPO_EUNSUPPORTED;
  }
  if (n <= 0) return DPPO_OK;
  WActArgs k{};
  if (squash && squash->env_actions) {
    if (!sh.continuous || sh.A > 32) {
      set_error("tanh squash needs a continuous action space of at most 32 dims");
      return DPPO_EINVAL;
    }
    k.env_act = squash->env_actions;
    k.squash = squash->low && squash->high ? 2 : 1;
    for (int j = 0; j < sh.A && k.squash == 2; ++j) {
      k.sq_lo[j] = squash->low[j];
      k.sq_half[j] = 0.5f * (squash->high[j] - squash->low[j]);
      k.sq_hi[j] = squash->high[j];
    }
  }
  k.w = base_args(sh, po, params);
  k.w.obs = obs;
  k.w.n = n;
  k.heads = heads;
  k.actions = actions;
  k.seed_lo = (uint32_t)seed;
  k.seed_hi = (uint32_t)(seed >> 32);
  k.ctr_lo = (uint32_t)counter;
  k.ctr_hi = (uint32_t)(counter >> 32);
  k.A = sh.A;
  raise_wide_lds();
  const bool c = sh.continuous != 0;
  const int64_t ntiles = (n + S - 1) / S;
  const int cus = cus_of(sh);
  const dim3 grid((unsigned)(ntiles < cus ? ntiles : cus)), block((unsigned)(sh.H * 4));
  const size_t lds = (size_t)k.w.L.total * sizeof(float);
  if (sh.A > 16) {  // hidden 64: wide_shape
    if (c) DPPO_LAUNCH((wide_act_kernel<64, true, 2>), grid, block, lds, s, k);
    else DPPO_LAUNCH((wide_act_kernel<64, false, 2>), grid, block, lds, s, k);
  } else if (sh.H == 128) {
    if (c) DPPO_LAUNCH((wide_act_kernel<128, true>), grid, block, lds, s, k);
    else DPPO_LAUNCH((wide_act_kernel<128, false>), grid, block, lds, s, k);
  } else {
    if (c) DPPO_LAUNCH((wide_act_kernel<64, true>), grid, block, lds, s, k);
    else DPPO_LAUNCH((wide_act_kernel<64, false>), grid, block, lds, s, k);
  }
  DPPO_LAUNCH_CHECK();
  return DPPO_OK;
}

int launch_wide_pack(const PackArgs& a, const float* mean_std, hipStream_t s) {
  if (a.B <= 0) return DPPO_OK;
  WPackArgs w{a, mean_std};
  const int64_t total = a.B * (a.R / 4);
  int64_t g = (total + 255) / 256;
  if (g > 4096) g = 4096;
  DPPO_LAUNCH(wide_pack_kernel, dim3((unsigned)g), dim3(256), 0, s, w);
  DPPO_LAUNCH_CHECK();
  return DPPO_OK;
}

}  // namespace dppo
