// GRU recurrence of a network that runs under the caller's autograd (RecurrentPPO's torch learn
// loop and rollout: network_hidden_dim != 64, wide observations, a custom network_cls around
// GRUCore), as two scans: the whole [T][N] forward sequence in one launch and the whole BPTT in
// another, instead of T cell launches each way (intended semantics of reference
// diamond/recurrent_ppo.py:41-91: a torch GRU cell stepped over t with the hidden state zeroed
// where dones[t], :82-87; restated in oracle/gru_torch.py::sequence).
//
// The input projection gi = x Wih^T + b_ih is NOT here: it is one GEMM over [T N, I] on the
// caller's side, and so are the five products of the backward that are sums over samples (dx, dWih,
// db_ih, dWhh, db_hh).  That leaves the kernels independent of the input width and of whatever
// surrounds the GRU.
//
// Mapping (grugrad.hip phases B and D, gruact.hip gru_forward): one 256-thread workgroup takes
// 256 / G envs over all T steps, G lanes per env, lane j = hidden unit j; an env never straddles a
// wave (G <= 64), so the per-step exchange of the hidden state (forward) and of the 3G gate deltas
// (backward) goes through LDS inside the wave, with no workgroup barrier in the time loop: a wave
// issues its LDS writes and reads in program order.  Whh sits in LDS with a row stride of G + 1
// (stage_whh): lane j's k-th read of its rows (forward) and its column reads (backward) fall on
// distinct consecutive banks.  The operands of the next step that do not depend on the carried
// state (gi, dones; dout, the saved gates, the earlier hidden state) are loaded a step ahead.
// Every sum runs over k in a fixed order inside one lane: no atomics, the same bits on every call,
// at any N and at any position in the batch.
#include "common.h"

namespace dppo {
namespace {

constexpr int kThr = 256;

template <int G>
struct ScanLds {
  float W[3 * G * (G + 1)];  // Whh, row stride G + 1
  float x[3 * kThr];         // per env: h [G] (forward) or the gate deltas [3G] (backward)
};

// Whh [3G][G] (16-byte aligned) with a row stride of G + 1
template <int G>
__device__ __forceinline__ void stage_whh(float* dst, const float* __restrict__ src, int tid) {
  static_assert(G % 4 == 0, "a 16-byte load stays inside a row");
  for (int k4 = tid; k4 < 3 * G * G / 4; k4 += kThr) {
    const f32x4 v = ((const f32x4*)src)[k4];
    const int k = 4 * k4;
    float* d = dst + (k / G) * (G + 1) + (k % G);
    d[0] = v[0];
    d[1] = v[1];
    d[2] = v[2];
    d[3] = v[3];
  }
}

struct ScanFwdArgs {
  const float* gi;       // [T][N][3G]
  const float* hx0;      // [N][G]
  const uint8_t* dones;  // [T][N] or null
  const float* Whh;      // [3G][G]
  const float* bhh;      // [3G]
  float* out;            // [T][N][G]
  float* saved;          // [T][N][4G] = r, z, n, gh_n; or null
  int64_t T, N;
};

template <int G>
__global__ __launch_bounds__(kThr) void gru_scan_fwd_kernel(ScanFwdArgs a) {
  constexpr int kEnvs = kThr / G, G3 = 3 * G, kWs = G + 1;
  __shared__ __attribute__((aligned(16))) ScanLds<G> lds;
  const int tid = threadIdx.x;
  stage_whh<G>(lds.W, a.Whh, tid);
  __syncthreads();
  const int e = tid / G, j = tid % G;
  const int64_t n = (int64_t)blockIdx.x * kEnvs + e;
  if (n >= a.N) return;  // no workgroup barrier below
  const int64_t T = a.T, N = a.N;
  const float* wr = lds.W + j * kWs;
  const float* wz = lds.W + (G + j) * kWs;
  const float* wn = lds.W + (2 * G + j) * kWs;
  const float br = a.bhh[j], bz = a.bhh[G + j], bn = a.bhh[2 * G + j];
  float* hb = lds.x + e * G;
  float h = a.hx0[n * G + j];
  // the next step's inputs are loaded a step ahead (they do not depend on h)
  float gir_n = a.gi[n * G3 + j], giz_n = a.gi[n * G3 + G + j], gin_n = a.gi[n * G3 + 2 * G + j];
  uint8_t done_n = a.dones ? a.dones[n] : (uint8_t)0;
  for (int64_t t = 0; t < T; ++t) {
    const int64_t i = t * N + n;
    const float gir = gir_n, giz = giz_n, gin = gin_n;
    const bool done = done_n != 0;
    {
      const int64_t in = (t + 1 < T ? t + 1 : T - 1) * N + n;
      gir_n = a.gi[in * G3 + j];
      giz_n = a.gi[in * G3 + G + j];
      gin_n = a.gi[in * G3 + 2 * G + j];
      if (a.dones) done_n = a.dones[in];
    }
    if (done) h = 0.0f;  // hx[:, dones[t]] = 0 (recurrent_ppo.py:84)
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
    const float r = sigm(gir + ghr), z = sigm(giz + ghz);
    const float nn = tanh_acc(gin + r * ghn);
    const float hn = (1.0f - z) * nn + z * h;
    a.out[i * G + j] = hn;
    if (a.saved) {
      float* sv = a.saved + i * (4 * G);
      sv[j] = r;
      sv[G + j] = z;
      sv[2 * G + j] = nn;
      sv[3 * G + j] = ghn;
    }
    h = hn;
  }
}

struct ScanBwdArgs {
  const float* dout;     // [T][N][G]
  const float* dhT;      // [N][G] or null (= 0)
  const float* saved;    // [T][N][4G]
  const float* out;      // [T][N][G]
  const float* hx0;      // [N][G]
  const uint8_t* dones;  // [T][N] or null
  const float* Whh;      // [3G][G]
  float* dgi;            // [T][N][3G]
  float* dgh;            // [T][N][3G]
  float* dh0;            // [N][G]
  int64_t T, N;
};

template <int G>
__global__ __launch_bounds__(kThr) void gru_scan_bwd_kernel(ScanBwdArgs a) {
  constexpr int kEnvs = kThr / G, G3 = 3 * G, kWs = G + 1;
  __shared__ __attribute__((aligned(16))) ScanLds<G> lds;
  const int tid = threadIdx.x;
  stage_whh<G>(lds.W, a.Whh, tid);
  __syncthreads();
  const int e = tid / G, j = tid % G;
  const int64_t n = (int64_t)blockIdx.x * kEnvs + e;
  if (n >= a.N) return;  // no workgroup barrier below
  const int64_t T = a.T, N = a.N;
  const float* wc = lds.W + j;  // column j
  float* gb = lds.x + e * G3;
  // the earlier step's operands are loaded a step ahead (they do not depend on dh)
  struct Saved {
    float dout, r, z, n, ghn, hprev;
    uint8_t done;
  };
  auto load = [&](int64_t t) {
    const int64_t i = t * N + n;
    const float* sv = a.saved + i * (4 * G);
    // the hidden state the step started from, before the reset
    const float hprev = t > 0 ? a.out[(i - N) * G + j] : a.hx0[n * G + j];
    return Saved{a.dout[i * G + j], sv[j], sv[G + j], sv[2 * G + j], sv[3 * G + j], hprev,
                 a.dones ? a.dones[i] : (uint8_t)0};
  };
  float dh = a.dhT ? a.dhT[n * G + j] : 0.0f;
  Saved nx = load(T - 1);
  for (int64_t t = T - 1; t >= 0; --t) {
    const int64_t i = t * N + n;
    const Saved cur = nx;
    nx = load(t > 0 ? t - 1 : 0);
    dh += cur.dout;
    const float r = cur.r, z = cur.z, nn = cur.n;
    const float hp = cur.done ? 0.0f : cur.hprev;
    const float dn = dh * (1.0f - z);
    const float dz = dh * (hp - nn);
    const float dan = dn * (1.0f - nn * nn);
    const float daz = dz * z * (1.0f - z);
    const float dar = (dan * cur.ghn) * r * (1.0f - r);
    const float dghn = dan * r;
    float* dgi = a.dgi + i * G3;
    float* dgh = a.dgh + i * G3;
    dgi[j] = dar;
    dgi[G + j] = daz;
    dgi[2 * G + j] = dan;
    dgh[j] = dar;
    dgh[G + j] = daz;
    dgh[2 * G + j] = dghn;
    gb[j] = dar;
    gb[G + j] = daz;
    gb[2 * G + j] = dghn;
    float dhp = dh * z;
#pragma unroll
    for (int q = 0; q < G3 / 4; ++q) {
      const f32x4 x = *(const f32x4*)(gb + 4 * q);
      dhp += wc[(4 * q) * kWs] * x[0] + wc[(4 * q + 1) * kWs] * x[1] +
             wc[(4 * q + 2) * kWs] * x[2] + wc[(4 * q + 3) * kWs] * x[3];
    }
    // hp = h_prev * keep  =>  dh_prev = dhp * keep
    dh = cur.done ? 0.0f : dhp;
  }
  a.dh0[n * G + j] = dh;
}

bool scan_width(int G) { return G == 16 || G == 32 || G == 64; }

// 0 when the geometry has no launch: unsupported G, T or N < 1, or more workgroups than a grid holds
int64_t scan_grid(int G, int64_t T, int64_t N) {
  if (!scan_width(G) || T < 1 || N < 1) return 0;
  const int64_t envs = kThr / G;
  const int64_t grid = (N + envs - 1) / envs;
  return grid > 0x7FFFFFFF ? 0 : grid;
}

bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int scan_check(const char* fn, int G, int64_t T, int64_t N) {
  if (!scan_width(G)) {
    set_error("%s: no scan kernel for gru_hidden=%d (16, 32 or 64)", fn, G);
    return DPPO_EUNSUPPORTED;
  }
  if (T < 1 || N < 1) {
    set_error("%s: T = %lld, N = %lld, need at least one step and one env", fn, (long long)T,
              (long long)N);
    return DPPO_EINVAL;
  }
  if (scan_grid(G, T, N) == 0) {
    set_error("%s: N = %lld is too large for one launch", fn, (long long)N);
    return DPPO_EINVAL;
  }
  return DPPO_OK;
}

template <int G>
void launch_fwd(unsigned grid, const ScanFwdArgs& a, hipStream_t s) {
  DPPO_LAUNCH(gru_scan_fwd_kernel<G>, dim3(grid), dim3(kThr), 0, s, a);
}
template <int G>
void launch_bwd(unsigned grid, const ScanBwdArgs& a, hipStream_t s) {
  DPPO_LAUNCH(gru_scan_bwd_kernel<G>, dim3(grid), dim3(kThr), 0, s, a);
}

}  // namespace
}  // namespace dppo

using namespace dppo;

extern "C" {

int dppo_gru_scan_plan(int32_t G, int64_t T, int64_t N, int64_t* out) {
  const int rc = scan_check("dppo_gru_scan_plan", G, T, N);
  if (rc != DPPO_OK) return rc;
  if (out) {
    out[0] = kThr / G;
    out[1] = scan_grid(G, T, N);
    out[2] = T * N * 4 * G;
    out[3] = T * N * 3 * G;
    out[4] = T * N * 3 * G;
  }
  return DPPO_OK;
}

int dppo_gru_scan_fwd_f32(const float* gi, const float* hx0, const uint8_t* dones,
                          const float* Whh, const float* b_hh, float* out, float* saved,
                          int64_t T, int64_t N, int32_t G, void* stream) {
  const char* fn = "dppo_gru_scan_fwd_f32";
  const int rc = scan_check(fn, G, T, N);
  if (rc != DPPO_OK) return rc;
  if (!gi || !hx0 || !Whh || !b_hh || !out) {
    set_error("%s: a required pointer is NULL", fn);
    return DPPO_EINVAL;
  }
  if (!aligned_to(Whh, 16)) {
    set_error("%s: Whh must be 16-byte aligned (staged with 16-byte loads)", fn);
    return DPPO_EINVAL;
  }
  if (!aligned_to(gi, 4) || !aligned_to(hx0, 4) || !aligned_to(b_hh, 4) || !aligned_to(out, 4) ||
      !aligned_to(saved, 4)) {
    set_error("%s: a float array is not 4-byte aligned", fn);
    return DPPO_EINVAL;
  }
  ScanFwdArgs a{gi, hx0, dones, Whh, b_hh, out, saved, T, N};
  const unsigned grid = (unsigned)scan_grid(G, T, N);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (G) {
    case 16: launch_fwd<16>(grid, a, s); break;
    case 32: launch_fwd<32>(grid, a, s); break;
    default: launch_fwd<64>(grid, a, s); break;
  }
  DPPO_LAUNCH_CHECK();
  return DPPO_OK;
}

int dppo_gru_scan_bwd_f32(const float* dout, const float* dh_T, const float* saved,
                          const float* out, const float* hx0, const uint8_t* dones,
                          const float* Whh, float* dgi, float* dgh, float* dh0, int64_t T,
                          int64_t N, int32_t G, void* stream) {
  const char* fn = "dppo_gru_scan_bwd_f32";
  const int rc = scan_check(fn, G, T, N);
  if (rc != DPPO_OK) return rc;
  if (!dout || !saved || !out || !hx0 || !Whh || !dgi || !dgh || !dh0) {
    set_error("%s: a required pointer is NULL", fn);
    return DPPO_EINVAL;
  }
  if (!aligned_to(Whh, 16)) {
    set_error("%s: Whh must be 16-byte aligned (staged with 16-byte loads)", fn);
    return DPPO_EINVAL;
  }
  if (!aligned_to(dout, 4) || !aligned_to(dh_T, 4) || !aligned_to(saved, 4) ||
      !aligned_to(out, 4) || !aligned_to(hx0, 4) || !aligned_to(dgi, 4) || !aligned_to(dgh, 4) ||
      !aligned_to(dh0, 4)) {
    set_error("%s: a float array is not 4-byte aligned", fn);
    return DPPO_EINVAL;
  }
  ScanBwdArgs a{dout, dh_T, saved, out, hx0, dones, Whh, dgi, dgh, dh0, T, N};
  const unsigned grid = (unsigned)scan_grid(G, T, N);
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (G) {
    case 16: launch_bwd<16>(grid, a, s); break;
    case 32: launch_bwd<32>(grid, a, s); break;
    default: launch_bwd<64>(grid, a, s); break;
  }
  DPPO_LAUNCH_CHECK();
  return DPPO_OK;
}

}  // extern "C"
