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
// Mapping: one 256-thread workgroup takes 256 / G envs over all T steps, G lanes per env, lane j =
// hidden unit j.  The recurrences themselves, Whh's LDS image and the reasons there is no
// workgroup barrier in the time loops are grucell.h's, shared with phases B and D of grugrad.hip;
// here are only the kernels' operands: gi / out / saved [4G] rows, and the hidden state a step
// started from re-derived from out[t - 1] (or hx0) and dones.  The results are the same bits on
// every call, at any N and at any position in the batch.
#include "grucell.h"

namespace dppo {
namespace {

constexpr int kThr = 256;

template <int G>
struct ScanLds {
  float W[3 * G * (G + 1)];  // Whh, row stride G + 1
  float x[3 * kThr];         // per env: h [G] (forward) or the gate deltas [3G] (backward)
};

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

// lane j of env n: sample i = t N + n
template <int G>
struct ScanFwdOps {
  const ScanFwdArgs& a;
  int64_t n;
  int j;
  __device__ __forceinline__ GruFwdIn in(int64_t t) const {
    const int64_t i = t * a.N + n;
    const float* gi = a.gi + i * (3 * G);
    return GruFwdIn{gi[j], gi[G + j], gi[2 * G + j], a.dones && a.dones[i] != 0};
  }
  __device__ __forceinline__ void store(int64_t t, float, float r, float z, float nn, float ghn,
                                        float hout) const {
    const int64_t i = t * a.N + n;
    a.out[i * G + j] = hout;
    if (a.saved) {
      float* sv = a.saved + i * (4 * G);
      sv[j] = r;
      sv[G + j] = z;
      sv[2 * G + j] = nn;
      sv[3 * G + j] = ghn;
    }
  }
};

template <int G>
__global__ __launch_bounds__(kThr) void gru_scan_fwd_kernel(ScanFwdArgs a) {
  constexpr int kEnvs = kThr / G;
  __shared__ __attribute__((aligned(16))) ScanLds<G> lds;
  const int tid = threadIdx.x;
  stage_whh<G, kThr>(lds.W, a.Whh, tid);
  __syncthreads();
  const int e = tid / G, j = tid % G;
  const int64_t n = (int64_t)blockIdx.x * kEnvs + e;
  if (n >= a.N) return;  // no workgroup barrier below
  gru_seq_fwd<G>(lds.W, a.bhh, lds.x + e * G, j, a.hx0[n * G + j], a.T, ScanFwdOps<G>{a, n, j});
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
struct ScanBwdOps {
  const ScanBwdArgs& a;
  int64_t n;
  int j;
  __device__ __forceinline__ GruBwdIn in(int64_t t) const {
    const int64_t i = t * a.N + n;
    const float* sv = a.saved + i * (4 * G);
    const bool done = a.dones && a.dones[i] != 0;
    // the hidden state the step started from, before the reset
    const float hprev = t > 0 ? a.out[(i - a.N) * G + j] : a.hx0[n * G + j];
    return GruBwdIn{a.dout[i * G + j], sv[j], sv[G + j], sv[2 * G + j], sv[3 * G + j],
                    done ? 0.0f : hprev, done};
  }
  __device__ __forceinline__ float* dgi(int64_t t) const { return a.dgi + (t * a.N + n) * (3 * G); }
  __device__ __forceinline__ float* dgh(int64_t t) const { return a.dgh + (t * a.N + n) * (3 * G); }
};

template <int G>
__global__ __launch_bounds__(kThr) void gru_scan_bwd_kernel(ScanBwdArgs a) {
  constexpr int kEnvs = kThr / G;
  __shared__ __attribute__((aligned(16))) ScanLds<G> lds;
  const int tid = threadIdx.x;
  stage_whh<G, kThr>(lds.W, a.Whh, tid);
  __syncthreads();
  const int e = tid / G, j = tid % G;
  const int64_t n = (int64_t)blockIdx.x * kEnvs + e;
  if (n >= a.N) return;  // no workgroup barrier below
  a.dh0[n * G + j] = gru_seq_bwd<G>(lds.W, lds.x + e * (3 * G), j,
                                    a.dhT ? a.dhT[n * G + j] : 0.0f, a.T, ScanBwdOps<G>{a, n, j});
}

// 0 when the geometry has no launch: unsupported G, T or N < 1, or more workgroups than a grid holds
int64_t scan_grid(int G, int64_t T, int64_t N) {
  if (!gru_width_ok(G) || T < 1 || N < 1) return 0;
  const int64_t envs = kThr / G;
  const int64_t grid = (N + envs - 1) / envs;
  return grid > 0x7FFFFFFF ? 0 : grid;
}

bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

int scan_check(const char* fn, int G, int64_t T, int64_t N) {
  if (!gru_width_ok(G)) {
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
  dispatch_gru_width(G, [&](auto g) {  // scan_check admitted G
    DPPO_LAUNCH(gru_scan_fwd_kernel<decltype(g)::value>, dim3(grid), dim3(kThr), 0, s, a);
  });
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
  dispatch_gru_width(G, [&](auto g) {  // scan_check admitted G
    DPPO_LAUNCH(gru_scan_bwd_kernel<decltype(g)::value>, dim3(grid), dim3(kThr), 0, s, a);
  });
  DPPO_LAUNCH_CHECK();
  return DPPO_OK;
}

}  // extern "C"
