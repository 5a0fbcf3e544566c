// RecurrentPPO fused kernels, host side: validation, the flat parameter layout, the handle and
// its workspace, the rollout kernels' timing pool and the C ABI (include/dppo.h).  The minibatch
// gradient kernel is grugrad.hip's, the rollout steps are gruact.hip's; both serve gru_hidden 16,
// 32 and 64 from one source each and are dispatched on G by their launchers.
#include <cstring>
#include <vector>

#include "grucell.h"

// ---------------------------------------------------------------------------------------------
// C ABI (include/dppo.h): handle = workspace for one rollout shape.
using namespace dppo;

struct dppo_gru_handle {
  int device = 0;
  bool gauss = false;     // the Gaussian head's layout and kernels (dppo_gru_gauss_create)
  int64_t ls_off = 0;     // actor_log_std in the Gaussian layout
  float* dls = nullptr;   // [B][16] per-sample log_std gradient rows (Gaussian)
  dppo_gru_dims dims{};
  dppo_layout layout{};
  GruOffsets po{};
  int64_t B = 0;
  int G = 1;
  int64_t slab_stride = 0;
  float* scratch = nullptr;  // one allocation, carved into GruScratch
  GruScratch sc{};
  float* wmask = nullptr;
  float* slabs = nullptr;
  double* sq_part = nullptr;
  // optional timing of the rollout kernels (dppo_gru_set_timing): event pairs per launch
  bool timing = false;
  std::vector<hipEvent_t> pool;
  size_t pool_used = 0;
  struct Rec {
    int cls;
    hipEvent_t a, b;
  };
  std::vector<Rec> recs;
};

namespace {

int gru_validate(const dppo_gru_dims* d) {
  if (!d || d->rollout_steps < 1 || d->num_envs < 1 || d->obs_dim < 1 || d->act_dim < 1 ||
      d->gru_hidden < 1) {
    set_error("invalid dppo_gru_dims");
    return DPPO_EINVAL;
  }
  if (d->hidden != kH || !gru_width_ok(d->gru_hidden) || d->obs_dim > (d->wide_obs ? 128 : 32) ||
      d->act_dim > kAPad) {
    set_error("fused GRU kernels support hidden=64, gru_hidden in {16, 32, 64}, obs_dim<=32 "
              "(<=128 with wide_obs), act_dim<=16 "
              "(got H=%d G=%d D=%d A=%d wide_obs=%d)", d->hidden, d->gru_hidden, d->obs_dim,
              d->act_dim, d->wide_obs);
    return DPPO_EUNSUPPORTED;
  }
  if ((int64_t)d->rollout_steps * d->num_envs > 0x7FFFFFFF / (4 * d->gru_hidden)) {
    set_error("T*N too large for the GRU workspace");
    return DPPO_EINVAL;
  }
  return DPPO_OK;
}

// gauss: RecurrentContinuousActorCriticNetwork's 15 tensors, actor_log_std [1][A] first
// (diamond/recurrent_continuous_ppo.py), then the same 14.
void gru_layout(const dppo_gru_dims* d, dppo_layout* L, bool gauss = false) {
  std::memset(L, 0, sizeof(*L));
  const int D = d->obs_dim, A = d->act_dim, G = d->gru_hidden;
  // RecurrentActorCriticNetwork.named_parameters() order (diamond/recurrent_ppo.py)
  const int rc[14][2] = {{kH, D}, {kH, 1}, {3 * G, kH}, {3 * G, G}, {3 * G, 1}, {3 * G, 1},
                         {kH, G}, {kH, 1}, {A, kH}, {A, 1}, {kH, G}, {kH, 1}, {1, kH}, {1, 1}};
  int64_t off = 0, real = 0;
  int c = 0;
  auto put = [&](int rows, int cols) {
    const int64_t ne = (int64_t)rows * cols;
    L->offset[c] = off;
    L->numel[c] = ne;
    L->rows[c] = rows;
    L->cols[c] = cols;
    off = (off + ne + 15) / 16 * 16;
    real += ne;
    ++c;
  };
  if (gauss) put(1, A);
  for (int i = 0; i < 14; ++i) put(rc[i][0], rc[i][1]);
  L->count = c;
  L->total = off;
  L->n_real = real;
}

int gru_layout_checked(const dppo_gru_dims* dims, dppo_layout* out, bool gauss) {
  if (!out) {
    set_error("out is NULL");
    return DPPO_EINVAL;
  }
  const int rc = gru_validate(dims);
  if (rc != DPPO_OK && rc != DPPO_EUNSUPPORTED) return rc;
  gru_layout(dims, out, gauss);
  return DPPO_OK;
}

int gru_plan(const dppo_gru_dims* dims, int32_t* out, bool gauss) {
  if (!out) {
    set_error("out is NULL");
    return DPPO_EINVAL;
  }
  const int rc = gru_validate(dims);
  if (rc != DPPO_OK) return rc;
  const int G = dims->gru_hidden;
  out[0] = gru_envs(G);
  out[1] = gru_grid(dims->num_envs, G);
  out[2] = (int32_t)(gauss ? gru_gauss_lds_bytes(dims->obs_dim, G)
                           : gru_lds_bytes(dims->obs_dim, G));
  out[3] = gru_act_envs();
  return DPPO_OK;
}

// A launch that belongs to the other head kind: DPPO_EINVAL, nothing launched.
int gru_kind_check(const dppo_gru_handle* h, bool gauss, const char* fn) {
  if (h->gauss == gauss) return DPPO_OK;
  set_error("%s: the handle was created for the %s head", fn,
            h->gauss ? "Gaussian (dppo_gru_gauss_create)" : "categorical (dppo_gru_create)");
  return DPPO_EINVAL;
}

// Hands the next launch of this thread an event pair of its own when the handle's timing is on
// (g_launch_timing, common.h); otherwise does nothing.
struct GruTimed {
  dppo_gru_handle* h;
  GruTimed(dppo_gru_handle* h_, int cls) : h(h_) {
    if (!h->timing) return;
    while (h->pool.size() < h->pool_used + 2) {
      hipEvent_t e = nullptr;
      if (hipEventCreate(&e) != hipSuccess) return;
      h->pool.push_back(e);
    }
    const hipEvent_t a = h->pool[h->pool_used], b = h->pool[h->pool_used + 1];
    h->pool_used += 2;
    g_launch_timing.start = a;
    g_launch_timing.stop = b;
    h->recs.push_back({cls, a, b});
  }
  ~GruTimed() {
    if (!g_launch_timing.stop) return;
    if (g_launch_timing.start) h->recs.pop_back();  // nothing was launched
    g_launch_timing = LaunchTiming{};
  }
};

}  // namespace

extern "C" {

int dppo_gru_param_layout(const dppo_gru_dims* dims, dppo_layout* out) {
  return gru_layout_checked(dims, out, false);
}

int dppo_gru_gauss_param_layout(const dppo_gru_dims* dims, dppo_layout* out) {
  return gru_layout_checked(dims, out, true);
}

void dppo_gru_destroy(dppo_gru_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  (void)hipFree(h->scratch);
  (void)hipFree(h->wmask);
  (void)hipFree(h->slabs);
  (void)hipFree(h->sq_part);
  (void)hipFree(h->dls);
  for (hipEvent_t e : h->pool) (void)hipEventDestroy(e);
  delete h;
}

}  // extern "C"

namespace {

int gru_create(int device, const dppo_gru_dims* dims, bool gauss, dppo_gru_handle** out) {
  if (!out) {
    set_error("out is NULL");
    return DPPO_EINVAL;
  }
  *out = nullptr;
  const int rc = gru_validate(dims);
  if (rc != DPPO_OK) return rc;
  DPPO_HIP_CHECK(hipSetDevice(device));
  dppo_gru_handle* h = new dppo_gru_handle();
  h->device = device;
  h->dims = *dims;
  h->gauss = gauss;
  gru_layout(dims, &h->layout, gauss);
  h->ls_off = h->layout.offset[0];
  const int64_t* o = h->layout.offset + (gauss ? 1 : 0);
  h->po = GruOffsets{o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], o[8], o[9], o[10], o[11],
                     o[12], o[13]};
  h->B = (int64_t)dims->rollout_steps * dims->num_envs;
  const int G = dims->gru_hidden;
  h->G = gru_grid(dims->num_envs, G);
  h->slab_stride = (h->layout.total + 8 + 63) / 64 * 64;
  const int D16 = (dims->obs_dim + 15) / 16 * 16;
  // per-sample rows: obs D16 | x1 64 | gi 3G | hi ho r z n ghn 6xG | ya yc 2x64 | dl dv 2x16 |
  // dya dyc 2x64 | dho G | dgi dgh 2x3G | dx1 64
  const int64_t row = D16 + kH + 3 * G + 6 * G + 2 * kH + 2 * kAPad + 2 * kH + G + 6 * G + kH;
  hipError_t e = hipMalloc((void**)&h->scratch, (size_t)(h->B * row) * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&h->wmask, (size_t)h->B * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&h->slabs, (size_t)(h->G * h->slab_stride) * sizeof(float));
  if (e == hipSuccess)
    e = hipMalloc((void**)&h->sq_part, (size_t)slab_reduce_blocks(h->layout.total) * sizeof(double));
  if (e == hipSuccess && gauss)
    e = hipMalloc((void**)&h->dls, (size_t)(h->B * kAPad) * sizeof(float));
  if (e != hipSuccess) {
    set_error("hipMalloc (GRU workspace) failed: %s", hipGetErrorString(e));
    dppo_gru_destroy(h);
    return DPPO_ENOMEM;
  }
  // the kernel never writes the layout's padding floats or the unused loss slots
  (void)hipMemset(h->slabs, 0, (size_t)(h->G * h->slab_stride) * sizeof(float));
  float* p = h->scratch;
  auto take = [&](int64_t w) {
    float* q = p;
    p += h->B * w;
    return q;
  };
  GruScratch& sc = h->sc;
  sc.obs = take(D16);
  sc.x1 = take(kH);
  sc.gi = take(3 * G);
  sc.hi = take(G);
  sc.ho = take(G);
  sc.r = take(G);
  sc.z = take(G);
  sc.n = take(G);
  sc.ghn = take(G);
  sc.ya = take(kH);
  sc.yc = take(kH);
  sc.dl = take(kAPad);
  sc.dv = take(kAPad);
  sc.dya = take(kH);
  sc.dyc = take(kH);
  sc.dho = take(G);
  sc.dgi = take(3 * G);
  sc.dgh = take(3 * G);
  sc.dx1 = take(kH);
  *out = h;
  return DPPO_OK;
}

}  // namespace

extern "C" {

int dppo_gru_create(int device, const dppo_gru_dims* dims, dppo_gru_handle** out) {
  return gru_create(device, dims, false, out);
}

int dppo_gru_gauss_create(int device, const dppo_gru_dims* dims, dppo_gru_handle** out) {
  return gru_create(device, dims, true, out);
}

int dppo_gru_minibatch_grad_f32(dppo_gru_handle* h, const float* params,
                                const dppo_gru_batch* batch, const int32_t* idx, int32_t m,
                                int32_t m_total, const dppo_hparams* hp, float* grad,
                                void* stream) {
  if (!h || !params || !batch || !idx || !hp || !grad || m < 0 || m_total <= 0 ||
      m > h->B || !batch->obs || !batch->actions || !batch->old_log_probs || !batch->advantages ||
      !batch->returns || !batch->prev_dones || !batch->hx0) {
    set_error("invalid argument to dppo_gru_minibatch_grad_f32");
    return DPPO_EINVAL;
  }
  if ((uintptr_t)params % 16 != 0) {
    set_error("dppo_gru_minibatch_grad_f32: params must be 16-byte aligned");
    return DPPO_EINVAL;
  }
  if (gru_kind_check(h, false, "dppo_gru_minibatch_grad_f32") != DPPO_OK) return DPPO_EINVAL;
  DPPO_HIP_CHECK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const dppo_gru_dims& d = h->dims;
  int rc = launch_gru_grad(d.gru_hidden, h->po, params, *batch, idx, m, h->wmask, h->B,
                           d.rollout_steps, d.num_envs, d.obs_dim, d.act_dim,
                           (float)(1.0 / (double)m_total), hp->ppo_clip, hp->value_loss_weight,
                           hp->entropy_beta, h->sc, h->slabs, h->slab_stride, h->layout.total, s);
  if (rc != DPPO_OK) return rc;
  return launch_slab_reduce(h->slabs, h->G, h->slab_stride, h->layout.total, grad, h->sq_part,
                            LogStdTerm{-1, 0, 0.0f, 0}, s);
}

int dppo_gru_gauss_minibatch_grad_f32(dppo_gru_handle* h, const float* params,
                                      const dppo_gru_gauss_batch* batch, const int32_t* idx,
                                      int32_t m, int32_t m_total, const dppo_hparams* hp,
                                      float* grad, void* stream) {
  if (!h || !params || !batch || !idx || !hp || !grad || m < 0 || m_total <= 0 ||
      m > h->B || !batch->obs || !batch->actions || !batch->old_log_probs || !batch->advantages ||
      !batch->returns || !batch->prev_dones || !batch->hx0) {
    set_error("invalid argument to dppo_gru_gauss_minibatch_grad_f32");
    return DPPO_EINVAL;
  }
  if ((uintptr_t)params % 16 != 0) {
    set_error("dppo_gru_gauss_minibatch_grad_f32: params must be 16-byte aligned");
    return DPPO_EINVAL;
  }
  if (gru_kind_check(h, true, "dppo_gru_gauss_minibatch_grad_f32") != DPPO_OK) return DPPO_EINVAL;
  DPPO_HIP_CHECK(hipSetDevice(h->device));
  hipStream_t s = (hipStream_t)stream;
  const dppo_gru_dims& d = h->dims;
  int rc = launch_gru_gauss_grad(d.gru_hidden, h->po, h->ls_off, params, *batch, idx, m, h->wmask,
                                 h->B, d.rollout_steps, d.num_envs, d.obs_dim, d.act_dim,
                                 (float)(1.0 / (double)m_total), hp->ppo_clip,
                                 hp->value_loss_weight, hp->entropy_beta, h->sc, h->dls, h->slabs,
                                 h->slab_stride, h->layout.total, s);
  if (rc != DPPO_OK) return rc;
  // the entropy bonus's log_std term is in the slabs already (grugrad.hip phase C)
  return launch_slab_reduce(h->slabs, h->G, h->slab_stride, h->layout.total, grad, h->sq_part,
                            LogStdTerm{-1, 0, 0.0f, 0}, s);
}

int dppo_gru_act_f32(dppo_gru_handle* h, const float* params, const dppo_gru_step* step,
                     int64_t n, uint64_t seed, uint64_t counter, void* stream) {
  if (!h || !params || !step || n < 0 || !step->obs || !step->prev_dones || !step->hx ||
      !step->hx_out || !step->actions || !step->log_probs || !step->values ||
      step->hx_out == step->hx || (uintptr_t)params % 16 != 0) {
    set_error("invalid argument to dppo_gru_act_f32 (NULL pointer, n < 0, hx_out == hx or "
              "params not 16-byte aligned)");
    return DPPO_EINVAL;
  }
  if (gru_kind_check(h, false, "dppo_gru_act_f32") != DPPO_OK) return DPPO_EINVAL;
  if (n == 0) return DPPO_OK;
  DPPO_HIP_CHECK(hipSetDevice(h->device));
  GruTimed timed(h, 0);
  return launch_gru_act(h->dims.gru_hidden, h->po, params, *step, n, h->dims.obs_dim,
                        h->dims.act_dim, seed, counter, (hipStream_t)stream);
}

int dppo_gru_gauss_act_f32(dppo_gru_handle* h, const float* params,
                           const dppo_gru_gauss_step* step, int64_t n, uint64_t seed,
                           uint64_t counter, void* stream) {
  if (!h || !params || !step || n < 0 || !step->obs || !step->prev_dones || !step->hx ||
      !step->hx_out || !step->actions || !step->log_probs || !step->values ||
      step->hx_out == step->hx || (uintptr_t)params % 16 != 0) {
    set_error("invalid argument to dppo_gru_gauss_act_f32 (NULL pointer, n < 0, hx_out == hx or "
              "params not 16-byte aligned)");
    return DPPO_EINVAL;
  }
  if (gru_kind_check(h, true, "dppo_gru_gauss_act_f32") != DPPO_OK) return DPPO_EINVAL;
  if (n == 0) return DPPO_OK;
  DPPO_HIP_CHECK(hipSetDevice(h->device));
  GruTimed timed(h, 0);
  return launch_gru_gauss_act(h->dims.gru_hidden, h->po, h->ls_off, params, *step, n,
                              h->dims.obs_dim, h->dims.act_dim, seed, counter,
                              (hipStream_t)stream);
}

int dppo_gru_value_f32(dppo_gru_handle* h, const float* params, const float* obs,
                       const float* hx, const uint8_t* dones, int64_t n, float* values,
                       void* stream) {
  if (!h || !params || !obs || !hx || !values || n < 0 || (uintptr_t)params % 16 != 0) {
    set_error("invalid argument to dppo_gru_value_f32 (NULL pointer, n < 0 or params not "
              "16-byte aligned)");
    return DPPO_EINVAL;
  }
  if (n == 0) return DPPO_OK;
  DPPO_HIP_CHECK(hipSetDevice(h->device));
  GruTimed timed(h, 1);
  return launch_gru_value(h->dims.gru_hidden, h->po, params, obs, hx, dones, n, h->dims.obs_dim,
                          values, (hipStream_t)stream);
}

int dppo_gru_plan(const dppo_gru_dims* dims, int32_t* out) { return gru_plan(dims, out, false); }

int dppo_gru_gauss_plan(const dppo_gru_dims* dims, int32_t* out) {
  return gru_plan(dims, out, true);
}

int dppo_gru_set_timing(dppo_gru_handle* h, int32_t enable) {
  if (!h) {
    set_error("null handle");
    return DPPO_EINVAL;
  }
  DPPO_HIP_CHECK(hipSetDevice(h->device));
  DPPO_HIP_CHECK(hipDeviceSynchronize());
  h->timing = enable != 0;
  h->recs.clear();
  h->pool_used = 0;
  return DPPO_OK;
}

int dppo_gru_get_timing(dppo_gru_handle* h, double* ms_sum, int64_t* counts) {
  if (!h || !ms_sum || !counts) {
    set_error("null argument to dppo_gru_get_timing");
    return DPPO_EINVAL;
  }
  DPPO_HIP_CHECK(hipSetDevice(h->device));
  for (int k = 0; k < DPPO_GRU_TIMING_CLASSES; ++k) {
    ms_sum[k] = 0.0;
    counts[k] = 0;
  }
  for (const auto& r : h->recs) {
    DPPO_HIP_CHECK(hipEventSynchronize(r.b));
    float ms = 0.f;
    DPPO_HIP_CHECK(hipEventElapsedTime(&ms, r.a, r.b));
    ms_sum[r.cls] += ms;
    counts[r.cls] += 1;
  }
  return DPPO_OK;
}

}  // extern "C"
