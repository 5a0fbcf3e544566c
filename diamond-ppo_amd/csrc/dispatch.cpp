// Which fused kernel family runs for a shape: the tuned class (hidden 64, D <= 32) has the
// sample-split kernel (mbwave.hip) where that kernel's own predicate admits the shape and the
// two-team kernel (mbstep.hip) otherwise -- more actions, the fused Adam tail, DPPO_MB_LEGACY=1 --
// with mlp.hip's evaluation and actor; the wide class (hidden 128, or hidden 64 with
// 32 < D <= 128; hidden 64 also "large heads", D <= 384 and A <= 32, on one rank) has mbwide.hip
// for all three.  Host code only; the kernel files know nothing of each other.
#include "common.h"

namespace dppo {

bool tuned_shape(const MlpShape& sh) { return sh.H == 64 && sh.D <= 32 && sh.A <= 16; }

// Large heads: hidden 64 past either limit of the two classes above (Humanoid: 348 / 376 x 17).
// The kernels have no segment form for it: one rank only (dppo_create).
bool wide_large_shape(const MlpShape& sh) {
  if (sh.H != 64 || sh.A < 1 || sh.A > 32 || sh.D < 1 || sh.D > 384) return false;
  return sh.D > 128 || sh.A > 16;
}

bool wide_shape(const MlpShape& sh) {
  if (wide_large_shape(sh)) return true;
  if (sh.A < 1 || sh.A > 16 || sh.D < 1 || sh.D > 128) return false;
  return sh.H == 128 || (sh.H == 64 && sh.D > 32);
}

MbKernel pick_mb_kernel(const MlpShape& sh, bool fused_tail) {
  if (tuned_shape(sh)) return !fused_tail && mbw_supported(sh) ? MbKernel::Split : MbKernel::Team;
  return wide_shape(sh) ? MbKernel::Wide : MbKernel::None;
}

int fused_mb_grid(MbKernel k, const MlpShape& sh, int32_t m) {
  switch (k) {
    case MbKernel::Split: return mbw_grid(m);
    case MbKernel::Wide: return wide_grid(sh, m);
    default: return mb_grid(m);  // (None launches nothing: such a handle keeps this sizing)
  }
}

int launch_fused_mb(MbKernel k, const MlpShape& sh, const ParamOffsets& po, const GradArgs& a,
                    int G, hipStream_t s, const FusedAdam* fused) {
  if (fused && k != MbKernel::Team) {
    set_error("the fused Adam tail exists only for the tuned shape class");
    return DPPO_EUNSUPPORTED;
  }
  switch (k) {
    case MbKernel::Split: return launch_mbw(sh, po, a, G, s);
    case MbKernel::Team: return launch_mb(sh, po, a, G, s, fused);
    default: return launch_wide_mb(sh, po, a, G, s);  // (None: its own shape check reports it)
  }
}

int launch_fused_eval(const MlpShape& sh, const ParamOffsets& po, const float* params,
                      const float* obs, const void* actions, const float* next_obs, float* logp,
                      float* values, float* next_values, int64_t n, hipStream_t s,
                      EvalReuse* reuse) {
  if (tuned_shape(sh))
    return launch_eval(sh, po, params, obs, actions, next_obs, logp, values, next_values, n, s,
                       reuse);
  return launch_wide_eval(sh, po, params, obs, actions, next_obs, logp, values, next_values, n, s);
}

int launch_fused_act(const MlpShape& sh, const ParamOffsets& po, const float* params,
                     const float* obs, void* actions, int64_t n, uint64_t seed, uint64_t counter,
                     hipStream_t s, float* heads, const ActSquash* squash) {
  if (tuned_shape(sh))
    return launch_act(sh, po, params, obs, actions, n, seed, counter, s, heads, squash);
  return launch_wide_act(sh, po, params, obs, actions, n, seed, counter, s, heads, squash);
}

}  // namespace dppo
