"""Shared helpers of the GPU test modules (synthetic rollouts, random default-network parameters,
C-ABI hyper-parameters, the near-regime element bound, the off-policy minibatch recipe).  Test
infrastructure only.  Nothing here
touches the GPU at import; synth_host, random_params and offpolicy_inputs are NumPy plus the oracle
and also run in the CPU suite."""
import numpy as np
import torch

from diamond import _native as N
from diamond.engine import DeviceRollout
from oracle import ppo_np as P

H = 64


def dev():
    return torch.device("cuda", 0)


def stream():
    return torch.cuda.current_stream().cuda_stream


class Box:
    def __init__(self, shape):
        self.shape = tuple(shape)


class Discrete:
    def __init__(self, n):
        self.n = int(n)


class SpecEnvs:
    """Spaces only: learn() on staged buffers never steps an environment."""

    def __init__(self, D, A, cont):
        self.single_observation_space = Box((D,))
        self.single_action_space = Box((A,)) if cont else Discrete(A)


def synth_host(T, Nn, D, A, cont, seed, reward_mean=1.0):
    """The host arrays of synth(): (obs, next_obs, actions, rewards, term, trunc)."""
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((T, Nn, D), dtype=np.float32)
    nobs = rng.standard_normal((T, Nn, D), dtype=np.float32)
    act = (rng.standard_normal((T, Nn, A), dtype=np.float32) if cont
           else rng.integers(0, A, (T, Nn)).astype(np.int32))
    rew = rng.normal(reward_mean, 1.0, (T, Nn)).astype(np.float32)
    te = (rng.random((T, Nn)) < (0.0 if cont else 0.02)).astype(np.uint8)
    tr = (rng.random((T, Nn)) < (0.001 if cont else 0.005)).astype(np.uint8)
    return obs, nobs, act, rew, te, tr


def to_device(host):
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev())
    return DeviceRollout(*[g(x) for x in host])


def synth(T, Nn, D, A, cont, seed):
    host = synth_host(T, Nn, D, A, cont, seed)
    return to_device(host), host


def random_params(L, names, D, A, cont, rng):
    """Parameters of the default network at a scale that keeps tanh units in their active range
    and the policy away from uniform (so the surrogate's clip and both tie branches occur)."""
    params = {}
    for i, n in enumerate(names):
        shp = (L.rows[i],) if n.endswith("bias") else (L.rows[i], L.cols[i])
        if n == "actor_log_std":
            params[n] = rng.normal(-0.5, 0.2, (1, A)).astype(np.float32)
        elif n.endswith("bias"):
            params[n] = rng.normal(0.0, 0.1, shp).astype(np.float32)
        else:
            params[n] = (rng.standard_normal(shp) * 1.2 / np.sqrt(shp[1])).astype(np.float32)
    flat = np.zeros(L.total, np.float32)
    for i, n in enumerate(names):
        flat[L.offset[i]:L.offset[i] + L.numel[i]] = params[n].ravel()
    return params, flat


def _figures(got, exact, o32):
    """Of |got - exact| <= 2e-5 max(1, |exact|) + 4 |oracle32 - exact| per element: (max |got -
    exact|, max |oracle32 - exact|, elements beyond the bound, largest excess over it)."""
    exact = np.asarray(exact, np.float64)
    d32 = np.abs(np.asarray(o32, np.float64) - exact)
    tol = 2e-5 * np.maximum(1.0, np.abs(exact)) + 4 * d32
    d = np.abs(np.asarray(got, np.float64) - exact)
    return float(d.max()), float(d32.max()), int((d > tol).sum()), float((d - tol).max())


def _within(got, exact, o32, what):
    figs = _figures(got, exact, o32)
    assert np.isfinite(got).all(), what
    assert figs[2] == 0, (what, figs)
    return figs[:2]


def hparams(**over):
    kw = dict(gamma=0.99, gae_lambda=0.95, ppo_clip=0.2, value_loss_weight=1.0,
              entropy_beta=0.01, grad_norm_clip=0.5, adam_beta1=0.9, adam_beta2=0.999,
              adam_eps=1e-5, advantage_norm=1, lr=3e-4, adam_step=0)
    kw.update(over)
    return N.HParams(**kw)


def nit_of(m):
    """32-sample steps per workgroup of the two-team kernel (mbstep.hip)."""
    steps = (m + 31) // 32
    G = min(steps, 256)
    return (steps + G - 1) // G


def sample_split(D, A, cont):
    """Whether learn() runs the sample-split kernel (mbwave.hip, mbw_supported) for this shape."""
    if cont and 5 <= A <= 6 and D == 17:
        return True  # the X1 instantiation (HalfCheetah)
    return D <= 32 and (A <= 4 or (A <= 8 and not cont and D <= 16))


def groups_per_wave(m):
    """16-sample groups each wave of the sample-split kernel runs (4 waves per workgroup, one
    workgroup per 64 samples up to 256)."""
    groups = (m + 15) // 16
    G = min((m + 63) // 64, 256)
    return (groups + 4 * G - 1) // (4 * G)


def production_depth(m, D, A, cont):
    return groups_per_wave(m) if sample_split(D, A, cont) else nit_of(m)


# ---------------------------------------------------------------------------------------------
# Off-policy minibatches: the gradient is taken at parameters other than the ones that produced
# the old log-probs, so every branch of the clipped surrogate (ppo.py:266-270) carries samples.
# ---------------------------------------------------------------------------------------------
OFFPOLICY_HYPER = {
    "clip.1": dict(ppo_clip=0.1, value_loss_weight=0.5, entropy_beta=0.05, advantage_norm=False),
    "clip.3": dict(ppo_clip=0.3, value_loss_weight=2.0, entropy_beta=0.0, advantage_norm=True),
}

REGIMES = ("in range", "above, adv > 0 (clipped)", "above, adv < 0 (passes)",
           "below, adv > 0 (passes)", "below, adv < 0 (clipped)")
NEAR_BOUND = 1e-3         # a float32 kernel may land on the other side of a bound this close
RATIO_RANGE = (1 / 16, 16)  # a few huge ratios would dominate the float32 loss sum
MAX_EXCLUDED = 0.05       # of the batch
MIN_REGIME = 0.05         # of the minibatch


def surrogate_regimes(ratio, adv, eps, near_bound=NEAR_BOUND):
    """Regime index (into REGIMES) of every sample; -1 where the sample is excluded: ratio within
    near_bound of 1 - eps or 1 + eps, or outside RATIO_RANGE."""
    ratio = np.asarray(ratio, np.float64)
    adv = np.asarray(adv, np.float64)
    lo, hi = 1.0 - eps, 1.0 + eps
    reg = np.zeros(ratio.shape, np.int64)
    reg[(ratio > hi) & (adv > 0)] = 1
    reg[(ratio > hi) & (adv <= 0)] = 2
    reg[(ratio < lo) & (adv > 0)] = 3
    reg[(ratio < lo) & (adv <= 0)] = 4
    near = (np.abs(ratio - lo) <= near_bound) | (np.abs(ratio - hi) <= near_bound)
    far = (ratio < RATIO_RANGE[0]) | (ratio > RATIO_RANGE[1])
    reg[near | far] = -1
    return reg, float(near.mean()), float(far.mean())


def perturbed_params(L, names, old, s, rng):
    """old + noise scaled like random_params' own draw: weights s * 1.2 / sqrt(fan_in), biases
    0.1 * s, actor_log_std s."""
    new = {}
    for n in names:
        shp = old[n].shape
        if n == "actor_log_std":
            k = s
        elif n.endswith("bias"):
            k = 0.1 * s
        else:
            k = s * 1.2 / np.sqrt(shp[1])
        new[n] = (old[n] + k * rng.standard_normal(shp)).astype(np.float32)
    flat = np.zeros(L.total, np.float32)
    for i, n in enumerate(names):
        flat[L.offset[i]:L.offset[i] + L.numel[i]] = new[n].ravel()
    return new, flat


def new_policy_logp64(params, obs, act, cont):
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    f = P.forward(p64, obs, cont, np.float64)
    if cont:
        return P.normal_logp_entropy(f["out"], p64["actor_log_std"], act, np.float64)[0]
    return P.categorical_logp_entropy(f["out"], act, np.float64)[0]


def flat32(L, names, params):
    """The parameters in the library's flat float32 layout."""
    flat = np.zeros(L.total, np.float32)
    for i, n in enumerate(names):
        flat[L.offset[i]:L.offset[i] + L.numel[i]] = params[n].ravel()
    return flat


def offpolicy_inputs(L, names, D, A, cont, T, Nn, m, hyper, s, seed, transform=None):
    """Old and new parameters, a rollout and a stratified minibatch index list for one off-policy
    gradient check.  Everything is the oracle's: old log-probs, values, GAE and (if
    hyper.advantage_norm) the normalised advantages in float32 as learn() computes them, the
    ratio exp(logp_new - logp_old) with the new log-prob in float64.  idx takes up to m / 5
    samples of each regime, then fills at random, never from the excluded samples.
    ``transform(params, obs, next_obs, actions, rewards)`` (tests/regime_cases.py) moves the old
    parameters and the rollout into a numerical regime before the new parameters are drawn."""
    B = T * Nn
    rng = np.random.default_rng(1000 + seed)
    old, old_flat = random_params(L, names, D, A, cont, rng)
    host = synth_host(T, Nn, D, A, cont, 2000 + seed,
                      reward_mean=1.0 if hyper.advantage_norm else 0.0)
    if transform is not None:
        old, *data = transform(old, *host[:4])
        old_flat, host = flat32(L, names, old), (*data, *host[4:])
    new, new_flat = perturbed_params(L, names, old, s, rng)
    obs, nobs, act, rew, te, tr = host
    logp_old, v, nv, _ = P.old_policy(old, obs, act, nobs, cont)
    adv = P.gae(rew, te, tr, v, nv, hyper.gamma, hyper.gae_lambda)
    ret = v + adv
    if hyper.advantage_norm:
        adv = P.normalize_adv(adv)
    obs_f = obs.reshape(B, D)
    act_f = act.reshape(B, A) if cont else act.reshape(B)
    ratio = np.exp(new_policy_logp64(new, obs_f, act_f, cont) - logp_old.ravel())
    reg, near, far = surrogate_regimes(ratio, adv.ravel(), hyper.ppo_clip)
    pick = np.random.default_rng(3000 + seed)
    chosen = [pick.permutation(np.flatnonzero(reg == k))[:m // 5] for k in range(5)]
    chosen = np.concatenate(chosen)
    rest = np.setdiff1d(np.flatnonzero(reg >= 0), chosen)
    fill = pick.permutation(rest)[:m - chosen.size]
    idx = pick.permutation(np.concatenate([chosen, fill])).astype(np.int32)
    batch_share = [float((reg == k).mean()) for k in range(5)]
    return dict(old=old, old_flat=old_flat, new=new, new_flat=new_flat, host=host, idx=idx,
                obs=obs_f, act=act_f, logp_old=logp_old.ravel(), adv=adv.ravel(),
                ret=ret.ravel(), ratio=ratio, regime=reg, near=near, far=far,
                batch_share=batch_share)


def check_offpolicy_conditions(regime_of_idx, m, near, far):
    """The conditions that keep an off-policy case from being vacuous (asserted by the CPU and
    the GPU module): a full minibatch without excluded samples, every regime with its share, and
    the exclusions small."""
    assert regime_of_idx.size == m, (regime_of_idx.size, m)
    assert (regime_of_idx >= 0).all()
    assert near + far <= MAX_EXCLUDED, (near, far)
    share = [float((regime_of_idx == k).mean()) for k in range(5)]
    assert min(share) >= MIN_REGIME, dict(zip(REGIMES, share))
    return share


def gradient_errors(L, names, got, grads):
    """(overall error / max|g|, {tensor: error / max(own scale, 1e-3 max|g|)}) of a flat-layout
    gradient against the oracle's dict."""
    exact = np.concatenate([np.asarray(grads[n], np.float64).ravel() for n in names])
    got = np.concatenate([np.asarray(got[L.offset[k]:L.offset[k] + L.numel[k]], np.float64)
                          for k in range(L.count)])
    scale = np.abs(exact).max()
    per, o = {}, 0
    for k, n in enumerate(names):
        a, b = got[o:o + L.numel[k]], exact[o:o + L.numel[k]]
        o += L.numel[k]
        per[n] = np.abs(a - b).max() / max(np.abs(b).max(), 1e-3 * scale)
    return np.abs(got - exact).max() / scale, per


def flat_of(L, names, grads):
    flat = np.zeros(L.total, np.float64)
    for i, n in enumerate(names):
        flat[L.offset[i]:L.offset[i] + L.numel[i]] = np.asarray(grads[n]).ravel()
    return flat


# (family, hidden, D, A, Gaussian head, num_envs, {hyper set: noise scale s}, also with m_total != m)
OFFPOLICY_SHAPES = [
    ("sample-split", 64, 8, 4, False, 96, {"clip.1": 0.2, "clip.3": 0.2}, True),
    # one action, three inputs: at s = 0.1 ratios past 16 exceed the exclusion allowance under
    # clip 0.1, and below 0.07 the two below-range regimes starve under clip 0.3
    ("sample-split", 64, 3, 1, True, 96, {"clip.1": 0.05, "clip.3": 0.08}, True),
    ("sample-split", 64, 16, 8, False, 96, {"clip.1": 0.2, "clip.3": 0.2}, False),
    ("sample-split", 64, 17, 6, True, 96, {"clip.1": 0.03, "clip.3": 0.03}, False),
    ("two-team", 64, 32, 16, False, 96, {"clip.1": 0.2, "clip.3": 0.2}, True),
    ("two-team", 64, 5, 10, True, 96, {"clip.1": 0.03, "clip.3": 0.03}, True),
    ("wide", 128, 8, 4, False, 96, {"clip.1": 0.2, "clip.3": 0.2}, True),
    ("wide", 128, 105, 8, True, 96, {"clip.1": 0.03, "clip.3": 0.03}, True),
    ("wide", 128, 128, 16, False, 96, {"clip.1": 0.2, "clip.3": 0.2}, False),
    ("wide", 128, 30, 1, True, 96, {"clip.1": 0.1, "clip.3": 0.1}, False),
    ("wide", 64, 40, 5, False, 96, {"clip.1": 0.2, "clip.3": 0.2}, False),
    ("wide", 64, 128, 16, True, 96, {"clip.1": 0.03, "clip.3": 0.03}, False),
    # the other four reachable wide_mb_kernel<H, CONT, NB1> (tests/wide_mb_cases.py INSTANTIATIONS).
    # Three Gaussian actions starve the below-range regimes under clip 0.3 at s = 0.02 (and nearly
    # at 0.03); eleven put more than 5 % of the ratios past 16 at s = 0.05 under clip 0.1
    ("wide", 128, 50, 7, False, 96, {"clip.1": 0.2, "clip.3": 0.2}, False),
    ("wide", 128, 33, 3, True, 96, {"clip.1": 0.05, "clip.3": 0.05}, False),
    ("wide", 64, 128, 16, False, 96, {"clip.1": 0.2, "clip.3": 0.2}, False),
    ("wide", 64, 57, 11, True, 96, {"clip.1": 0.02, "clip.3": 0.02}, False),
]
OFFPOLICY_T, OFFPOLICY_M, OFFPOLICY_RAGGED = 16, 4, 5


def offpolicy_cases():
    """(id, seed, family, hidden, D, A, cont, Nn, hyper key, s, m_total is 2m + 3)"""
    out = []
    for j, (fam, Hd, D, A, cont, Nn, noise, scaled) in enumerate(OFFPOLICY_SHAPES):
        for k, key in enumerate(OFFPOLICY_HYPER):
            for sc in ((False, True) if scaled else (False,)):
                name = f"{fam}-H{Hd}-D{D}-A{A}-{'gauss' if cont else 'cat'}-{key}" + \
                       ("-mtotal" if sc else "")
                out.append((name, 10 * j + k, fam, Hd, D, A, cont, Nn, key, noise[key], sc))
    return out


def offpolicy_hyper(key):
    return P.Hyper(**OFFPOLICY_HYPER[key])
