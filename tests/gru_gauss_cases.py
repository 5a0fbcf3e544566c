"""Inputs of the Gaussian GRU minibatch kernel's cases (tests/test_gpu_gru_gauss.py;
csrc/grugrad.hip's gru_grad_kernel<G, WIDE_OBS, true> behind dppo_gru_gauss_minibatch_grad_f32),
built on the CPU so every case's clip-regime guards can be evaluated with the float64 oracle alone
(tests/test_gru_gauss_cpu.py) before the kernel runs them.  Test infrastructure only.

The recipe is tests/gru_cases.py's (initial weights + 0.3 N(0, 1); observations, advantages,
returns, dones and hx0 of gru_cases.data at seed T * 100 + N + seed_shift) with what a Gaussian
head needs in place of the categorical columns:
  actor_log_std  zeros (the init, regime "zero"), or uniform in [-1.5, 0.5] per dimension
                 (regime "spread": at sigma = 1 every exp(-log_std) factor is 1 and a wrong power
                 of sigma would pass);
  actions        float32 [T, N, A]: the oracle's mean + sigma * eps, eps ~ N(0, 1), or with
                 ``tail`` eps = +-4 (the project's "tail actions" regime);
  old_log_probs  on-policy: the oracle's own log-probs in float32.  Off-policy: those plus
                 OLD_NOISE * N(0, 1) (the case's old_noise where it has one: the wider clip of
                 the hyperparameter case needs a wider spread), so the log-ratio's spread is
                 the same at every A (a perturbation of the weights would spread the joint
                 log-ratio with A) and both sides of the clip are populated.
Per G, with E = 256 / G envs per workgroup, the shapes (T, N, D, A) are those of ``shapes``.
``SEED_SHIFT`` moves a case's seed where the guards of gru_cases.guards fail at 0."""
from dataclasses import dataclass, replace

import numpy as np
import torch

import gru_cases
import gru_gauss_oracle as GO
from gru_wide_cases import ENVS_PER_WG

WIDTHS = (16, 32, 64)
OLD_NOISE = 0.3
REGIMES = ("zero", "spread")
_x = lambda s: "x".join(map(str, s))


@dataclass(frozen=True)
class Case(gru_cases.Case):
    G: int = 16
    regime: str = "zero"     # actor_log_std: zero | spread
    tail: bool = False       # actions 4 sigma from the mean
    wide_obs: bool = False

    def __str__(self):
        return f"g{self.G}-{self.regime}-{self.name}"


def shapes(G):
    E = ENVS_PER_WG[G]
    return [(5, 3, 4, 1), (7, E + 1, 8, 3), (3, 5, 5, 6), (6, 2 * E + 1, 17, 6), (4, 9, 32, 16)]


WIDE_SHAPE = (3, 5, 65, 4)
TAIL_SHAPE = (3, 5, 5, 6)


def _cases(G, regime):
    sh = shapes(G)
    mk = lambda name, s, **kw: Case(name, s, G=G, regime=regime, **kw)
    return ([mk(f"{_x(s)}-{f}", s, frac=f) for s in sh for f in (1.0, 0.4)]
            + [mk(f"wide-{_x(WIDE_SHAPE)}-{f}", WIDE_SHAPE, frac=f, wide_obs=True)
               for f in (1.0, 0.4)]
            + [mk(f"onpolicy-{_x(s)}", s, on_policy=True) for s in (sh[1], sh[4])]
            + [mk(f"tail-{_x(TAIL_SHAPE)}", TAIL_SHAPE, tail=True)])


def _further(G):
    s2, s4 = shapes(G)[1], shapes(G)[3]
    mk = lambda name, s, **kw: Case(name, s, G=G, regime="spread", **kw)
    return ([mk(f"mtotal2-{_x(s2)}", s2, frac=0.4, m_total_mul=2),
             mk(f"hyper-{_x(s2)}", s2, clip=0.3, vf=0.5, ent=0.05, old_noise=0.5)]
            + [mk(f"dones-{d}-{_x(s4)}", s4, dones=d) for d in ("env_always", "last")])


# (G, regime, case name) -> seed_shift, where the guards fail at 0
# (the share of clipped samples among the 36 / 63 / 119 selected falls below 20 % there)
SEED_SHIFT = {(16, "zero", "4x9x32x16-1.0"): 1, (16, "spread", "4x9x32x16-1.0"): 1,
              (16, "spread", "hyper-7x17x8x3"): 1, (32, "zero", "7x9x8x3-1.0"): 2,
              (32, "zero", "4x9x32x16-1.0"): 1, (32, "spread", "7x9x8x3-1.0"): 2,
              (32, "spread", "4x9x32x16-1.0"): 1, (64, "zero", "4x9x32x16-1.0"): 1,
              (64, "spread", "4x9x32x16-1.0"): 1}

CASES = [replace(c, seed_shift=SEED_SHIFT.get((c.G, c.regime, c.name), 0))
         for G in WIDTHS for c in ([c for r in REGIMES for c in _cases(G, r)] + _further(G))]


def config(G, **kw):
    from diamond.recurrent_continuous_ppo import RecurrentContinuousPPOConfig
    return RecurrentContinuousPPOConfig(gru_hidden_dim=G, **kw)


def network(D, A, G, seed=42):
    """RecurrentContinuousPPO's network with its initial weights, built on the CPU."""
    import gym_stub
    from math import sqrt
    from diamond.continuous_ppo import network_parameter_init_
    from diamond.recurrent_continuous_ppo import RecurrentContinuousActorCriticNetwork
    torch.manual_seed(seed)
    net = RecurrentContinuousActorCriticNetwork(gym_stub.Box(shape=(D,)), gym_stub.Box(shape=(A,)),
                                                cfg=config(G))
    network_parameter_init_(net, gain=sqrt(2.0))
    return net


def initial_params(D, A, G, seed=42):
    p = {n: t.detach().numpy().copy() for n, t in network(D, A, G, seed).named_parameters()}
    assert list(p) == GO.PARAM_NAMES
    return p


def log_std(A, regime, seed):
    if regime == "zero":
        return np.zeros((1, A), np.float32)
    assert regime == "spread"
    return np.random.default_rng(seed + 3).uniform(-1.5, 0.5, (1, A)).astype(np.float32)


def build(case):
    """(params, data dict, mb_idx int32, m_total) of one case."""
    T, Nn, D, A = case.shape
    seed = T * 100 + Nn + case.seed_shift
    rng = np.random.default_rng(seed + 1)
    params = {n: (p + 0.3 * rng.standard_normal(p.shape)).astype(np.float32)
              for n, p in initial_params(D, A, case.G).items()}
    params["actor_log_std"] = log_std(A, case.regime, seed)
    x = gru_cases.data(T, Nn, D, 2, seed, G=case.G)
    pd = x["prev_dones"]
    if case.dones == "env_always":
        pd[:, min(gru_cases.DONE_ENV, Nn - 1)] = True
    elif case.dones == "last":
        pd[:] = False
        pd[T - 1] = True
    else:
        assert case.dones == "random"
    mean, _ = GO.forward(params, x["obs"], pd, x["hx0"])
    sigma = np.exp(params["actor_log_std"].astype(np.float64))
    arng = np.random.default_rng(seed + 4)
    eps = arng.standard_normal(mean.shape)
    if case.tail:
        eps = np.where(eps >= 0, 4.0, -4.0)
    x["actions"] = (mean + sigma * eps).astype(np.float32)
    lp = GO.log_probs(params, x["obs"], x["actions"], pd, x["hx0"])
    if case.on_policy:
        x["old_log_probs"] = lp.astype(np.float32)
    else:
        noise = np.random.default_rng(seed + 2).standard_normal(lp.shape)
        x["old_log_probs"] = (lp + (case.old_noise or OLD_NOISE) * noise).astype(np.float32)
    B = T * Nn
    m = max(1, int(B * case.frac))
    mb_idx = np.random.default_rng(7).permutation(B)[:m].astype(np.int32)
    return params, x, mb_idx, case.m_total_mul * len(mb_idx)


def guards(case, params, x, mb_idx):
    """gru_cases.guards with the Gaussian oracle's log-probs: (nearest distance of a selected
    ratio to a clip edge, share of selected samples whose policy gradient is zero)."""
    lp = GO.log_probs(params, x["obs"], x["actions"], x["prev_dones"], x["hx0"])
    ratio = np.exp(lp - x["old_log_probs"].astype(np.float64)).reshape(-1)[mb_idx]
    adv = x["advantages"].astype(np.float64).reshape(-1)[mb_idx]
    edge = min(np.abs(ratio - (1 - case.clip)).min(), np.abs(ratio - (1 + case.clip)).min())
    clipped = ((adv > 0) & (ratio > 1 + case.clip)) | ((adv < 0) & (ratio < 1 - case.clip))
    share = float(clipped.mean())
    if case.on_policy:
        assert np.all((ratio >= 1 - 1e-5) & (ratio <= 1 + 1e-5)), (ratio.min(), ratio.max())
        assert share == 0.0
    else:
        assert edge >= 1e-4, edge
        if len(mb_idx) >= 15:
            k, m = int(clipped.sum()), len(mb_idx)      # at least 20 % on either side
            assert 5 * k >= m and 5 * (m - k) >= m, share
    return float(edge), share
