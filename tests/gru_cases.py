"""Inputs of the GRU minibatch kernel's edge cases (tests/test_gpu_gru.py), built on the CPU so the
clip-regime guards of every case can be evaluated with the float64 oracle alone
(tests/test_gru_oracle_cpu.py) before the kernel runs them.  Test infrastructure only.

A case is (shape, selection, hyperparameters, dones pattern, old-policy recipe).  The weights are
RecurrentPPO's initial ones (orthogonal init under the config's seed) plus 0.3 * N(0, 1), so gates
and heads leave their linear range; the data is the recipe of test_gpu_gru._data at seed
T * 100 + N.  The PPO surrogate has a kink at ratio = 1 +- clip where the gradient is undefined:
``guards`` are the conditions that keep every selected sample away from it and both branches of
the clip populated."""
from dataclasses import dataclass
from math import sqrt

import numpy as np
import torch

from oracle import gru_torch as GT

G = 16  # RecurrentPPOConfig.gru_hidden_dim


@dataclass(frozen=True)
class Case:
    name: str
    shape: tuple                 # (T, N, D, A)
    frac: float = 1.0            # share of the batch selected (a seeded permutation's head)
    pick: tuple | None = None    # (t, n): select this one sample instead
    clip: float = 0.15
    vf: float = 1.0
    ent: float = 0.01
    m_total_mul: int = 1         # m_total = mul * m (the data-parallel union minibatch)
    dones: str = "random"        # random | none | first | env_always | last
    on_policy: bool = False
    # numerical regimes (tests/regime_cases.py); the defaults leave a case as it was
    obs_scale: float = 1.0       # on the observations
    gru_scale: float = 1.0       # on gru.weight_ih_l0 and gru.weight_hh_l0 (gates, candidate)
    actor_scale: float = 1.0     # on actor_head.2.weight (the logits)
    ret_scale: float = 1.0       # on the returns
    old_noise: float = 0.0       # > 0: old log-probs = the parameters' own + old_noise * N(0, 1)
    seed_shift: int = 0          # added to the shape's seed (weights and data)

    def __str__(self):
        return self.name


KTAIL_SHAPES = [(1, 1, 1, 1), (3, 1, 2, 2), (5, 3, 4, 2), (7, 17, 5, 3), (9, 18, 32, 16),
                (6, 33, 31, 15)]
MID = (7, 17, 5, 3)
DONE_ENV = 5    # the env that is done at every step in "env_always"

CASES = (
    # S = T * ne per workgroup of 16 envs: S % 4 = 1, 3, 3, {0,3}, {0,2}, {0,0,2}
    [Case(f"ktail-{'x'.join(map(str, s))}-{f}", s, frac=f) for s in KTAIL_SHAPES for f in (1.0, 0.4)]
    + [Case(f"hyper-c{c}-v{v}-e{e}-x{k}", MID, clip=c, vf=v, ent=e, m_total_mul=k)
       for c, v, e in ((0.3, 0.5, 0.0), (0.05, 2.0, 0.05)) for k in (1, 3)]
    + [Case(f"dones-{d}", MID, dones=d) for d in ("none", "first", "env_always", "last")]
    + [Case("pick-last-step", MID, pick=(MID[0] - 1, 2), dones="none"),
       Case("pick-first-step", MID, pick=(0, 2), dones="none")]
    + [Case(f"onpolicy-{'x'.join(map(str, s))}", s, on_policy=True) for s in (MID, (9, 18, 32, 16))]
)


def initial_params(D, A, seed=42, G=G):
    """RecurrentPPO's initial weights for RecurrentPPOConfig(gru_hidden_dim=G, seed=seed), built
    on the CPU."""
    import gym_stub
    from diamond.recurrent_ppo import (RecurrentActorCriticNetwork, RecurrentPPOConfig,
                                       network_parameter_init_)
    torch.manual_seed(seed)
    net = RecurrentActorCriticNetwork(gym_stub.Box(shape=(D,)), gym_stub.Discrete(A),
                                      cfg=RecurrentPPOConfig(gru_hidden_dim=G))
    network_parameter_init_(net, gain=sqrt(2.0))
    p = {n: t.detach().numpy().copy() for n, t in net.named_parameters()}
    assert list(p) == GT.GRU_NAMES
    return p


def data(T, Nn, D, A, seed, G=G):
    rng = np.random.default_rng(seed)
    return dict(obs=rng.standard_normal((T, Nn, D)).astype(np.float32),
                actions=rng.integers(0, A, (T, Nn)).astype(np.int32),
                old_log_probs=(-rng.uniform(0.2, 1.5, (T, Nn))).astype(np.float32),
                advantages=rng.standard_normal((T, Nn)).astype(np.float32),
                returns=rng.standard_normal((T, Nn)).astype(np.float32),
                prev_dones=(rng.random((T, Nn)) < 0.08),
                hx0=(rng.standard_normal((Nn, G)) * 0.5).astype(np.float32))


def scaled_params(params, case):
    """The parameters with the case's regime scales on the GRU and actor output weights."""
    params = dict(params)
    for n, k in (("gru.weight_ih_l0", case.gru_scale), ("gru.weight_hh_l0", case.gru_scale),
                 ("actor_head.2.weight", case.actor_scale)):
        if k != 1.0:
            params[n] = params[n] * np.float32(k)
    return params


def build(case):
    """(params, data dict, mb_idx int32, m_total) of one case, at the case's own G where it has
    one (tests/gru_wide_cases.py) and at 16 otherwise."""
    T, Nn, D, A = case.shape
    width = getattr(case, "G", G)
    seed = T * 100 + Nn + case.seed_shift
    rng = np.random.default_rng(seed + 1)
    params = {n: (p + 0.3 * rng.standard_normal(p.shape)).astype(np.float32)
              for n, p in initial_params(D, A, G=width).items()}
    x = data(T, Nn, D, A, seed, G=width)
    params = scaled_params(params, case)
    if case.obs_scale != 1.0:
        x["obs"] = x["obs"] * np.float32(case.obs_scale)
    if case.ret_scale != 1.0:
        x["returns"] = x["returns"] * np.float32(case.ret_scale)
    pd = x["prev_dones"]
    if case.dones == "none":
        pd[:] = False
    elif case.dones == "first":
        pd[0] = True
    elif case.dones == "env_always":
        pd[:, DONE_ENV] = True
    elif case.dones == "last":
        pd[:] = False
        pd[T - 1] = True
    else:
        assert case.dones == "random"
    if case.on_policy:
        lp = GT.log_probs(params, x["obs"], x["actions"], pd, x["hx0"])
        x["old_log_probs"] = lp.astype(np.float32)
    elif case.old_noise > 0.0:
        lp = GT.log_probs(params, x["obs"], x["actions"], pd, x["hx0"])
        noise = np.random.default_rng(seed + 2).standard_normal(lp.shape)
        x["old_log_probs"] = (lp + case.old_noise * noise).astype(np.float32)
    B = T * Nn
    if case.pick is not None:
        mb_idx = np.array([case.pick[0] * Nn + case.pick[1]], np.int32)
    else:
        m = max(1, int(B * case.frac))
        mb_idx = np.random.default_rng(7).permutation(B)[:m].astype(np.int32)
    return params, x, mb_idx, case.m_total_mul * len(mb_idx)


def guards(case, params, x, mb_idx):
    """The clip-regime conditions of one case, from the float64 oracle alone.  Returns
    (nearest distance of a selected sample's ratio to an edge 1 +- clip, share of selected samples
    whose policy gradient is zero) after asserting them."""
    lp = GT.log_probs(params, x["obs"], x["actions"], x["prev_dones"], x["hx0"])
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
