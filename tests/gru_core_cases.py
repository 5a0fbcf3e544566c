"""Shapes, networks and CPU replicas shared by the ``fused_core`` tests (tests/test_gru_core_cpu.py,
tests/test_gpu_gru_core_learn.py).  Test infrastructure only.

Every shape here is one the fused GRU class turns down (``fused_gru_shape`` False, or a network
class of the user's own), so RecurrentPPO runs its torch learn loop and torch rollout."""
import copy
from math import sqrt

import numpy as np
import torch
import torch.nn as nn

import gym_stub
from diamond.recurrent_ppo import (GRUCore, RecurrentActorCriticNetwork, RecurrentPPOConfig,
                                   network_parameter_init_)

T, NENVS = 8, 9
# name -> (network_hidden_dim, gru_hidden_dim, obs_dim, act_dim)
LEARN_SHAPES = {"h128-g32": (128, 32, 40, 6), "h64-g64": (64, 64, 33, 17)}
DEFAULT_SHAPE = (64, 16, 8, 4)          # the fused class serves this one

ROLLOUT_T = 4
ROLLOUT_SHAPE = LEARN_SHAPES["h128-g32"]
ROLLOUT_ENV_SEED = 29     # of seeds 0..59 the one with the largest smallest margin
# On the actor's output layer: the initial logits (gain 0.01) become so far apart that
# Categorical.sample() returns the arg-max action whatever the generator draws -- an action of
# margin M in the logits loses with probability below act_dim * exp(-M).
PEAK_SCALE = 2.0e5
PEAK_MARGIN = 30.0


class TwoLayerBaseNetwork(nn.Module):
    """A network of the user's own around GRUCore: two-layer base, hidden 96, GRUCore(96, 16)."""

    def __init__(self, observation_space, action_space, cfg) -> None:
        super().__init__()
        d = int(np.prod(observation_space.shape))
        self.base = nn.Sequential(nn.Linear(d, 96), nn.Tanh(), nn.Linear(96, 96), nn.Tanh())
        self.gru = GRUCore(96, 16)
        self.actor_head = nn.Sequential(nn.Linear(16, 96), nn.Tanh(),
                                        nn.Linear(96, int(action_space.n)))
        self.actor_out_layer = self.actor_head[-1]
        self.critic_head = nn.Sequential(nn.Linear(16, 96), nn.Tanh(), nn.Linear(96, 1))

    def get_values(self, observations, hx, dones):
        x, hx = self.gru.forward(self.base(observations), hx, dones)
        return self.critic_head(x).squeeze(-1)

    def get_logits_values_and_hx(self, observations, hx, dones):
        x, hx = self.gru.forward(self.base(observations), hx, dones)
        return self.actor_head(x), self.critic_head(x).squeeze(-1), hx


def config(shape, **kw):
    H, G, _, _ = shape
    kw.setdefault("rollout_steps", T)
    kw.setdefault("num_envs", NENVS)
    return RecurrentPPOConfig(network_hidden_dim=H, gru_hidden_dim=G, verbose=False, **kw)


def make_envs(shape, n=NENVS):
    _, _, D, A = shape
    return gym_stub.SyncVectorEnv([lambda: gym_stub.SyntheticEnv(D, A, p_term=0.1)] * n)


def initial_network(shape, cfg, network_cls=RecurrentActorCriticNetwork):
    """RecurrentPPO's initial network for ``cfg``, built on the CPU as __init__ builds it."""
    _, _, D, A = shape
    torch.manual_seed(cfg.seed)
    net = network_cls(gym_stub.Box(shape=(D,)), gym_stub.Discrete(A), cfg=cfg)
    network_parameter_init_(net, gain=sqrt(2.0))
    return net


def initial_params(shape, cfg):
    return {n: p.detach().numpy().copy() for n, p in initial_network(shape, cfg).named_parameters()}


def rollout_start(shape, n=NENVS):
    """The hidden state the rollout tests start from."""
    g = torch.Generator().manual_seed(5)
    return torch.randn(1, n, shape[1], generator=g) * 0.5


def peak_(network):
    with torch.no_grad():
        network.actor_out_layer.weight.mul_(PEAK_SCALE)


def replica_logits(network, shape, steps=ROLLOUT_T, n=NENVS, env_seed=ROLLOUT_ENV_SEED):
    """RecurrentPPO.rollout()'s logits [steps, n, A] and hidden states from the float64 CPU copy of
    ``network`` on the stub env's observation stream (which no action influences)."""
    net = copy.deepcopy(network).double().cpu()
    for m in net.modules():
        if isinstance(m, GRUCore):
            m.fused_scan = False
    envs = make_envs(shape, n)
    obs, _ = envs.reset(seed=env_seed)
    hx = rollout_start(shape, n).double()
    prev = np.zeros(n, bool)
    logits, hxs = [], []
    with torch.no_grad():
        for _ in range(steps):
            lg, _, hx = net.get_logits_values_and_hx(
                torch.as_tensor(obs[None], dtype=torch.float64), hx, torch.as_tensor(prev[None]))
            logits.append(lg[0])
            hxs.append(hx)
            nobs, _, te, tr, _ = envs.step(np.zeros(n, np.int64))
            prev = np.logical_or(te, tr)
            obs = envs.reset(options={"reset_mask": prev})[0] if prev.any() else nobs
    return torch.stack(logits), torch.stack(hxs)


def action_margins(logits):
    """Per sample, the gap between the largest and the second largest logit."""
    top = logits.topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]
