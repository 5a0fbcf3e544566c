"""Float64 PyTorch-CPU yardstick of RecurrentContinuousPPO's minibatch loss, gradient and learn().
TEST INFRASTRUCTURE ONLY.

The reference has no recurrent Gaussian agent, and its RecurrentPPO cannot run (oracle/gru_torch.py).
This restates the Gaussian head and loss of reference diamond/continuous_ppo.py (JointNormal :40-47,
the state-independent actor_log_std :95, the loss :276-292) on top of the recurrent sequence
``oracle.gru_torch.sequence``: that function is handed the parameter dict with ``actor_mean_head.*``
under the ``actor_head.*`` keys, so its "logits" are the means.  The distribution is
``torch.distributions.Normal(mean, log_std.exp())`` with log-prob and entropy summed over the last
axis.  ``log_probs``, ``minibatch_grads`` (with ``dt=torch.float32``: torch's own float32 error)
and ``learn`` mirror oracle/gru_torch.py's.

Parameters: dict name -> numpy array in ``named_parameters()`` order (PARAM_NAMES).
"""
from __future__ import annotations

import numpy as np
import torch

from oracle import gru_torch as GT
from oracle import ppo_np as P

PARAM_NAMES = ["actor_log_std"] + [n.replace("actor_head.", "actor_mean_head.")
                                   for n in GT.GRU_NAMES]


def _seq_params(p):
    """The dict oracle.gru_torch.sequence reads: the mean head under the actor head's keys."""
    return {n.replace("actor_mean_head.", "actor_head."): v for n, v in p.items()
            if n != "actor_log_std"}


def _dist(p, obs, prev_dones, hx0):
    mean, values = GT.sequence(_seq_params(p), obs, prev_dones, hx0)
    log_std = torch.broadcast_to(p["actor_log_std"], mean.shape)
    return torch.distributions.Normal(mean, log_std.exp()), mean, values


def forward(params, obs, prev_dones, hx0):
    """Float64 (means [T, N, A], values [T, N]) under ``params``."""
    d = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float64)
    with torch.no_grad():
        _, mean, values = _dist({k: d(v) for k, v in params.items()}, d(obs),
                                torch.as_tensor(np.asarray(prev_dones, bool)), d(hx0))
    return mean.numpy(), values.numpy()


def log_probs(params, obs, actions, prev_dones, hx0, entropy=False):
    """Float64 joint log-probabilities [T, N] of the taken actions [T, N, A] under ``params``
    (and the joint entropy [T, N] with ``entropy``)."""
    d = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float64)
    with torch.no_grad():
        dist, _, _ = _dist({k: d(v) for k, v in params.items()}, d(obs),
                           torch.as_tensor(np.asarray(prev_dones, bool)), d(hx0))
        lp = dist.log_prob(d(actions)).sum(-1).numpy()
        return (lp, dist.entropy().sum(-1).numpy()) if entropy else lp


def minibatch_grads(params, obs, actions, old_log_probs, advantages, returns, prev_dones, hx0,
                    mb_idx, m_total, clip=0.15, vf=1.0, ent=0.01, dt=torch.float64):
    """(loss sums {policy, value, entropy}, grads dict) for the samples mb_idx (flat t * N + n) of
    one rollout, divided by m_total: oracle.gru_torch.minibatch_grads with the Gaussian head."""
    p = {k: torch.tensor(np.asarray(v), dtype=dt, requires_grad=True) for k, v in params.items()}
    d = lambda x: torch.as_tensor(np.asarray(x), dtype=dt)
    dist, mean, values = _dist(p, d(obs), torch.as_tensor(np.asarray(prev_dones, bool)), d(hx0))
    A = mean.shape[-1]
    mb_idx = np.asarray(mb_idx).astype(np.int64)
    act = d(actions).reshape(-1, A)
    lp = dist.log_prob(act.reshape(mean.shape)).sum(-1).reshape(-1)[mb_idx]
    en = dist.entropy().sum(-1).reshape(-1)[mb_idx].sum()
    v = values.reshape(-1)[mb_idx]
    ratio = torch.exp(lp - d(old_log_probs).reshape(-1)[mb_idx])
    adv = d(advantages).reshape(-1)[mb_idx]
    ret = d(returns).reshape(-1)[mb_idx]
    pi = torch.maximum(-adv * ratio, -adv * torch.clamp(ratio, 1 - clip, 1 + clip)).sum()
    vl = (0.5 * (v - ret) ** 2).sum()
    loss = (pi + vf * vl - ent * en) / m_total
    loss.backward()
    sums = np.array([pi.item(), vl.item(), en.item()])
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return sums, {k: zero(t).numpy().copy() for k, t in p.items()}


stack_experience = GT.stack_experience
lr_after_learn = GT.lr_after_learn


def learn(params, adam, exp, cfg, lr, perms):
    """One learn() call: oracle.gru_torch.learn with the Gaussian minibatch gradient.  Updates
    ``params`` (float32 arrays) and ``adam`` (ppo_np.new_adam_state) in place; same returns."""
    f32 = np.float32
    values = np.asarray(exp["values"], f32)
    adv = P.gae(exp["rewards"], exp["terms"], exp["truncs"], values, exp["next_values"],
                cfg.gamma, cfg.gae_lambda)
    returns = values + adv
    if cfg.advantage_norm:
        adv = P.normalize_adv(adv)
    T, Nn = values.shape
    B = T * Nn
    E, M = cfg.num_epochs, cfg.num_minibatches
    mb = B // M
    idx = np.asarray(perms).reshape(E, M, mb)
    losses, norms = [], []
    for e in range(E):
        for j in range(M):
            sums, g = minibatch_grads(params, exp["obs"], exp["actions"], exp["log_probs"], adv,
                                      returns, exp["prev_dones"], exp["hx0"], idx[e, j], mb,
                                      cfg.ppo_clip, cfg.value_loss_weight, cfg.entropy_beta)
            g = {n: g[n].astype(f32) for n in PARAM_NAMES}
            norm, _ = P.clip_grad_norm(g, PARAM_NAMES, cfg.grad_norm_clip)
            P.adam_step(params, g, adam, PARAM_NAMES, lr, cfg.adam_eps)
            pi, vl, en = sums / mb
            losses.append([pi + cfg.value_loss_weight * vl - cfg.entropy_beta * en, pi, vl, en])
            norms.append(norm)
    return dict(params=params, adam=adam, losses=np.array(losses), norm=np.array(norms), adv=adv,
                returns=returns, idx=idx)
