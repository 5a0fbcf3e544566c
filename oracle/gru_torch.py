"""Float64 PyTorch-CPU restatement of RecurrentPPO's minibatch loss and gradient -- the INTENDED
semantics of reference diamond/recurrent_ppo.py.  TEST INFRASTRUCTURE ONLY.

The reference cannot run (GRUCore.forward evaluates ``hx or torch.zeros(...)`` and
``dones or ...`` on multi-element tensors, recurrent_ppo.py:78-79, raising RuntimeError for every
num_envs: SURVEY.md §3.5, §8(c)), so no golden trace exists.  This restates what its code says it
does, evaluated in float64 with autograd as the yardstick of the fused HIP kernel (grugrad.hip):

* ``RecurrentActorCriticNetwork`` (:94-149): base Linear(D, 64) + tanh; ``GRUCore`` (:41-91) = a
  torch GRU cell stepped over t with the hidden state zeroed where ``dones[t]`` (:82-87);
  actor / critic heads Linear(16, 64) tanh Linear(64, A | 1) on the GRU output.
* ``learn`` (:301-367): the full [T, N] sequence recomputed from the rollout's initial hidden
  state (:313, :337), flattened t-major (:340-341), the minibatch's samples selected, the PPO loss
  (:343-356, as ppo.py:264-280), backward.

* ``learn`` below restates the whole update (:301-367) around ``minibatch_grads``: float32 GAE,
  returns and advantage normalisation, the minibatch split, and per minibatch the float64 gradient
  cast to float32, clip_grad_norm_ and Adam (oracle/ppo_np.py, the yardsticks of the MLP agents).

Parameters: dict name -> numpy array in ``named_parameters()`` order (GRU_NAMES).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from . import ppo_np as P

GRU_NAMES = ["base.0.weight", "base.0.bias", "gru.weight_ih_l0", "gru.weight_hh_l0",
             "gru.bias_ih_l0", "gru.bias_hh_l0", "actor_head.0.weight", "actor_head.0.bias",
             "actor_head.2.weight", "actor_head.2.bias", "critic_head.0.weight",
             "critic_head.0.bias", "critic_head.2.weight", "critic_head.2.bias"]


def sequence(p, obs, prev_dones, hx0):
    """Heads over the whole rollout: logits [T, N, A], values [T, N] (recurrent_ppo.py:127-149)."""
    T = obs.shape[0]
    G = p["gru.weight_hh_l0"].shape[1]
    x1 = torch.tanh(F.linear(obs, p["base.0.weight"], p["base.0.bias"]))
    gi = F.linear(x1, p["gru.weight_ih_l0"], p["gru.bias_ih_l0"])
    h = hx0
    outs = []
    for t in range(T):
        h = h * (~prev_dones[t]).to(h.dtype)[:, None]          # hx[:, dones[t]] = 0 (:84)
        gh = F.linear(h, p["gru.weight_hh_l0"], p["gru.bias_hh_l0"])
        r = torch.sigmoid(gi[t, :, :G] + gh[:, :G])
        z = torch.sigmoid(gi[t, :, G:2 * G] + gh[:, G:2 * G])
        n = torch.tanh(gi[t, :, 2 * G:] + r * gh[:, 2 * G:])
        h = (1 - z) * n + z * h
        outs.append(h)
    ho = torch.stack(outs)
    ya = torch.tanh(F.linear(ho, p["actor_head.0.weight"], p["actor_head.0.bias"]))
    logits = F.linear(ya, p["actor_head.2.weight"], p["actor_head.2.bias"])
    yc = torch.tanh(F.linear(ho, p["critic_head.0.weight"], p["critic_head.0.bias"]))
    values = F.linear(yc, p["critic_head.2.weight"], p["critic_head.2.bias"]).squeeze(-1)
    return logits, values


def log_probs(params, obs, actions, prev_dones, hx0):
    """Float64 log-probabilities [T, N] of the taken actions under ``params``."""
    d = lambda x: torch.as_tensor(np.asarray(x), dtype=torch.float64)
    with torch.no_grad():
        logits, _ = sequence({k: d(v) for k, v in params.items()}, d(obs),
                             torch.as_tensor(np.asarray(prev_dones, bool)), d(hx0))
        act = torch.as_tensor(np.asarray(actions), dtype=torch.int64)
        return torch.distributions.Categorical(logits=logits).log_prob(act).numpy()


def minibatch_grads(params, obs, actions, old_log_probs, advantages, returns, prev_dones, hx0,
                    mb_idx, m_total, clip=0.15, vf=1.0, ent=0.01, dt=torch.float64):
    """(loss sums {policy, value, entropy}, grads dict) in float64 for the samples mb_idx (flat
    t * N + n) of one rollout, divided by m_total (recurrent_ppo.py:337-358).  ``dt=torch.float32``
    evaluates the same graph in float32: torch's own float32 error, the yardstick of a float32
    kernel's distance from the float64 result."""
    p = {k: torch.tensor(np.asarray(v), dtype=dt, requires_grad=True) for k, v in params.items()}
    d = lambda x: torch.as_tensor(np.asarray(x), dtype=dt)
    logits, values = sequence(p, d(obs), torch.as_tensor(np.asarray(prev_dones, bool)), d(hx0))
    A = logits.shape[-1]
    lg = logits.reshape(-1, A)[mb_idx]
    v = values.reshape(-1)[mb_idx]
    act = torch.as_tensor(np.asarray(actions).reshape(-1)[mb_idx], dtype=torch.int64)
    dist = torch.distributions.Categorical(logits=lg)
    ratio = torch.exp(dist.log_prob(act) - d(old_log_probs).reshape(-1)[mb_idx])
    adv = d(advantages).reshape(-1)[mb_idx]
    ret = d(returns).reshape(-1)[mb_idx]
    pi = torch.maximum(-adv * ratio, -adv * torch.clamp(ratio, 1 - clip, 1 + clip)).sum()
    vl = (0.5 * (v - ret) ** 2).sum()
    en = dist.entropy().sum()
    loss = (pi + vf * vl - ent * en) / m_total
    loss.backward()
    sums = np.array([pi.item(), vl.item(), en.item()])
    return sums, {k: t.grad.numpy().copy() for k, t in p.items()}


EXP_KEYS = ("obs", "actions", "rewards", "terms", "truncs", "prev_dones", "log_probs", "values",
            "next_values")


def stack_experience(experience):
    """RecurrentPPO.rollout()'s list of per-step rows -> dict of stacked [T, N, ...] numpy arrays
    plus ``hx0`` [N, G], the first row's hidden state (recurrent_ppo.py:303-313)."""
    host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    cols = list(zip(*experience))
    out = {k: np.stack([host(x) for x in col]) for k, col in zip(EXP_KEYS, cols)}
    hx = host(cols[9][0])
    out["hx0"] = hx.reshape(hx.shape[-2], hx.shape[-1])
    return out


def lr_after_learn(lr_now, calls_done, cfg):
    """param_groups[0]["lr"] after the ``calls_done``-th learn()'s lr_scheduler.step()
    (recurrent_ppo.py:190-195, :367): LinearLR from 1.0 to 0.05 when ``decay_lr``, else constant."""
    total_iters = cfg.total_steps // (cfg.num_envs * cfg.rollout_steps)
    return P.linear_lr_factor_step(lr_now, calls_done, total_iters, 1.0,
                                   0.05 if cfg.decay_lr else 1.0)


def learn(params, adam, exp, cfg, lr, perms):
    """One learn() call (recurrent_ppo.py:301-367), updating ``params`` (float32 arrays) and the
    Adam state ``adam`` (ppo_np.new_adam_state) in place.  ``exp`` is stack_experience()'s dict,
    ``cfg`` any object with RecurrentPPOConfig's hyperparameter fields, ``perms`` the [E, B]
    permutations (:330).  Returns {"params", "adam", "losses" [E*M, 4] = the minibatches' mean
    {loss, policy, value, entropy}, "norm" [E*M] (gradient norms before the clip), "adv", "returns"
    [T, N] float32, "idx" [E, M, B // M]}."""
    f32 = np.float32
    values = np.asarray(exp["values"], f32)
    adv = P.gae(exp["rewards"], exp["terms"], exp["truncs"], values, exp["next_values"],
                cfg.gamma, cfg.gae_lambda)                                       # :315
    returns = values + adv                                                       # :316
    if cfg.advantage_norm:
        adv = P.normalize_adv(adv)                                               # :317-318
    T, Nn = values.shape
    B = T * Nn
    E, M = cfg.num_epochs, cfg.num_minibatches
    mb = B // M
    idx = np.asarray(perms).reshape(E, M, mb)                                    # :329-331
    losses, norms = [], []
    for e in range(E):
        for j in range(M):
            sums, g = minibatch_grads(params, exp["obs"], exp["actions"], exp["log_probs"], adv,
                                      returns, exp["prev_dones"], exp["hx0"], idx[e, j], mb,
                                      cfg.ppo_clip, cfg.value_loss_weight, cfg.entropy_beta)
            g = {n: g[n].astype(f32) for n in GRU_NAMES}
            norm, _ = P.clip_grad_norm(g, GRU_NAMES, cfg.grad_norm_clip)         # :364
            P.adam_step(params, g, adam, GRU_NAMES, lr, cfg.adam_eps)            # :365
            pi, vl, en = sums / mb
            losses.append([pi + cfg.value_loss_weight * vl - cfg.entropy_beta * en, pi, vl, en])
            norms.append(norm)
    return dict(params=params, adam=adam, losses=np.array(losses), norm=np.array(norms), adv=adv,
                returns=returns, idx=idx)
