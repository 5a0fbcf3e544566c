"""CPU pin of oracle/gru_torch.py.

* Its functional GRU sequence equals the package's RecurrentActorCriticNetwork (nn.GRU cell stepped
  per t with hidden resets -- the intended semantics of reference recurrent_ppo.py:41-91,94-149)
  on the same parameters, in float64.
* Its learn() (the whole update of recurrent_ppo.py:301-367: minibatch split, float64 gradient
  cast to float32, float32 clip_grad_norm_ and Adam, LinearLR between calls) equals plain torch
  on the CPU: that network in float64, the loss as the reference writes it,
  nn.utils.clip_grad_norm_, torch.optim.Adam and LinearLR, on the same advantages and permutations.
  Parameters agree to 1e-6: torch keeps the parameters in float64, the oracle rounds them to
  float32 after every step (half an ulp of a weight below 2 is 1.2e-7 at the most, and the
  steps' roundings do not all point the same way), over four to six steps of lr 3e-4.
  A minibatch count has to divide T * N (the reference reshapes the permutation, :331), so the
  15-sample shape (5, 3, 4, 2) runs 2 x 3 minibatches and the 2 x 2 split runs at (5, 4, 4, 2).
* The clip-regime guards of every edge case of tests/test_gpu_gru.py (tests/gru_cases.py) hold,
  evaluated with the float64 oracle alone.
"""
from math import sqrt

import numpy as np
import pytest
import torch

import gru_cases
from diamond.recurrent_ppo import (RecurrentActorCriticNetwork, RecurrentPPOConfig,
                                   network_parameter_init_)
from oracle import gru_torch as GT
from oracle import ppo_np


class Box:
    def __init__(self, n):
        self.shape = (n,)


class Discrete:
    def __init__(self, n):
        self.n = n


def test_oracle_sequence_matches_module():
    T, Nn, D, A = 12, 9, 5, 3
    torch.manual_seed(1)
    net = RecurrentActorCriticNetwork(Box(D), Discrete(A), RecurrentPPOConfig()).double()
    rng = np.random.default_rng(0)
    obs = torch.from_numpy(rng.standard_normal((T, Nn, D)))
    dones = torch.from_numpy(rng.random((T, Nn)) < 0.2)
    hx = torch.from_numpy(rng.standard_normal((1, Nn, 16)))
    with torch.no_grad():
        lg, v, _ = net.get_logits_values_and_hx(obs, hx, dones)
    p = {n: t.detach() for n, t in net.named_parameters()}
    assert list(p) == GT.GRU_NAMES
    lg2, v2 = GT.sequence(p, obs, dones, hx[0])
    torch.testing.assert_close(lg2, lg, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(v2, v, rtol=1e-12, atol=1e-12)


def _torch_learn(net, opt, sched, x, cfg, adv, returns, idx):
    """One learn() in plain torch on the CPU (float64 network), the loss term by term as
    recurrent_ppo.py:337-367 writes it, on given advantages, returns and minibatch indices."""
    d = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    obs, hx = d(x["obs"]), d(x["hx0"])[None]
    dones = torch.as_tensor(np.asarray(x["prev_dones"], bool))
    actions = torch.as_tensor(np.asarray(x["actions"]).reshape(-1), dtype=torch.int64)
    old, adv, returns = d(x["log_probs"]).reshape(-1), d(adv).reshape(-1), d(returns).reshape(-1)
    for b_idx in idx:
        for mb in b_idx:
            mb = torch.as_tensor(mb, dtype=torch.int64)
            logits, values, _ = net.get_logits_values_and_hx(obs, hx, dones)
            logits, values = logits.reshape(-1, logits.shape[-1])[mb], values.reshape(-1)[mb]
            dist = torch.distributions.Categorical(logits=logits)
            ratio = (dist.log_prob(actions[mb]) - old[mb]).exp()
            unclipped = -adv[mb] * ratio
            clipped = -adv[mb] * torch.clamp(ratio, 1.0 - cfg.ppo_clip, 1.0 + cfg.ppo_clip)
            loss = (torch.max(unclipped, clipped).mean()
                    + cfg.value_loss_weight * 0.5 * torch.nn.functional.mse_loss(values, returns[mb])
                    - cfg.entropy_beta * dist.entropy().mean())
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(net.parameters(), cfg.grad_norm_clip)
            opt.step()
    sched.step()


def _pin(T, Nn, D, A, calls, **kw):
    from dist_scripts.recurrent_dp import synth_experience
    cfg = RecurrentPPOConfig(rollout_steps=T, num_envs=Nn, **kw)
    torch.manual_seed(3)
    net = RecurrentActorCriticNetwork(Box(D), Discrete(A), cfg)
    network_parameter_init_(net, gain=sqrt(2.0))
    params = {n: t.detach().numpy().copy() for n, t in net.named_parameters()}
    net = net.double()
    opt = torch.optim.Adam(net.parameters(), lr=cfg.lr, eps=cfg.adam_eps)
    sched = torch.optim.lr_scheduler.LinearLR(
        opt, start_factor=1.0, end_factor=0.05 if cfg.decay_lr else 1.0,
        total_iters=cfg.total_steps // (Nn * T))
    adam = ppo_np.new_adam_state(params, GT.GRU_NAMES)
    lr, B = cfg.lr, T * Nn
    for call in range(calls):
        x = GT.stack_experience(synth_experience(T, Nn, D, A, cfg.gru_hidden_dim, "cpu",
                                                 seed=10 + call))
        rs = np.random.RandomState(20 + call)
        perms = np.stack([rs.permutation(B) for _ in range(cfg.num_epochs)])
        out = GT.learn(params, adam, x, cfg, lr, perms)
        lr = GT.lr_after_learn(lr, call + 1, cfg)
        _torch_learn(net, opt, sched, x, cfg, out["adv"], out["returns"], out["idx"])
        assert opt.param_groups[0]["lr"] == lr
        steps = (call + 1) * cfg.num_epochs * cfg.num_minibatches
        assert adam["step"] == steps
        moved = 0.0
        for n, t in net.named_parameters():
            np.testing.assert_allclose(params[n], t.detach().numpy(), rtol=0, atol=1e-6, err_msg=n)
            st = opt.state[t]
            assert int(st["step"]) == steps
            np.testing.assert_allclose(adam["m"][n], st["exp_avg"].numpy(), rtol=1e-5, atol=1e-9)
            np.testing.assert_allclose(adam["v"][n], st["exp_avg_sq"].numpy(), rtol=1e-5,
                                       atol=1e-12)
            moved = max(moved, np.abs(adam["m"][n]).max())
        assert moved > 0 and np.all(np.isfinite(out["losses"]))
    return lr, cfg


@pytest.mark.parametrize("T,Nn,D,A,E,M", [(5, 3, 4, 2, 2, 3), (5, 4, 4, 2, 2, 2)])
def test_oracle_learn_matches_plain_torch(T, Nn, D, A, E, M):
    lr, cfg = _pin(T, Nn, D, A, 1, num_epochs=E, num_minibatches=M)
    assert lr == cfg.lr


def test_oracle_learn_decaying_lr_two_calls():
    """Two learn() calls of 1 x 2 minibatches under decay_lr: the second call runs at the decayed
    rate and carries the first call's Adam state and step count."""
    T, Nn = 5, 4
    lr, cfg = _pin(T, Nn, 4, 2, 2, num_epochs=1, num_minibatches=2, decay_lr=True,
                   total_steps=3 * T * Nn)
    # LinearLR over 3 iterations from 1.0 to 0.05: factor 1 - 0.95 * 2 / 3 after two steps
    assert lr == pytest.approx(cfg.lr * (1 - 0.95 * 2 / 3), rel=1e-12)


@pytest.mark.parametrize("case", gru_cases.CASES, ids=str)
def test_gradient_case_guards_hold(case):
    params, x, mb_idx, m_total = gru_cases.build(case)
    assert m_total == case.m_total_mul * len(mb_idx) and len(set(mb_idx.tolist())) == len(mb_idx)
    edge, share = gru_cases.guards(case, params, x, mb_idx)
    print(f"{case}: m={len(mb_idx)} nearest edge {edge:.3e} zero-policy-gradient share {share:.2f}")
