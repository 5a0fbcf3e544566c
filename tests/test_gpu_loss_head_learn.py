"""learn() with ``fused_loss = True``: the generic path of PPO / ContinuousPPO and RecurrentPPO's
torch loop take the loss head from csrc/losshead.hip and still meet the bounds their torch
versions are held to; with the flag off nothing runs the kernel."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

import diamond
import gru_cases
import test_gpu_gru_learn as GL


def experience(z, li):
    keys = ("obs", "next_obs", "actions", "rewards", "term", "trunc")
    arrs = [z[f"exp{li}/" + k] for k in keys]
    return [[a[k] for a in arrs] for k in range(arrs[0].shape[0])]


def _custom_agent(z, fused_loss):
    """The agent of test_generic_network_path_matches_reference_trace: a subclass of the default
    network, which no fused class claims."""
    import gym_stub
    T, Nn, D, A, cont, n_learn = (int(x) for x in z["dims"])
    base = diamond.continuous_ppo.ContinuousActorCriticNetwork if cont else \
        diamond.ppo.ActorCriticNetwork

    class CustomNet(base):
        pass

    Cfg = diamond.ContinuousPPOConfig if cont else diamond.PPOConfig
    Agent = diamond.ContinuousPPO if cont else diamond.PPO
    kw = {k: z["cfg/" + k].item() for k in ("num_epochs", "num_minibatches", "lr", "adam_eps",
                                             "gamma", "gae_lambda", "ppo_clip",
                                             "value_loss_weight", "entropy_beta",
                                             "grad_norm_clip", "total_steps")}
    cfg = Cfg(rollout_steps=T, num_envs=Nn, verbose=False,
              advantage_norm=bool(z["cfg/advantage_norm"]), decay_lr=bool(z["cfg/decay_lr"]), **kw)
    envs = gym_stub.SyncVectorEnv([lambda: gym_stub.SyntheticEnv(D, A, continuous=bool(cont),
                                                                 act_dim=A)] * Nn)
    agent = Agent(None, cfg, network_cls=CustomNet, envs=envs)
    assert not agent._learner.fused
    agent.fused_loss = fused_loss
    sd = {n: torch.from_numpy(z["init/" + n]) for n in z["param_names"]}
    if hasattr(agent.network, "actor_out_layer"):
        sd["actor_out_layer.weight"] = sd["actor_head.2.weight"]
        sd["actor_out_layer.bias"] = sd["actor_head.2.bias"]
    agent.network.load_state_dict(sd)
    return agent, n_learn


def _learn_all(z, agent, n_learn):
    for li in range(n_learn):
        np.random.set_state(("MT19937", z[f"rng_state_before{li}"].astype(np.uint32),
                             int(z[f"rng_pos_before{li}"]), 0, 0.0))
        agent.learn(experience(z, li))
        torch.cuda.synchronize()
    return np.concatenate([p.detach().cpu().numpy().ravel() for p in agent.network.parameters()])


@pytest.mark.parametrize("name", ["cartpole_small", "cheetah_small"])
def test_generic_path_with_fused_loss_matches_reference_trace(name):
    z = load_golden(f"learn_{name}.npz")
    agent, n_learn = _custom_agent(z, True)
    _learn_all(z, agent, n_learn)
    E, M = agent.cfg.num_epochs, agent.cfg.num_minibatches
    assert agent._learner.loss_head_calls == n_learn * E * M     # the kernel ran
    for n, p in agent.network.named_parameters():
        d = np.abs(p.detach().cpu().numpy() - z["final/" + n]).max()
        print(name, n, "max|param - reference|", d)
        np.testing.assert_allclose(p.detach().cpu().numpy(), z["final/" + n], rtol=0, atol=5e-6,
                                   err_msg=n)


@pytest.mark.parametrize("name", ["cartpole_small", "cheetah_small"])
def test_two_fused_loss_learns_from_one_state_are_bit_identical(name):
    z = load_golden(f"learn_{name}.npz")
    runs = []
    for _ in range(2):
        agent, _ = _custom_agent(z, True)
        runs.append(_learn_all(z, agent, 1))
    assert runs[0].tobytes() == runs[1].tobytes()


@pytest.mark.parametrize("name", ["cartpole_small", "cheetah_small"])
def test_flag_off_never_calls_the_kernel(name):
    z = load_golden(f"learn_{name}.npz")
    agent, _ = _custom_agent(z, False)
    _learn_all(z, agent, 1)
    assert agent._learner.loss_head_calls == 0


def test_recurrent_torch_loop_with_fused_loss_matches_oracle():
    """gru_cases' tiny case, fused_gru = False, fused_loss = True: the torch path's bound of
    test_gpu_gru_learn.py -- 3e-5 on parameters against oracle/gru_torch.learn (2e-5 for 4 steps
    of lr 3e-4, grown to this case's 6 steps), m within 1e-3 and v within 2e-3 of their largest
    entry."""
    name = "tiny"
    (T, Nn, D, A), kw, seeds, _, _ = GL.CASES[name]
    import gym_stub
    envs = gym_stub.SyncVectorEnv([lambda: gym_stub.SyntheticEnv(D, A)] * Nn)
    agent = diamond.RecurrentPPO(None, GL._config(name), envs=envs)
    agent.fused_gru = False
    agent.fused_loss = True
    names = [n for n, _ in agent.network.named_parameters()]
    init = gru_cases.initial_params(D, A, agent.cfg.seed)
    for n, p in agent.network.named_parameters():
        assert np.array_equal(p.detach().cpu().numpy(), init[n]), n
    for call, ref in enumerate(GL._oracle(name)):
        np.random.seed(5 + call)
        agent.learn(GL._experience(name, call, agent.device))
        torch.cuda.synchronize()
        assert agent.optimizer.param_groups[0]["lr"] == ref["lr_after"]
    steps = kw["num_epochs"] * kw["num_minibatches"] * len(seeds)
    assert agent.loss_head_calls == steps
    ref = GL._oracle(name)[-1]
    flat = lambda d: np.concatenate([d[n].ravel() for n in names])
    mine = lambda buf: np.concatenate([v.cpu().numpy().ravel() for v in agent.flat.views(buf)])
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    dp = float(np.abs(mine(agent.flat.flat) - flat(ref["params"])).max())
    dm, dv = rel(mine(agent.m), flat(ref["m"])), rel(mine(agent.v), flat(ref["v"]))
    print(f"tiny fused_loss: max|param - oracle| {dp:.2e}, m {dm:.2e}, v {dv:.2e}")
    grown = 2e-5 * max(1.0, steps * kw.get("lr", 3e-4) / (4 * 3e-4))
    assert abs(grown - 3e-5) < 1e-12
    assert dp <= grown and dm <= 1e-3 and dv <= 2e-3, (dp, dm, dv)
