"""RecurrentPPO.learn() at gru_hidden_dim 32 and 64 against oracle/gru_torch.py's learn(): the
comparisons and tolerances of tests/test_gpu_gru_learn.py on (T, N, D, A) = (8, 20, 6, 3) with
2 epochs x 2 minibatches, and per G on a shape whose full workgroups hold more samples than the
gradient kernel's 256 threads take in one pass -- (40, 9, 6, 3) at 32, (72, 5, 6, 3) at 64, each
with a 1-env last workgroup -- with 2 epochs x 3 minibatches; two learn() calls under a decaying
LR (8 / 12 Adam steps at lr <= 3e-4).  Both of the agent's paths -- the fused kernel
(fused_gru=True, csrc/grugrad.hip) and torch autograd (fused_gru=False) -- are compared with the
oracle; then with each other under the bound of test_recurrent_learn_fused_matches_torch_path.

Per learn() call, fused path: the returns == values + ppo_np.gae bit for bit, the normalised
advantages within 2e-6 of the oracle's, the minibatch indices, the Adam step and the LR handed to
the update; last_losses within rtol 1e-5 + atol 1e-5.  Both paths: the LR after the call.  At the
end, parameters: the fused path within max(2e-5, 2 x the torch path's deviation); the torch path
within 2e-5 grown in proportion to steps x lr over the 4 steps of lr 3e-4 that bound was set for
(4e-5 at 8 steps, 6e-5 at 12).  Adam m and v relative to their largest entry: floors 1e-3 and 2e-3.

Measured on an MI355X, max|param - oracle| (parameters moved by 2.0e-3 / 3.1e-3), torch path then
fused path: (8, 20, 6, 3) 3.0e-8 / 3.0e-8 at both G; (40, 9, 6, 3) G 32 3.0e-8 / 3.0e-8;
(72, 5, 6, 3) G 64 3.0e-8 / 6.0e-8.  m 0.9e-7 .. 1.4e-7 and v 1.3e-5 of their largest entry on
either path, every shape: float32 autograd meets the bound set at T = 8 at the long shapes too,
so it stands unchanged."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diamond
import gru_wide_cases as W
from oracle import gru_torch as GT
from oracle import ppo_np

SHAPE = (8, 20, 6, 3)
# per G, a shape whose full workgroups (8 / 4 envs) hold 320 / 288 samples, more than one pass of
# the kernel's 256 threads, with a 1-env last workgroup and minibatches of a third of the batch
LONG_SHAPE = {32: (40, 9, 6, 3), 64: (72, 5, 6, 3)}
CASES = [(G, SHAPE) for G in W.WIDTHS] + [(G, LONG_SHAPE[G]) for G in W.WIDTHS]
SEEDS = (3, 4)      # one rollout, one learn() each


def _id(case):
    G, shape = case
    return str(G) if shape == SHAPE else f"{G}-" + "x".join(map(str, shape))


def _kw(shape):
    return dict(num_epochs=2, num_minibatches=2 if shape == SHAPE else 3, decay_lr=True,
                total_steps=3 * shape[0] * shape[1])


def _config(G, shape):
    return diamond.RecurrentPPOConfig(rollout_steps=shape[0], num_envs=shape[1], verbose=False,
                                      gru_hidden_dim=G, **_kw(shape))


def _experience(G, shape, call, device):
    from dist_scripts.recurrent_dp import synth_experience
    return synth_experience(*shape, G, device, seed=SEEDS[call])


def _perms(shape, call):
    rs = np.random.RandomState(5 + call)     # as np.random.seed(5 + call) before agent.learn
    return np.stack([rs.permutation(shape[0] * shape[1])
                     for _ in range(_kw(shape)["num_epochs"])])


@functools.lru_cache(maxsize=None)
def _oracle(G, shape):
    """The oracle's learn() calls, computed once and shared by both paths."""
    cfg = _config(G, shape)
    params = W.initial_params(shape[2], shape[3], G, cfg.seed)
    adam = ppo_np.new_adam_state(params, GT.GRU_NAMES)
    lr, calls = cfg.lr, []
    for call in range(len(SEEDS)):
        x = GT.stack_experience(_experience(G, shape, call, "cpu"))
        out = GT.learn(params, adam, x, cfg, lr, _perms(shape, call))
        raw = ppo_np.gae(x["rewards"], x["terms"], x["truncs"], x["values"], x["next_values"],
                         cfg.gamma, cfg.gae_lambda)
        lr_used, lr = lr, GT.lr_after_learn(lr, call + 1, cfg)
        calls.append(dict(out, x=x, raw_adv=raw, lr_used=lr_used, lr_after=lr,
                          step_before=adam["step"] - len(out["losses"]),
                          params={n: v.copy() for n, v in params.items()},
                          m={n: v.copy() for n, v in adam["m"].items()},
                          v={n: v.copy() for n, v in adam["v"].items()}))
    return calls


@functools.lru_cache(maxsize=None)
def _run(G, shape, fused):
    """The agent's learn() calls on one path, each checked against the oracle's; returns the final
    deviations (parameters absolute; m, v relative to their largest entry) and the final flat
    parameters and first moments."""
    import gym_stub
    T, Nn, D, A = shape
    envs = gym_stub.SyncVectorEnv([lambda: gym_stub.SyntheticEnv(D, A)] * Nn)
    agent = diamond.RecurrentPPO(None, _config(G, shape), envs=envs)
    assert agent.gru is not None, "gru_hidden_dim %d did not take the fused path" % G
    agent.fused_gru = fused
    names = [n for n, _ in agent.network.named_parameters()]
    assert names == GT.GRU_NAMES
    init = W.initial_params(D, A, G, agent.cfg.seed)
    for n, p in agent.network.named_parameters():
        assert np.array_equal(p.detach().cpu().numpy(), init[n]), n
    captured = []
    inner = agent._learn_fused

    def capture(observations, actions, log_probs, advantages, returns, prev_dones, hx, idx, step,
                lr, *rest):
        captured.append(dict(adv=advantages.cpu().numpy().copy(), ret=returns.cpu().numpy().copy(),
                             idx=idx.cpu().numpy().copy(), step=step, lr=lr))
        return inner(observations, actions, log_probs, advantages, returns, prev_dones, hx, idx,
                     step, lr, *rest)

    agent._learn_fused = capture
    for call, ref in enumerate(_oracle(G, shape)):
        exp = _experience(G, shape, call, agent.device)
        np.random.seed(5 + call)
        agent.learn(exp)
        torch.cuda.synchronize()
        assert agent.optimizer.param_groups[0]["lr"] == ref["lr_after"]
        if not fused:
            assert not captured
            continue
        got = captured.pop()
        assert not captured
        x = ref["x"]
        assert np.array_equal(got["ret"], (x["values"] + ref["raw_adv"]).reshape(-1))
        d_adv = np.abs(got["adv"] - ref["adv"].reshape(-1)).max()
        print(f"G={G} {shape} call {call}: max|adv - oracle| {d_adv:.2e}")
        assert d_adv <= 2e-6
        assert np.array_equal(got["idx"], ref["idx"])
        assert got["step"] == ref["step_before"] and got["lr"] == ref["lr_used"]
        losses = agent.last_losses.cpu().numpy()
        assert losses.shape == ref["losses"].shape
        np.testing.assert_allclose(losses, ref["losses"], rtol=1e-5, atol=1e-5)
    ref = _oracle(G, shape)[-1]
    # the LR did decay across the calls
    assert ref["lr_after"] < ref["lr_used"] < _config(G, shape).lr
    flat = lambda d: np.concatenate([d[n].ravel() for n in names])
    mine = lambda buf: np.concatenate([v.cpu().numpy().ravel() for v in agent.flat.views(buf)])
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    dev = dict(p=float(np.abs(mine(agent.flat.flat) - flat(ref["params"])).max()),
               m=rel(mine(agent.m), flat(ref["m"])), v=rel(mine(agent.v), flat(ref["v"])))
    moved = np.abs(flat(ref["params"]) - flat(init)).max()
    assert moved > 1e-4          # the update itself is far above every bound below
    print(f"G={G} {shape} fused={fused}: max|param - oracle| {dev['p']:.2e} (moved {moved:.1e}), "
          f"m {dev['m']:.2e}, v {dev['v']:.2e}")
    return dev, mine(agent.flat.flat), mine(agent.m)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_wide_recurrent_learn_matches_oracle(case, fused):
    G, shape = case
    KW = _kw(shape)
    torch_dev = _run(G, shape, False)[0]
    dev = _run(G, shape, fused)[0]
    if fused:
        bound = dict(p=max(2e-5, 2 * torch_dev["p"]), m=max(1e-3, 2 * torch_dev["m"]),
                     v=max(2e-3, 2 * torch_dev["v"]))
    else:
        steps = KW["num_epochs"] * KW["num_minibatches"] * len(SEEDS)
        bound = dict(p=2e-5 * max(1.0, steps * 3e-4 / (4 * 3e-4)), m=1e-3, v=2e-3)
    for k in ("p", "m", "v"):
        assert dev[k] <= bound[k], (k, dev[k], bound[k], torch_dev[k])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_wide_recurrent_learn_fused_matches_torch_path(case):
    """The two paths end with the same parameters and first moments
    (test_recurrent_learn_fused_matches_torch_path's bounds)."""
    _, p1, m1 = _run(*case, True)
    _, p2, m2 = _run(*case, False)
    assert np.abs(p1 - p2).max() <= 2e-5
    np.testing.assert_allclose(m1, m2, rtol=1e-3, atol=1e-7)
