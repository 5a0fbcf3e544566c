"""RecurrentPPO with ``fused_core`` (every GRUCore of the network on the GRU scan kernels,
csrc/gruseq.hip) at shapes the fused GRU class turns down, so learn() runs its torch loop and
rollout() its torch path.

learn(): two calls under decay_lr, 2 epochs x 3 minibatches, T = 8, N = 9, against
oracle/gru_torch.py::learn on the same experience and permutations -- the flag-on agent and the
flag-off agent each against the oracle, never against each other -- at the bounds
tests/test_gpu_gru_learn.py sets for the torch path: parameters within 2e-5 grown in proportion to
steps x lr over its 4 steps of 3e-4 (12 steps here: 6e-5), Adam m within 1e-3 and v within 2e-3 of
their largest entry, the LR after each call equal, and (flag on, which records them) the
minibatches' {loss, policy, value, entropy} within rtol 1e-5 + atol 1e-5.

Then the call counts, the composition with ``fused_loss``, the precedence of ``fused_gru`` at the
class's default shape, a network class of the user's own, and rollout().
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diamond
import gru_core_cases as C
from dist_scripts.recurrent_dp import synth_experience
from oracle import gru_torch as GT
from oracle import ppo_np

E, M = 2, 3
SEEDS = (3, 4)          # one learn() each
KW = dict(num_epochs=E, num_minibatches=M, decay_lr=True, total_steps=3 * C.T * C.NENVS)
STEPS = E * M * len(SEEDS)
P_BOUND = 2e-5 * max(1.0, STEPS * 3e-4 / (4 * 3e-4))
M_BOUND, V_BOUND = 1e-3, 2e-3


def _experience(shape, call, device):
    _, G, D, A = shape
    return synth_experience(C.T, C.NENVS, D, A, G, device, seed=SEEDS[call])


def _perms(call):
    rs = np.random.RandomState(5 + call)     # as np.random.seed(5 + call) before agent.learn
    return np.stack([rs.permutation(C.T * C.NENVS) for _ in range(E)])


@functools.lru_cache(maxsize=None)
def _oracle(name):
    shape = C.LEARN_SHAPES[name]
    cfg = C.config(shape, **KW)
    params = C.initial_params(shape, cfg)
    assert list(params) == GT.GRU_NAMES
    adam = ppo_np.new_adam_state(params, GT.GRU_NAMES)
    lr, calls = cfg.lr, []
    for call in range(len(SEEDS)):
        x = GT.stack_experience(_experience(shape, call, "cpu"))
        out = GT.learn(params, adam, x, cfg, lr, _perms(call))
        lr = GT.lr_after_learn(lr, call + 1, cfg)
        calls.append(dict(losses=out["losses"].copy(), lr_after=lr,
                          params={n: v.copy() for n, v in params.items()},
                          m={n: v.copy() for n, v in adam["m"].items()},
                          v={n: v.copy() for n, v in adam["v"].items()}))
    return calls


def _agent(shape, kw, core, loss=False, network_cls=None):
    extra = {} if network_cls is None else dict(network_cls=network_cls)
    agent = diamond.RecurrentPPO(None, C.config(shape, **kw), envs=C.make_envs(shape), **extra)
    agent.fused_core, agent.fused_loss = core, loss
    return agent


@functools.lru_cache(maxsize=None)
def _run(name, core, loss):
    """The agent's two learn() calls, each checked against the oracle's; returns the final
    deviations (parameters absolute; m, v relative to their largest entry)."""
    shape = C.LEARN_SHAPES[name]
    agent = _agent(shape, KW, core, loss)
    assert agent.gru is None                 # outside the fused GRU class: the torch loop
    names = [n for n, _ in agent.network.named_parameters()]
    assert names == GT.GRU_NAMES
    init = C.initial_params(shape, agent.cfg)
    for n, p in agent.network.named_parameters():
        assert np.array_equal(p.detach().cpu().numpy(), init[n]), n
    for call, ref in enumerate(_oracle(name)):
        exp = _experience(shape, call, agent.device)
        np.random.seed(5 + call)
        scans0, heads0 = agent.core_scan_calls, agent.loss_head_calls
        agent.learn(exp)
        torch.cuda.synchronize()
        assert agent.core_scan_calls - scans0 == (E * M if core else 0)
        assert agent.loss_head_calls - heads0 == (E * M if loss else 0)
        assert agent.optimizer.param_groups[0]["lr"] == ref["lr_after"]
        if not core:
            assert agent.last_losses is None
            continue
        losses = agent.last_losses.cpu().numpy()
        assert losses.shape == ref["losses"].shape
        d_loss = np.abs(losses - ref["losses"]) - 1e-5 * np.abs(ref["losses"])
        print(f"{name} call {call}: max(|loss - oracle| - 1e-5 |oracle|) {d_loss.max():.2e}")
        np.testing.assert_allclose(losses, ref["losses"], rtol=1e-5, atol=1e-5)
    ref = _oracle(name)[-1]
    flat = lambda d: np.concatenate([d[n].ravel() for n in names])
    mine = lambda buf: np.concatenate([v.cpu().numpy().ravel() for v in agent.flat.views(buf)])
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    dev = dict(p=float(np.abs(mine(agent.flat.flat) - flat(ref["params"])).max()),
               m=rel(mine(agent.m), flat(ref["m"])), v=rel(mine(agent.v), flat(ref["v"])))
    moved = np.abs(flat(ref["params"]) - flat(init)).max()
    assert moved > 1e-4          # the update itself is far above every bound below
    print(f"{name} fused_core={core} fused_loss={loss}: max|param - oracle| {dev['p']:.2e} "
          f"(moved {moved:.1e}), m {dev['m']:.2e}, v {dev['v']:.2e}")
    return dev


LEARN_CASES = [(name, core, False) for name in C.LEARN_SHAPES for core in (True, False)] \
    + [("h128-g32", True, True)]     # fused_loss on as well, at one shape


@pytest.mark.parametrize("name,core,loss", LEARN_CASES,
                         ids=[f"{n}-{'core' if c else 'torch'}{'+loss' if l else ''}"
                              for n, c, l in LEARN_CASES])
def test_learn_matches_oracle(name, core, loss):
    dev = _run(name, core, loss)
    assert dev["p"] <= P_BOUND and dev["m"] <= M_BOUND and dev["v"] <= V_BOUND, dev


def test_default_shape_still_takes_the_fused_learn():
    """fused_gru wins where it serves the agent: no GRUCore forward runs at all."""
    shape = C.DEFAULT_SHAPE
    agent = _agent(shape, dict(num_epochs=E, num_minibatches=M), core=True)
    assert agent.gru is not None and agent.fused_gru
    taken = []
    inner = agent._learn_fused
    agent._learn_fused = lambda *a: (taken.append(1), inner(*a))[1]
    np.random.seed(5)
    agent.learn(_experience(shape, 0, agent.device))
    torch.cuda.synchronize()
    assert taken == [1] and agent.core_scan_calls == 0
    assert agent.last_losses.shape == (E * M, 4)


def test_custom_network_class():
    """A two-layer base of hidden 96 around GRUCore(96, 16): one learn() with the flag on leaves
    the parameters within the torch path's bound for its 6 steps of lr 3e-4 of the flag-off
    agent's on the same inputs."""
    shape = (96, 16, 8, 4)
    kw = dict(num_epochs=E, num_minibatches=M)
    got = {}
    for core in (False, True):
        agent = _agent(shape, kw, core, network_cls=C.TwoLayerBaseNetwork)
        assert agent.gru is None
        start = agent.flat.flat.clone()
        np.random.seed(5)
        agent.learn(_experience(shape, 0, agent.device))
        torch.cuda.synchronize()
        assert agent.core_scan_calls == (E * M if core else 0)
        got[core] = (start, agent.flat.flat.clone())
    assert torch.equal(got[False][0], got[True][0])
    moved = float((got[False][1] - got[False][0]).abs().max())
    d = float((got[True][1] - got[False][1]).abs().max())
    print(f"custom network: max|on - off| {d:.2e}, moved {moved:.1e}")
    assert moved > 1e-4
    assert d <= 2e-5 * max(1.0, E * M * 3e-4 / (4 * 3e-4))


def _rollout(core, peaked):
    shape = C.ROLLOUT_SHAPE
    agent = _agent(shape, dict(rollout_steps=C.ROLLOUT_T), core)
    if peaked:
        C.peak_(agent.network)
    agent.current_observations, _ = agent.envs.reset(seed=C.ROLLOUT_ENV_SEED)
    agent.prev_dones = np.zeros(C.NENVS, dtype=bool)
    agent.current_hx = C.rollout_start(shape).to(agent.device)
    torch.manual_seed(123)
    exp = agent.rollout()
    torch.cuda.synchronize()
    assert agent.core_scan_calls == (2 * C.ROLLOUT_T if core else 0)
    col = lambda k: torch.stack([torch.as_tensor(row[k]) for row in exp]).cpu()
    return dict(obs=col(0), actions=col(1), prev_dones=col(5), log_probs=col(6), values=col(7),
                next_values=col(8), hx=col(9), last_hx=agent.current_hx.cpu(), agent=agent)


@pytest.mark.parametrize("peaked", [True, False], ids=["peaked", "initial"])
def test_rollout(peaked):
    """T = 4 with the flag on against the flag-off agent at equal weights and equal generator
    state.  The stub env's observations and resets do not depend on the actions, so values,
    next values and hidden states are comparable on every sample (2e-5).  Peaked policy (margins
    checked in float64 by tests/test_gru_core_cpu.py): every action is the float64 module's
    arg-max on both paths.  Initial policy (near-uniform, margins ~1e-4): log-probs are compared
    where the two paths drew the same action; both draw from the same generator state on logits
    ~1e-7 apart, so at most one of the 36 samples may differ."""
    off, on = _rollout(False, peaked), _rollout(True, peaked)
    assert torch.equal(off["obs"], on["obs"]) and torch.equal(off["prev_dones"], on["prev_dones"])
    for k in ("values", "next_values", "hx", "last_hx"):
        d = float((off[k] - on[k]).abs().max())
        print(f"rollout peaked={peaked} {k}: max|on - off| {d:.2e}")
        assert d <= 2e-5, (k, d)
    ref_logits, ref_hx = C.replica_logits(off["agent"].network, C.ROLLOUT_SHAPE)
    # the hidden state each step started from: row t + 1 is the float64 module's after step t
    for r in (off, on):
        d = float((r["hx"][1:].double() - ref_hx[:-1]).abs().max())
        assert d <= 2e-5, d
        assert float((r["last_hx"].double() - ref_hx[-1]).abs().max()) <= 2e-5
    same = off["actions"] == on["actions"]
    if peaked:
        assert C.action_margins(ref_logits).min() >= C.PEAK_MARGIN
        assert torch.equal(off["actions"], ref_logits.argmax(-1))
        assert torch.equal(on["actions"], ref_logits.argmax(-1))
    else:
        assert int((~same).sum()) <= 1
    d = float((off["log_probs"] - on["log_probs"])[same].abs().max())
    print(f"rollout peaked={peaked} log_probs: max|on - off| {d:.2e} on {int(same.sum())} samples")
    assert d <= 2e-5
