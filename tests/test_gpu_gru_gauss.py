"""The fused RecurrentContinuousPPO minibatch kernel (csrc/grugrad.hip's
gru_grad_kernel<G, WIDE_OBS, true> behind dppo_gru_gauss_minibatch_grad_f32) against the float64
autograd yardstick tests/gru_gauss_oracle.py on the cases of tests/gru_gauss_cases.py, under the
bound of tests/test_gpu_gru.py: per tensor (actor_log_std a tensor of its own) max|diff| <=
2e-5 x max|g|, loss sums rtol 1e-5 and atol 1e-5 m, a repeat call bit for bit, m = 0 exact zeros.
Every case prints its max|diff| / max|g| over all tensors and for actor_log_std alone, with the
float32 oracle's own figures beside them."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diamond
import gru_gauss_cases as C
import gru_gauss_oracle as GO
from diamond import _native as N


def _agent(T, Nn, D, A, G, **kw):
    import gym_stub
    np.random.seed(0)
    torch.manual_seed(0)
    envs = gym_stub.SyncVectorEnv(
        [lambda: gym_stub.SyntheticEnv(D, continuous=True, act_dim=A)] * Nn)
    cfg = diamond.RecurrentContinuousPPOConfig(rollout_steps=T, num_envs=Nn, verbose=False,
                                               gru_hidden_dim=G, **kw)
    return diamond.RecurrentContinuousPPO(None, cfg, envs=envs)


def _kernel_grad(agent, x, mb_idx, m_total, clip, vf, ent):
    """One dppo_gru_gauss_minibatch_grad_f32 launch on the agent's parameters: the flat gradient
    with the three loss sums behind it, as a device tensor."""
    dev = agent.device
    m = len(mb_idx)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in x.items()}
    t["prev_dones"] = t["prev_dones"].to(torch.uint8)
    assert t["actions"].dtype == torch.float32
    batch = N.GruGaussBatch(*[t[k].data_ptr() for k in ("obs", "actions", "old_log_probs",
                                                           "advantages", "returns", "prev_dones",
                                                           "hx0")])
    idx = torch.from_numpy(mb_idx if m else np.zeros(1, np.int32)).to(dev)
    hp = N.HParams(gamma=0.99, gae_lambda=0.95, ppo_clip=clip, value_loss_weight=vf,
                   entropy_beta=ent, grad_norm_clip=0.5, adam_beta1=0.9, adam_beta2=0.999,
                   adam_eps=1e-5, advantage_norm=1, lr=3e-4, adam_step=0)
    grad = torch.zeros(agent.gru.layout.total + 8, device=dev)
    N.check(agent.gru.lib.dppo_gru_gauss_minibatch_grad_f32(
        agent.gru.h, agent.flat.flat.data_ptr(), ctypes.byref(batch), idx.data_ptr(), m, m_total,
        ctypes.byref(hp), grad.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return grad


_agents = {}


def _case_agent(case, params):
    """One agent per (G, shape), shared by the cases: each loads its own weights, and whatever an
    earlier case left in the handle's scratch must not show."""
    key = (case.G, case.shape)
    if key not in _agents:
        _agents[key] = _agent(*case.shape, case.G, wide_observations=case.wide_obs)
    agent = _agents[key]
    assert agent.gru is not None and agent.gru.gauss
    assert agent.gru.dims.wide_obs == int(case.wide_obs)
    with torch.no_grad():
        for n, p in agent.network.named_parameters():
            p.copy_(torch.from_numpy(params[n]))
    return agent


def _args(x, mb_idx, m_total, case):
    return (x["obs"], x["actions"], x["old_log_probs"], x["advantages"], x["returns"],
            x["prev_dones"], x["hx0"], mb_idx, m_total, case.clip, case.vf, case.ent)


def _check_case(case):
    params, x, mb_idx, m_total = C.build(case)
    C.guards(case, params, x, mb_idx)
    agent = _case_agent(case, params)
    L = agent.gru.layout
    assert [n for n, _ in agent.network.named_parameters()] == GO.PARAM_NAMES
    grad = _kernel_grad(agent, x, mb_idx, m_total, case.clip, case.vf, case.ent)
    g = grad.cpu().numpy()
    sums, ref = GO.minibatch_grads(params, *_args(x, mb_idx, m_total, case))
    _, ref32 = GO.minibatch_grads(params, *_args(x, mb_idx, m_total, case), dt=torch.float32)
    scale = max(np.abs(r).max() for r in ref.values())
    err, err32 = {}, {}
    for i, n in enumerate(GO.PARAM_NAMES):
        got = g[L.offset[i]:L.offset[i] + L.numel[i]].reshape(ref[n].shape)
        err[n] = np.abs(got - ref[n]).max() / scale
        err32[n] = np.abs(ref32[n].astype(np.float64) - ref[n]).max() / scale
    worst, worst32 = max(err.values()), max(err32.values())
    print(f"{case}: m {len(mb_idx)} err_kernel {worst:.2e} (log_std {err['actor_log_std']:.2e}) "
          f"err_oracle32 {worst32:.2e} (log_std {err32['actor_log_std']:.2e})")
    for n in GO.PARAM_NAMES:
        assert err[n] <= 2e-5, (n, err[n], scale)
    assert np.abs(ref["actor_log_std"]).max() > 0
    np.testing.assert_allclose(g[L.total:L.total + 3], sums, rtol=1e-5, atol=1e-5 * len(mb_idx))
    # the layout's padding floats and the unused loss slots stay zero
    used = np.zeros(L.total + 8, bool)
    for i in range(L.count):
        used[L.offset[i]:L.offset[i] + L.numel[i]] = True
    used[L.total:L.total + 3] = True
    assert not g[~used].any()
    # deterministic: the same call twice gives the same bits
    assert torch.equal(grad, _kernel_grad(agent, x, mb_idx, m_total, case.clip, case.vf, case.ent))
    return agent, x, mb_idx, m_total, grad


@pytest.mark.parametrize("case", C.CASES, ids=str)
def test_gauss_gru_minibatch_gradient(case):
    _check_case(case)


@pytest.mark.parametrize("G", C.WIDTHS)
def test_gauss_gru_empty_selection_after_full_batch(G):
    """m = 0 on a handle whose scratch holds a full-batch call: every gradient entry, actor_log_std's
    entropy term included, and the three loss sums are exactly 0."""
    case = next(c for c in C.CASES if c.G == G and c.regime == "spread"
                and c.shape == C.shapes(G)[1] and c.frac == 1.0 and not c.on_policy
                and c.clip == 0.15)
    agent, x, mb_idx, m_total, full = _check_case(case)
    total = agent.gru.layout.total
    assert torch.count_nonzero(full[:total + 3]).item() > total // 2
    assert torch.count_nonzero(full[:case.shape[3]]).item() == case.shape[3]
    for m_tot in (1, len(mb_idx)):
        empty = _kernel_grad(agent, x, mb_idx[:0], m_tot, case.clip, case.vf, case.ent)
        assert torch.count_nonzero(empty).item() == 0


def test_gauss_gru_two_halves_sum_to_the_union_minibatch():
    """What the data-parallel all-reduce relies on: two disjoint selections, each divided by the
    union's size, sum to the union's gradient, the entropy bonus's -ent per log_std dimension
    once."""
    case = next(c for c in C.CASES if c.G == 16 and c.regime == "spread"
                and c.shape == C.shapes(16)[1] and c.frac == 1.0 and not c.on_policy
                and c.clip == 0.15)
    params, x, mb_idx, _ = C.build(case)
    agent = _case_agent(case, params)
    m = len(mb_idx)
    a, b = mb_idx[:m // 2], mb_idx[m // 2:]
    kw = (case.clip, case.vf, case.ent)
    ga, gb = _kernel_grad(agent, x, a, m, *kw), _kernel_grad(agent, x, b, m, *kw)
    gu = _kernel_grad(agent, x, mb_idx, m, *kw)
    total, A = agent.gru.layout.total, case.shape[3]
    s = (ga + gb).cpu().numpy()
    u = gu.cpu().numpy()
    assert np.abs(s[:total] - u[:total]).max() <= 2e-6 * np.abs(u[:total]).max()
    _, ref = GO.minibatch_grads(params, *_args(x, mb_idx, m, case))
    scale = max(np.abs(r).max() for r in ref.values())
    assert np.abs(s[:A] - ref["actor_log_std"].reshape(-1)).max() <= 2e-5 * scale
