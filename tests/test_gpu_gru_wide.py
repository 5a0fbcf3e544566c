"""The fused RecurrentPPO minibatch kernel per width (csrc/grugrad.hip behind
dppo_gru_minibatch_grad_f32) against the float64 autograd oracle (oracle/gru_torch.py), on the
cases of tests/gru_wide_cases.py: at gru_hidden_dim 32 and 64 tests/gru_cases.py's edge cases
rebuilt per G; env counts around the kernel's envs per workgroup (16 at G = 16, 8 at G = 32, 4 at
G = 64); and LONG_CASES: workgroups whose T * ne samples take two and three passes of the 256
threads (full and partial ones), S = 256 exactly, and 1030 envs (65 / 129 / 258 gradient slabs),
under the same bounds.  (G = 16 on gru_cases.CASES themselves: tests/test_gpu_gru.py.)

Tolerances, the project's bound for this kernel (tests/test_gpu_gru.py): per tensor
max|diff| <= 2e-5 x max|g|, loss sums rtol 1e-5 and atol 1e-5 m.  Every case also checks that the
agent took the fused path at all, a repeat call bit for bit, and that m = 0 on the same handle
(scratch full of the call before) returns exact zeros."""
from dataclasses import replace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diamond
import gru_wide_cases as W
from oracle import gru_torch as GT

from test_gpu_gru import _kernel_grad


def _agent(T, Nn, D, A, G, **kw):
    import gym_stub
    np.random.seed(0)
    torch.manual_seed(0)
    envs = gym_stub.SyncVectorEnv([lambda: gym_stub.SyntheticEnv(D, A)] * Nn)
    cfg = diamond.RecurrentPPOConfig(rollout_steps=T, num_envs=Nn, verbose=False,
                                     gru_hidden_dim=G, **kw)
    return diamond.RecurrentPPO(None, cfg, envs=envs)


_case_agents = {}


def _case_agent(case, params):
    """One agent per (G, shape), shared by the cases (each loads its own weights; whatever an
    earlier case left in the handle's scratch must not show)."""
    key = (case.G, case.shape)
    if key not in _case_agents:
        _case_agents[key] = _agent(*case.shape, case.G)
    agent = _case_agents[key]
    assert agent.gru is not None, "gru_hidden_dim %d did not take the fused path" % case.G
    assert agent.gru.dims.gru_hidden == case.G
    with torch.no_grad():
        for n, p in agent.network.named_parameters():
            p.copy_(torch.from_numpy(params[n]))
    return agent


def _slices(L, g, ref):
    return {n: g[L.offset[i]:L.offset[i] + L.numel[i]].reshape(ref[n].shape)
            for i, n in enumerate(GT.GRU_NAMES)}


def _check_case(case):
    """The kernel on one case against the float64 oracle; returns what the long cases go on with."""
    params, x, mb_idx, m_total = W.build(case)
    W.guards(case, params, x, mb_idx)
    agent = _case_agent(case, params)
    L, m = agent.gru.layout, len(mb_idx)
    args = (mb_idx, m_total, case.clip, case.vf, case.ent)
    grad = _kernel_grad(agent, x, *args)
    g = grad.cpu().numpy()
    sums, ref = GT.minibatch_grads(params, x["obs"], x["actions"], x["old_log_probs"],
                                   x["advantages"], x["returns"], x["prev_dones"], x["hx0"],
                                   *args)
    scale = max(np.abs(r).max() for r in ref.values())
    worst = 0.0
    for i, n in enumerate(GT.GRU_NAMES):
        got = g[L.offset[i]:L.offset[i] + L.numel[i]].reshape(ref[n].shape)
        worst = max(worst, np.abs(got - ref[n]).max() / scale)
    print(f"{case}: max|diff| / max|g| = {worst:.2e} (max|g| {scale:.2e})")
    for i, n in enumerate(GT.GRU_NAMES):
        got = g[L.offset[i]:L.offset[i] + L.numel[i]].reshape(ref[n].shape)
        err = np.abs(got - ref[n]).max()
        assert err <= 2e-5 * scale, (n, err, scale)
    np.testing.assert_allclose(g[L.total:L.total + 3], sums, rtol=1e-5, atol=1e-5 * m)
    # deterministic: the same call twice gives the same bits
    assert torch.equal(_kernel_grad(agent, x, *args), grad)
    # m = 0 on the scratch this call left: every entry and the three loss sums exactly 0
    if m > 1:
        assert torch.count_nonzero(grad[:L.total + 3]).item() > L.total // 2
    for m_tot in (1, m_total):
        empty = _kernel_grad(agent, x, mb_idx[:0], m_tot, case.clip, case.vf, case.ent)
        assert torch.count_nonzero(empty).item() == 0
    if case.dones == "first":
        # every env starts the rollout reset: hx0 has no effect and gets no gradient
        x2 = dict(x, hx0=np.random.default_rng(11).standard_normal(x["hx0"].shape)
                  .astype(np.float32) * 2)
        assert np.abs(x2["hx0"] - x["hx0"]).min() > 0
        assert torch.equal(_kernel_grad(agent, x2, *args), grad)
    if case.pick is not None:
        # the recurrent weights see the sample through every earlier step, or through none: with
        # no dones and t = T-1 the oracle's Whh gradient is dense; at t = 0 it is the one outer
        # product with the initial hidden state -- and so is the kernel's
        whh = ref["gru.weight_hh_l0"]
        assert np.count_nonzero(whh) == whh.size
        rank = np.linalg.matrix_rank(whh, tol=1e-12 * np.abs(whh).max())
        assert rank == 1 if case.pick[0] == 0 else rank > 1
    return params, x, mb_idx, m_total, g, ref, worst


@pytest.mark.parametrize("case", W.CASES, ids=str)
def test_wide_gru_minibatch_gradient(case):
    _check_case(case)


@pytest.mark.parametrize("case", W.LONG_CASES, ids=str)
def test_wide_gru_minibatch_gradient_long(case):
    """More than one pass per workgroup, many slabs (tests/gru_wide_cases.py LONG_CASES)."""
    import regime_cases as R
    params, x, mb_idx, m_total, g, ref, worst = _check_case(case)
    _, err32 = R.gru_oracle_pair(case, params, x, mb_idx, m_total)
    print(f"{case}: err_kernel {worst:.2e} err_oracle32 {err32:.2e} m {len(mb_idx)}")
    if case.shape != W.MANY_ENVS or case.frac != 1.0 or case.on_policy:
        return
    # A full last workgroup and a partial one give the same per-env contribution: the first 1024
    # envs alone (every workgroup full), with the divisor of the whole batch, against the oracle
    # on that slice; and what the last 6 envs add is the oracle's difference of the two.
    T, Nn, D, A = case.shape
    H = W.MANY_ENVS_HEAD
    head = dict({k: np.ascontiguousarray(v[:, :H]) for k, v in x.items() if k != "hx0"},
                hx0=x["hx0"][:H])
    idx = np.arange(T * H, dtype=np.int32)
    agent = _case_agent(replace(case, shape=(T, H, D, A)), params)
    args = (idx, m_total, case.clip, case.vf, case.ent)
    gh = _kernel_grad(agent, head, *args).cpu().numpy()
    L = agent.gru.layout
    sums_h, ref_h = GT.minibatch_grads(params, head["obs"], head["actions"], head["old_log_probs"],
                                       head["advantages"], head["returns"], head["prev_dones"],
                                       head["hx0"], *args)
    scale = max(np.abs(r).max() for r in ref.values())
    scale_h = max(np.abs(r).max() for r in ref_h.values())
    got, got_h = _slices(L, g, ref), _slices(L, gh, ref_h)
    for n in GT.GRU_NAMES:
        assert np.abs(got_h[n] - ref_h[n]).max() <= 2e-5 * scale_h, n
        # two fp32 sums (2060 and 2048 samples), each within 2e-5 of its own oracle's scale
        tail = np.abs((got[n] - got_h[n]) - (ref[n] - ref_h[n])).max()
        assert tail <= 2e-5 * (scale + scale_h), (n, tail, scale)
        assert np.abs(ref[n] - ref_h[n]).max() > 0
    np.testing.assert_allclose(gh[L.total:L.total + 3], sums_h, rtol=1e-5, atol=1e-5 * len(idx))
