"""RecurrentPPO's fused rollout step at observations of 33 to 128 floats (csrc/gruact.hip's
gru_act_kernel<G, 128> / gru_value_kernel<G, 128> behind dppo_gru_act_f32 / dppo_gru_value_f32,
asked for with RecurrentPPOConfig.wide_observations) and the rollout() path on it:
tests/test_gpu_gru_wide_act.py's comparisons with the same yardstick (the float64 CPU module), the
same bounds (atol 2e-5, rtol 1e-5) and the same NumPy restatement of the Philox stream, which
must not depend on the observation width."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gru_torch as GT

import test_gpu_gru_act as base
from test_gpu_gru_act import (ATOL, M32, RTOL, _inputs, _oracle_net, log_softmax64, oracle_step,
                              oracle_value, run_act, run_value)
from test_gpu_rollout_ckpt import philox4x32_10, u01

WIDTHS = (16, 32, 64)
ENVS_PER_WG = 4
BIG = 4101          # 1025 full workgroups and one env

_agents = {}


def _agent(G, D, A, T=2, Nn=4):
    key = (G, D, A, T, Nn)
    if key not in _agents:
        _agents[key] = base._agent(T, Nn, D, A, G=G, wide_observations=True)
    agent = _agents[key]
    assert agent.gru.dims.obs_dim == D > 32 and agent.gru.dims.wide_obs == 1
    return agent


# ---- 1. one step against the float64 module
@pytest.mark.parametrize("G", WIDTHS)
@pytest.mark.parametrize("D", [33, 64, 100, 128])
@pytest.mark.parametrize("A", [2, 16])
@pytest.mark.parametrize("n", [1, ENVS_PER_WG + 1, BIG])
def test_one_step_matches_float64_module(G, n, D, A):
    agent = _agent(G, D, A)
    net = _oracle_net(agent)
    obs, mixed, hx = _inputs(n, D, seed=n * 10 + A, G=G)
    nobs = np.random.default_rng(n).standard_normal((n, D)).astype(np.float32)
    close = lambda got, want, what: np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL,
                                                               err_msg=what)
    for tag, dones in (("mixed", mixed), ("all", np.ones(n, bool)), ("none", np.zeros(n, bool))):
        got = run_act(agent, obs, dones, hx, seed=5, counter=3)
        lg, v, h = oracle_step(net, obs, dones, hx)
        assert h.shape == (n, G)
        close(got["logits"], lg, tag + " logits")
        close(got["values"], v, tag + " values")
        close(got["hx_out"], h, tag + " hx_out")
        act = got["actions"]
        assert act.dtype == np.int32 and act.min() >= 0 and act.max() < A
        close(got["log_probs"], log_softmax64(lg)[np.arange(n), act], tag + " log_probs")
        # V(next_obs) from the step's new hidden state, without and with a reset
        close(run_value(agent, nobs, got["hx_out"]), oracle_value(net, nobs, got["hx_out"]),
              tag + " next values")
        close(run_value(agent, nobs, hx, dones), oracle_value(net, nobs, hx, dones),
              tag + " values with dones")
        # the logits are optional
        lean = run_act(agent, obs, dones, hx, seed=5, counter=3, logits=False)
        for k in ("hx_out", "actions", "log_probs", "values"):
            assert np.array_equal(lean[k], got[k]), (tag, k)


# ---- 2. the draws are the documented Philox stream, whatever D
@pytest.mark.parametrize("G", WIDTHS)
@pytest.mark.parametrize("D", [33, 128])
def test_draws_are_the_documented_philox_stream(G, D):
    """actions = inverse CDF of the ORACLE's softmax at u01(c0) of Philox4x32-10 (key = seed,
    counter = {i lo, i hi, ctr lo, ctr hi}), compared exactly where u is more than 1e-5 from every
    CDF boundary (test_gpu_gru_wide_act.py: a sample misses that margin with probability
    <= 15 x 2e-5, against an allowance of 1 %)."""
    n, A = BIG, 16
    agent = _agent(G, D, A)
    net = _oracle_net(agent)
    obs, dones, hx = _inputs(n, D, seed=11, G=G)
    seed, counter = 0x1234_5678_9ABC_DEF1, 77
    got = run_act(agent, obs, dones, hx, seed, counter)
    lg, _, _ = oracle_step(net, obs, dones, hx)
    p = np.exp(log_softmax64(lg))
    cdf = np.cumsum(p / p.sum(1, keepdims=True), axis=1)
    i = np.arange(n, dtype=np.uint64)
    c = philox4x32_10((i & M32, i >> np.uint64(32), np.full(n, counter), np.zeros(n)),
                      (seed & 0xFFFFFFFF, seed >> 32))
    u = u01(c[0])
    want = np.minimum((u[:, None] >= cdf).sum(1), A - 1)
    clear = np.abs(u[:, None] - cdf[:, :-1]).min(1) > 1e-5
    assert clear.mean() >= 0.99
    assert np.array_equal(got["actions"][clear], want[clear])
    assert len(np.unique(got["actions"])) > A // 2          # the draws use the action range
    again = run_act(agent, obs, dones, hx, seed, counter)
    for k in got:
        assert np.array_equal(got[k], again[k]), k
    nxt = run_act(agent, obs, dones, hx, seed, counter + 1)
    assert not np.array_equal(got["actions"], nxt["actions"])
    for k in ("hx_out", "values", "logits"):                # only the draw depends on the counter
        assert np.array_equal(got[k], nxt[k]), k


# ---- 3. batch independence
@pytest.mark.parametrize("G", WIDTHS)
@pytest.mark.parametrize("D,A", [(100, 2), (128, 16)])
def test_outputs_do_not_depend_on_batch_size_or_position(G, D, A):
    n = BIG
    agent = _agent(G, D, A)
    obs, dones, hx = _inputs(n, D, seed=21, G=G)
    big = run_act(agent, obs, dones, hx, seed=2, counter=5)
    small = run_act(agent, obs[:3], dones[:3], hx[:3], seed=2, counter=5)
    for k in big:   # same sample indices: the draw and its log-prob agree too
        assert np.array_equal(big[k][:3], small[k]), k
    obs2, dones2, hx2 = obs.copy(), dones.copy(), hx.copy()
    obs2[4098:], dones2[4098:], hx2[4098:] = obs[:3], dones[:3], hx[:3]   # other slots of a workgroup
    moved = run_act(agent, obs2, dones2, hx2, seed=2, counter=5)
    for k in ("hx_out", "values", "logits"):
        assert np.array_equal(moved[k][4098:], small[k]), k
    v_big = run_value(agent, obs, hx, dones)
    assert np.array_equal(v_big[:3], run_value(agent, obs[:3], hx[:3], dones[:3]))
    assert np.array_equal(run_value(agent, obs2, hx2, dones2)[4098:], v_big[:3])


# ---- 4. the rollout on it
@pytest.mark.parametrize("G", WIDTHS)
def test_chained_rollout_matches_the_recomputed_sequence_and_feeds_learn(G):
    """test_gpu_gru_wide_act.py's chained-rollout check at T = 4, N = 9, D = 100: the fused
    rollout's cached log_probs / values against GT.sequence in float64 on the rollout's own
    inputs, no further from it than 4x the torch path's own fp32 distance (floor 2e-5); the rows
    then feed both learn() paths."""
    T, Nn, D, A = 4, 9, 100, 6
    agent = base._rollout_agent(T, Nn, D, A, True, G=G, num_epochs=2, wide_observations=True)
    assert agent.gru is not None and agent.gru.dims.obs_dim == D
    exp = agent.rollout()
    torch.cuda.synchronize()
    st = agent._rollout_staging
    assert tuple(st["obs"].shape) == tuple(st["nobs"].shape) == tuple(st["nobs_d"].shape) == (Nn, D)
    assert len(exp) == T and tuple(exp[0][0].shape) == (Nn, D)
    assert tuple(exp[0][9].shape) == (1, Nn, G) and tuple(agent.current_hx.shape) == (1, Nn, G)
    obs = torch.stack([r[0] for r in exp])
    act = torch.stack([r[1] for r in exp])
    pd = torch.stack([r[5] for r in exp])
    lp_f = torch.stack([r[6] for r in exp]).cpu().double().numpy()
    v_f = torch.stack([r[7] for r in exp]).cpu().double().numpy()
    hx0 = exp[0][9]
    params = {k: torch.from_numpy(p.detach().cpu().double().numpy())
              for k, p in agent.network.named_parameters()}
    assert list(params) == GT.GRU_NAMES
    with torch.no_grad():
        lg64, v64 = GT.sequence(params, obs.cpu().double(), pd.cpu(), hx0[0].cpu().double())
        lp64 = torch.log_softmax(lg64, -1).gather(-1, act.cpu()[..., None])[..., 0].numpy()
        v64 = v64.numpy()
        lg32, v32, _ = agent.network.get_logits_values_and_hx(obs, hx0, pd)
        lp32 = torch.distributions.Categorical(logits=lg32).log_prob(act).cpu().double().numpy()
        v32 = v32.cpu().double().numpy()
    d_fused = max(np.abs(lp_f - lp64).max(), np.abs(v_f - v64).max())
    d_torch = max(np.abs(lp32 - lp64).max(), np.abs(v32 - v64).max())
    print(f"G={G}: d_fused = {d_fused:.3e}  d_torch = {d_torch:.3e}")
    assert d_fused <= max(4 * d_torch, 2e-5), (d_fused, d_torch)
    # every row's hx is the previous row's step output: the kernel run again on that row
    for t in (0, T - 1):
        row = exp[t]
        again = run_act(agent, row[0].cpu().numpy(), row[5].cpu().numpy(),
                        row[9][0].cpu().numpy(), agent._act_seed, t)
        nxt = exp[t + 1][9] if t + 1 < T else agent.current_hx
        assert np.array_equal(again["hx_out"], nxt[0].cpu().numpy()), t
        assert np.array_equal(again["actions"], row[1].cpu().numpy()), t
        assert np.array_equal(again["log_probs"], row[6].cpu().numpy()), t
    for fused_gru in (True, False):
        agent.fused_gru = fused_gru
        p0 = agent.flat.flat.clone()
        np.random.seed(3)
        agent.learn(exp)
        torch.cuda.synchronize()
        assert torch.isfinite(agent.flat.flat).all()
        assert float((agent.flat.flat - p0).abs().max()) > 1e-5, fused_gru
