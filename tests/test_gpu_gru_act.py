"""RecurrentPPO's fused rollout step (csrc/gruact.hip: dppo_gru_act_f32 / dppo_gru_value_f32,
SURVEY §8 f4 rollout) and the rollout() path built on it (RecurrentPPO.fused_rollout), at the
default gru_hidden_dim 16; the helpers take the width (tests/test_gpu_gru_wide_act.py: 32, 64).

Yardstick: ``RecurrentActorCriticNetwork(...).double()`` on the CPU with the agent's parameters
(tests/test_gru_oracle_cpu.py pins it to oracle/gru_torch.py; the reference itself crashes at
recurrent_ppo.py:78).  Tolerance of every forward quantity: atol 2e-5, rtol 1e-5, the project's
bound for head outputs (test_actor_heads_match_reference_forward).  Draws are reproduced from the
documented Philox4x32-10 stream on the oracle's softmax.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diamond
from diamond import _native as N
from diamond.recurrent_ppo import RecurrentActorCriticNetwork
from oracle import gru_torch as GT

from test_gpu_rollout_ckpt import philox4x32_10, u01

M32 = np.uint64(0xFFFFFFFF)
G = 16
ATOL, RTOL = 2e-5, 1e-5


def _agent(T, Nn, D, A, spread=True, G=G, **kw):
    import gym_stub
    np.random.seed(0)
    torch.manual_seed(0)
    envs = gym_stub.SyncVectorEnv([lambda: gym_stub.SyntheticEnv(D, A)] * Nn)
    cfg = diamond.RecurrentPPOConfig(rollout_steps=T, num_envs=Nn, verbose=False,
                                     gru_hidden_dim=G, **kw)
    agent = diamond.RecurrentPPO(None, cfg, envs=envs)
    assert agent.gru is not None, "gru_hidden_dim %d did not take the fused path" % G
    if spread:   # spread the weights so gates and heads leave their linear range
        torch.manual_seed(1)
        with torch.no_grad():
            for p in agent.network.parameters():
                p.add_(torch.randn_like(p) * 0.3)
    return agent


def _oracle_net(agent):
    """The float64 CPU module with the agent's parameters."""
    net = RecurrentActorCriticNetwork(agent.envs.single_observation_space,
                                      agent.envs.single_action_space, cfg=agent.cfg).double()
    net.load_state_dict({k: v.detach().cpu().double()
                         for k, v in agent.network.state_dict().items()})
    return net


def _inputs(n, D, seed, done_frac=0.3, G=G):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, D)).astype(np.float32),
            rng.random(n) < done_frac,
            (rng.standard_normal((n, G)) * 0.5).astype(np.float32))


def _dev(agent, x, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(agent.device)
    return t if dt is None else t.to(dt)


def run_act(agent, obs, dones, hx, seed=1, counter=0, logits=True):
    """One dppo_gru_act_f32 call on host arrays -> dict of host arrays."""
    n, A, G, dev = obs.shape[0], agent.gru.dims.act_dim, agent.gru.dims.gru_hidden, agent.device
    o, d, h = _dev(agent, obs), _dev(agent, dones, torch.uint8), _dev(agent, hx)
    out = dict(hx_out=torch.empty((n, G), device=dev),
               actions=torch.empty(n, dtype=torch.int32, device=dev),
               log_probs=torch.empty(n, device=dev), values=torch.empty(n, device=dev),
               logits=torch.empty((n, A), device=dev) if logits else None)
    step = N.GruStep(o.data_ptr(), d.data_ptr(), h.data_ptr(), out["hx_out"].data_ptr(),
                     out["actions"].data_ptr(), out["log_probs"].data_ptr(),
                     out["values"].data_ptr(), out["logits"].data_ptr() if logits else None)
    N.check(agent.gru.lib.dppo_gru_act_f32(
        agent.gru.h, agent.flat.flat.data_ptr(), ctypes.byref(step), n, seed, counter,
        torch.cuda.current_stream().cuda_stream), "dppo_gru_act_f32")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def run_value(agent, obs, hx, dones=None):
    n = obs.shape[0]
    o, h = _dev(agent, obs), _dev(agent, hx)
    d = None if dones is None else _dev(agent, dones, torch.uint8)
    v = torch.empty(n, device=agent.device)
    N.check(agent.gru.lib.dppo_gru_value_f32(
        agent.gru.h, agent.flat.flat.data_ptr(), o.data_ptr(), h.data_ptr(),
        None if d is None else d.data_ptr(), n, v.data_ptr(),
        torch.cuda.current_stream().cuda_stream), "dppo_gru_value_f32")
    torch.cuda.synchronize()
    return v.cpu().numpy()


def oracle_step(net, obs, dones, hx):
    """float64: logits [n, A], values [n], new hidden state [n, 16]."""
    with torch.no_grad():
        lg, v, h = net.get_logits_values_and_hx(torch.from_numpy(obs).double()[None],
                                                torch.from_numpy(hx).double()[None],
                                                torch.from_numpy(np.asarray(dones, bool))[None])
    return lg[0].numpy(), v[0].numpy(), h[0].numpy()


def oracle_value(net, obs, hx, dones=None):
    with torch.no_grad():
        d = None if dones is None else torch.from_numpy(np.asarray(dones, bool))[None]
        return net.get_values(torch.from_numpy(obs).double()[None],
                              torch.from_numpy(hx).double()[None], d)[0].numpy()


def log_softmax64(lg):
    z = lg - lg.max(1, keepdims=True)
    return z - np.log(np.exp(z).sum(1, keepdims=True))


# ---- 1. one step against the float64 module
@pytest.mark.parametrize("n,D,A", [(1, 1, 1), (3, 4, 2), (17, 7, 3), (33, 17, 6), (64, 32, 16),
                                   (4101, 8, 4)])
def test_one_step_matches_float64_module(n, D, A):
    agent = _agent(2, 4, D, A)
    net = _oracle_net(agent)
    obs, mixed, hx = _inputs(n, D, seed=n * 10 + A)
    nobs = np.random.default_rng(n).standard_normal((n, D)).astype(np.float32)
    close = lambda got, want, what: np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL,
                                                               err_msg=what)
    for tag, dones in (("mixed", mixed), ("all", np.ones(n, bool)), ("none", np.zeros(n, bool))):
        got = run_act(agent, obs, dones, hx, seed=5, counter=3)
        lg, v, h = oracle_step(net, obs, dones, hx)
        close(got["logits"], lg, tag + " logits")
        close(got["values"], v, tag + " values")
        close(got["hx_out"], h, tag + " hx_out")
        act = got["actions"]
        assert act.dtype == np.int32 and act.min() >= 0 and act.max() < A
        close(got["log_probs"], log_softmax64(lg)[np.arange(n), act], tag + " log_probs")
        if A == 1:
            assert np.all(act == 0) and np.abs(got["log_probs"]).max() <= 1e-6
        # V(next_obs) from the step's new hidden state, without and with a reset
        close(run_value(agent, nobs, got["hx_out"]), oracle_value(net, nobs, got["hx_out"]),
              tag + " next values")
        close(run_value(agent, nobs, hx, dones), oracle_value(net, nobs, hx, dones),
              tag + " values with dones")
        # the logits are optional
        lean = run_act(agent, obs, dones, hx, seed=5, counter=3, logits=False)
        for k in ("hx_out", "actions", "log_probs", "values"):
            assert np.array_equal(lean[k], got[k]), (tag, k)


# ---- 2. the draws are the documented Philox stream
def test_draws_are_the_documented_philox_stream():
    """actions = inverse CDF of the ORACLE's softmax at u01(c0) of Philox4x32-10 (key = seed,
    counter = {i lo, i hi, ctr lo, ctr hi}), compared exactly where u is more than 1e-5 from every
    CDF boundary.  A sample misses that margin with probability <= (A - 1) * 2e-5 = 3e-4: about one
    of the 4096 against an allowance of 1 % (41)."""
    n, D, A = 4096, 8, 16
    agent = _agent(2, 4, D, A)
    net = _oracle_net(agent)
    obs, dones, hx = _inputs(n, D, seed=11)
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


# ---- 3. distribution
def test_action_frequencies_match_softmax():
    D, A, n = 8, 4, 1 << 17
    agent = _agent(2, 4, D, A, spread=False)
    with torch.no_grad():
        agent.network.actor_out_layer.weight.mul_(100.0)   # spread the probabilities out
    net = _oracle_net(agent)
    rng = np.random.default_rng(3)
    o = rng.standard_normal((1, D)).astype(np.float32)
    h = (rng.standard_normal((1, G)) * 0.5).astype(np.float32)
    none = np.zeros(1, bool)
    p = np.exp(log_softmax64(oracle_step(net, o, none, h)[0]))[0]
    assert p.min() > 0.01
    got = run_act(agent, np.tile(o, (n, 1)), np.zeros(n, bool), np.tile(h, (n, 1)), 1234, 9,
                  logits=False)
    freq = np.bincount(got["actions"], minlength=A) / n
    sig = np.sqrt(p * (1 - p) / n)
    assert np.all(np.abs(freq - p) <= 5 * sig), (freq, p)


# ---- 4. batch independence
def test_outputs_do_not_depend_on_batch_size_or_position():
    n, D, A = 4101, 8, 4
    agent = _agent(2, 4, D, A)
    obs, dones, hx = _inputs(n, D, seed=21)
    big = run_act(agent, obs, dones, hx, seed=2, counter=5)
    small = run_act(agent, obs[:3], dones[:3], hx[:3], seed=2, counter=5)
    for k in big:   # same sample indices: the draw and its log-prob agree too
        assert np.array_equal(big[k][:3], small[k]), k
    obs2, dones2, hx2 = obs.copy(), dones.copy(), hx.copy()
    obs2[4098:], dones2[4098:], hx2[4098:] = obs[:3], dones[:3], hx[:3]
    moved = run_act(agent, obs2, dones2, hx2, seed=2, counter=5)
    for k in ("hx_out", "values", "logits"):
        assert np.array_equal(moved[k][4098:], small[k]), k
    v_big = run_value(agent, obs, hx, dones)
    assert np.array_equal(v_big[:3], run_value(agent, obs[:3], hx[:3], dones[:3]))
    assert np.array_equal(run_value(agent, obs2, hx2, dones2)[4098:], v_big[:3])


# ---- 5. argument checks on a live handle
def test_argument_checks_on_a_live_handle():
    n, D, A = 5, 4, 2
    agent = _agent(2, 4, D, A)
    obs, dones, hx = _inputs(n, D, seed=1)
    o, d, h = _dev(agent, obs), _dev(agent, dones, torch.uint8), _dev(agent, hx)
    dev = agent.device
    hx_out = torch.full((n, G), 7.0, device=dev)
    act = torch.full((n,), -3, dtype=torch.int32, device=dev)
    lp, v = torch.full((n,), 7.0, device=dev), torch.full((n,), 7.0, device=dev)
    call = lambda step, m: N.check(agent.gru.lib.dppo_gru_act_f32(
        agent.gru.h, agent.flat.flat.data_ptr(), ctypes.byref(step), m, 1, 0,
        torch.cuda.current_stream().cuda_stream), "dppo_gru_act_f32")
    alias = N.GruStep(o.data_ptr(), d.data_ptr(), h.data_ptr(), h.data_ptr(), act.data_ptr(),
                      lp.data_ptr(), v.data_ptr(), None)
    with pytest.raises(ValueError):
        call(alias, n)
    good = N.GruStep(o.data_ptr(), d.data_ptr(), h.data_ptr(), hx_out.data_ptr(), act.data_ptr(),
                     lp.data_ptr(), v.data_ptr(), None)
    with pytest.raises(ValueError):
        call(good, -1)
    missing = N.GruStep(o.data_ptr(), d.data_ptr(), h.data_ptr(), hx_out.data_ptr(),
                        act.data_ptr(), None, v.data_ptr(), None)
    with pytest.raises(ValueError):
        call(missing, n)
    call(good, 0)                                     # OK, no launch
    N.check(agent.gru.lib.dppo_gru_value_f32(
        agent.gru.h, agent.flat.flat.data_ptr(), o.data_ptr(), h.data_ptr(), None, 0,
        v.data_ptr(), torch.cuda.current_stream().cuda_stream), "dppo_gru_value_f32")
    torch.cuda.synchronize()
    assert torch.all(hx_out == 7.0) and torch.all(act == -3)
    assert torch.all(lp == 7.0) and torch.all(v == 7.0)
    assert torch.equal(h.cpu(), torch.from_numpy(hx))


# ---- 6. the rollout surface
def _start(agent, env_seed=7):
    """What train() sets up before its first rollout()."""
    cfg = agent.cfg
    agent.current_observations, _ = agent.envs.reset(seed=env_seed)
    agent.prev_dones = np.zeros(cfg.num_envs, dtype=bool)
    agent.current_hx = torch.zeros(1, cfg.num_envs, cfg.gru_hidden_dim, device=agent.device)


def _rollout_agent(T, Nn, D, A, fused, G=G, **kw):
    import gym_stub
    agent = _agent(T, Nn, D, A, G=G, **kw)
    # episodes end often enough for several hidden resets inside T steps
    agent.envs = gym_stub.SyncVectorEnv(
        [lambda: gym_stub.SyntheticEnv(D, A, p_term=0.1, p_trunc=0.05)] * Nn)
    agent.fused_rollout = fused
    _start(agent)
    return agent


@pytest.mark.parametrize("T,Nn,D,A", [(16, 8, 4, 2), (16, 20, 7, 3)])
def test_fused_rollout_surface(T, Nn, D, A):
    agent = _rollout_agent(T, Nn, D, A, True, num_epochs=2)
    exp = agent.rollout()
    dev = agent.device
    assert len(exp) == T
    f32, cuda = torch.float32, dev.type
    for row in exp:
        assert len(row) == 10
        obs, act, rew, term, trunc, pd, lp, v, nv, hx = row
        for x, shape, dt in ((obs, (Nn, D), f32), (act, (Nn,), torch.int64), (pd, (Nn,), torch.bool),
                             (lp, (Nn,), f32), (v, (Nn,), f32), (nv, (Nn,), f32),
                             (hx, (1, Nn, G), f32)):
            assert isinstance(x, torch.Tensor) and tuple(x.shape) == shape and x.dtype == dt
            assert x.device.type == cuda and x.device.index == dev.index
        for x in (rew, term, trunc):
            assert isinstance(x, np.ndarray) and x.shape == (Nn,)
        assert int(act.min()) >= 0 and int(act.max()) < A
    assert torch.all(exp[0][9] == 0)
    assert any(bool(row[5].any()) for row in exp[1:])       # resets happened
    assert tuple(agent.current_hx.shape) == (1, Nn, G)
    # every row's hx is the previous row's step output (the kernel run again on that row), and
    # so are its cached values; next_values come from that output and the next observation
    for t, row in enumerate(exp):
        again = run_act(agent, row[0].cpu().numpy(), row[5].cpu().numpy(),
                        row[9][0].cpu().numpy(), agent._act_seed, t)
        nxt = exp[t + 1][9] if t + 1 < T else agent.current_hx
        assert np.array_equal(again["hx_out"], nxt[0].cpu().numpy()), t
        assert np.array_equal(again["actions"], row[1].cpu().numpy()), t
        assert np.array_equal(again["log_probs"], row[6].cpu().numpy()), t
        assert np.array_equal(again["values"], row[7].cpu().numpy()), t
    # a second rollout leaves the first experience unchanged
    before = [[x.clone() if isinstance(x, torch.Tensor) else np.array(x) for x in row]
              for row in exp]
    h_end = agent.current_hx.clone()
    exp2 = agent.rollout()
    torch.cuda.synchronize()
    assert torch.equal(exp2[0][9], h_end)
    for row, old in zip(exp, before):
        for x, y in zip(row, old):
            assert (torch.equal(x, y) if isinstance(x, torch.Tensor) else np.array_equal(x, y))
    assert not torch.equal(exp2[0][0], exp[0][0])
    # learn() takes the rows unchanged, on both of its paths
    for fused_gru in (True, False):
        agent.fused_gru = fused_gru
        p0 = agent.flat.flat.clone()
        np.random.seed(3)
        agent.learn(exp)
        torch.cuda.synchronize()
        assert torch.isfinite(agent.flat.flat).all()
        assert float((agent.flat.flat - p0).abs().max()) > 1e-5, fused_gru


def test_fused_rollout_is_reproducible_from_the_seed():
    T, Nn, D, A = 16, 8, 4, 2
    rows = []
    for _ in range(2):
        agent = _rollout_agent(T, Nn, D, A, True)
        exp = agent.rollout() + agent.rollout()
        torch.cuda.synchronize()
        rows.append(([[x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
                       for x in row] for row in exp], agent.current_hx.cpu().numpy()))
    (e1, h1), (e2, h2) = rows
    assert np.array_equal(h1, h2)
    for r1, r2 in zip(e1, e2):
        for x, y in zip(r1, r2):
            assert np.array_equal(x, y)


def test_default_rollout_still_draws_from_torch():
    """fused_rollout = False (the default): the actions under torch.manual_seed(s) are those of
    the torch ops rollout() has always run, restated here inline."""
    T, Nn, D, A, s = 16, 8, 4, 2, 1234
    agent = _rollout_agent(T, Nn, D, A, False)
    assert diamond.RecurrentPPO.fused_rollout is False
    torch.manual_seed(s)
    exp = agent.rollout()
    ref = _rollout_agent(T, Nn, D, A, False)
    torch.manual_seed(s)
    obs, hx, pd = ref.current_observations, ref.current_hx, ref.prev_dones
    for t in range(T):
        obs_t = torch.as_tensor(obs[None, ...], dtype=torch.float32, device=ref.device)
        pd_t = torch.as_tensor(pd[None, ...], dtype=torch.bool, device=ref.device)
        with torch.inference_mode():
            logits, values, new_hx = ref.network.get_logits_values_and_hx(obs_t, hx, pd_t)
        dist = torch.distributions.Categorical(logits=logits.squeeze(0))
        actions = dist.sample()
        log_probs = dist.log_prob(actions)
        nobs, rew, term, trunc, _ = ref.envs.step(actions.cpu().numpy())
        assert torch.equal(exp[t][1], actions), t
        assert exp[t][1].dtype == torch.int64
        assert torch.equal(exp[t][6], log_probs) and torch.equal(exp[t][7], values.squeeze(0))
        assert torch.equal(exp[t][9], hx) and np.array_equal(exp[t][2], rew)
        dones = np.logical_or(term, trunc)
        obs = ref.envs.reset(options={"reset_mask": dones})[0] if np.any(dones) else nobs
        hx, pd = new_hx, dones


# ---- 7. the chained sequence agrees with what learn() recomputes
def test_cached_rollout_outputs_match_the_recomputed_sequence():
    """The fused rollout's cached log_probs / values (chained through T steps in fp32) against
    GT.sequence in float64 on the rollout's own (obs, prev_dones, hx[0], actions), beside the
    torch path's fp32 GPU outputs for the same inputs: the fused path may be no further from the
    float64 result than 4x the torch path's own distance (floor 2e-5), the rule of
    tests/test_gpu_production.py.

    Measured on MI355X at this shape: d_fused = 1.13e-6, d_torch = 9.0e-7."""
    T, Nn, D, A = 16, 20, 7, 3
    agent = _rollout_agent(T, Nn, D, A, True)
    exp = agent.rollout()
    torch.cuda.synchronize()
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
    print(f"d_fused = {d_fused:.3e}  d_torch = {d_torch:.3e}")
    assert d_fused <= max(4 * d_torch, 2e-5), (d_fused, d_torch)
