"""GPU checks of the wide class's fused rollout sampler (csrc/mbwide.hip wide_act_kernel, reached
through dppo_actor_forward_f32 / dppo_act_f32 / dppo_act_squash_f32 and, opt-in, rollout()).

* heads against the NumPy oracle's forward at rtol = atol = 2e-5 (the bound
  test_wide_old_policy_and_records_vs_oracle holds the same forward to), also with obs at a
  4-byte-offset view;
* discrete draws = the documented Philox stream: inverse CDF of the oracle's float64 softmax at
  u01(c0) on the samples whose u is farther than 1e-4 from every CDF boundary (a logit within 2e-5
  moves a CDF value by less than 5e-5), at least 99 % of the samples being that clear
  (tests/test_wide_act_cpu.py shows the inputs keep that);
* Gaussian draws against oracle_gaussian_draws at rtol = atol = 1e-4, the squashed environment
  actions against oracle.ppo_np.squash_action on the kernel's own samples;
* determinism, the shared call counter, the public surface (fused_actions_wide), and the shapes
  of neither class staying unsupported.

Shapes and sizes: tests/wide_act_cases.py.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diamond
from diamond import _native as N
from oracle import ppo_np as P

import wide_act_cases as W
from gpu_helpers import SpecEnvs, dev, stream
from test_gpu_rollout_ckpt import oracle_gaussian_draws, philox4x32_10, u01


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _cases(cont=None):
    return [pytest.param(c, id=W.case_id(c)) for c in W.cases(cont)]


def _resolve(case):
    """The case with its size spelled out (32 * CUs + 7 needs the device)."""
    return (*case[:4], W.real_n(case[4], _cus()))


@functools.lru_cache(maxsize=None)
def _case(Hd, D, A, cont, n):
    """One case's inputs and oracle heads, computed once and shared (read-only) by the tests."""
    params, flat, obs = W.inputs(Hd, D, A, cont, n)
    out = P.forward(params, obs, cont)["out"]
    for a in (flat, obs, out):
        a.setflags(write=False)
    return params, flat, obs, out


@functools.lru_cache(maxsize=None)
def _handle(Hd, D, A, cont):
    return N.Handle(0, W.dims(Hd, D, A, cont))


def _to_dev(x):
    return torch.tensor(x, device=dev())  # (a copy: the shared inputs are read-only)


def _heads(h, pd, od, n, A):
    out = torch.empty((n, A), device=dev())
    N.check(h.lib.dppo_actor_forward_f32(h.h, pd.data_ptr(), od.data_ptr(), n, out.data_ptr(),
                                         stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _act(h, pd, od, n, A, cont, seed, counter):
    act = torch.empty((n, A) if cont else (n,), dtype=torch.float32 if cont else torch.int32,
                      device=dev())
    N.check(h.lib.dppo_act_f32(h.h, pd.data_ptr(), od.data_ptr(), n, seed, counter,
                               act.data_ptr(), stream()))
    torch.cuda.synchronize()
    return act.cpu().numpy()


def _act_squash(h, pd, od, n, A, seed, counter, lo, hi):
    u = torch.empty((n, A), device=dev())
    env = torch.empty((n, A), device=dev())
    N.check(h.lib.dppo_act_squash_f32(
        h.h, pd.data_ptr(), od.data_ptr(), n, seed, counter,
        None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data,
        u.data_ptr(), env.data_ptr(), stream()))
    torch.cuda.synchronize()
    return u.cpu().numpy(), env.cpu().numpy()


# ---- 1: heads ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _cases())
def test_wide_actor_heads_vs_oracle(case):
    case = _resolve(case)
    Hd, D, A, cont, n = case
    _, flat, obs, out = _case(*case)
    got = _heads(_handle(Hd, D, A, cont), _to_dev(flat), _to_dev(obs), n, A)
    print(f"{W.case_id(case)}: max |heads - oracle| {np.abs(got - out).max():.3g}")
    np.testing.assert_allclose(got, out, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("shape", [(128, 8, 4, False), (64, 105, 8, True)])
def test_wide_actor_heads_with_obs_at_a_4_byte_offset(shape):
    Hd, D, A, cont = shape
    n = 33
    _, flat, obs, out = _case(*shape, n)
    buf = torch.zeros(n * D + 1, device=dev())
    od = buf[1:].view(n, D)
    od.copy_(_to_dev(obs))
    assert od.data_ptr() % 16 == 4
    got = _heads(_handle(*shape), _to_dev(flat), od, n, A)
    np.testing.assert_allclose(got, out, rtol=2e-5, atol=2e-5)


# ---- 2: discrete draws ------------------------------------------------------------------------
@pytest.mark.parametrize("case", _cases(cont=False))
def test_wide_discrete_draws_are_the_documented_philox_stream(case):
    case = _resolve(case)
    Hd, D, A, cont, n = case
    _, flat, obs, out = _case(*case)
    got = _act(_handle(Hd, D, A, cont), _to_dev(flat), _to_dev(obs), n, A, False, W.SEED,
               W.COUNTER)
    want, clear = W.categorical_oracle(out, W.SEED, W.COUNTER, philox4x32_10, u01)
    print(f"{W.case_id(case)}: clear share {clear.mean():.4f}, "
          f"equal on clear {np.mean(got[clear] == want[clear]):.4f}")
    assert clear.mean() >= W.MIN_CLEAR
    assert got.min() >= 0 and got.max() < A
    assert np.array_equal(got[clear], want[clear])


# ---- 4: Gaussian draws and squash -------------------------------------------------------------
def _bounds(A):
    return (np.linspace(-2.0, -0.25, A).astype(np.float32),
            np.linspace(0.5, 3.0, A).astype(np.float32))


@pytest.mark.parametrize("case", _cases(cont=True))
def test_wide_gaussian_draws_and_squash(case):
    case = _resolve(case)
    Hd, D, A, cont, n = case
    params, flat, obs, out = _case(*case)
    h, pd, od = _handle(Hd, D, A, cont), _to_dev(flat), _to_dev(obs)
    u = _act(h, pd, od, n, A, True, W.SEED, W.COUNTER)
    want = oracle_gaussian_draws(out.astype(np.float64), params["actor_log_std"], W.SEED,
                                 W.COUNTER)
    print(f"{W.case_id(case)}: max |u - oracle| {np.abs(u - want).max():.3g}")
    np.testing.assert_allclose(u, want, rtol=1e-4, atol=1e-4)
    lo, hi = _bounds(A)
    for bounded in (False, True):
        u2, env = _act_squash(h, pd, od, n, A, W.SEED, W.COUNTER, lo if bounded else None,
                              hi if bounded else None)
        assert np.array_equal(u2, u)  # bit for bit the plain call's draws
        if bounded:
            env_own = P.squash_action(u2, lo.astype(np.float64), hi.astype(np.float64))
            assert np.all(env >= lo) and np.all(env <= hi)
            atol = float(4e-7 * (1 + np.abs(lo).max()))
        else:
            env_own = np.tanh(u2.astype(np.float64))
            assert np.all(np.abs(env) <= 1.0)
            atol = 4e-7
        print(f"  bounded={bounded}: max |env - squash(u)| {np.abs(env - env_own).max():.3g}")
        np.testing.assert_allclose(env, env_own, rtol=0, atol=atol)


# ---- 5: determinism and counters --------------------------------------------------------------
@pytest.mark.parametrize("shape", [(128, 8, 4, False), (64, 105, 8, True)])
def test_wide_draws_are_deterministic_and_follow_the_counter(shape):
    Hd, D, A, cont = shape
    n = 33
    _, flat, obs, _ = _case(*shape, n)
    h, pd, od = _handle(*shape), _to_dev(flat), _to_dev(obs)
    a = _act(h, pd, od, n, A, cont, W.SEED, W.COUNTER)
    b = _act(h, pd, od, n, A, cont, W.SEED, W.COUNTER)
    c = _act(h, pd, od, n, A, cont, W.SEED, W.COUNTER + 1)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)


def _agent(Hd, D, A, cont, T, Nn, envs=None, **kw):
    Cfg = diamond.ContinuousPPOConfig if cont else diamond.PPOConfig
    Agent = diamond.ContinuousPPO if cont else diamond.PPO
    cfg = Cfg(network_hidden_dim=Hd, rollout_steps=T, num_envs=Nn, verbose=False, **kw)
    return Agent(None, cfg, envs=envs if envs is not None else SpecEnvs(D, A, cont))


def test_learner_act_shares_one_counter_with_the_squashing_sampler():
    Hd, D, A, n = 64, 40, 3, 33
    agent = _agent(Hd, D, A, True, 4, 32)
    L = agent._learner
    assert L.shape_class == "wide" and not L.fused_act and not L.wide_act
    obs = np.random.default_rng(5).standard_normal((n, D), dtype=np.float32)
    with pytest.raises(RuntimeError):
        L.act(obs, 9)
    L.wide_act = True
    seed = 0x0123_4567_89AB_CDEF
    a0 = L.act(obs, seed)
    u1, env1 = L.act(obs, seed, squash=True)
    a2 = L.act(obs, seed)
    assert L._act_counter == 3
    od = _to_dev(obs)
    for counter, got in ((0, a0), (1, u1), (2, a2)):
        want = _act(L.handle, L.flat.flat, od, n, A, True, seed, counter)
        assert np.array_equal(got, want), counter
    assert a0.dtype == np.float32 and a0.shape == (n, A)
    np.testing.assert_allclose(env1, np.tanh(u1.astype(np.float64)), rtol=0, atol=4e-7)
    assert not np.array_equal(a0, a2)


# ---- 6: public surface ------------------------------------------------------------------------
def _torch_rng():
    """torch's generators that sampling can draw from: the host's and the device's (get_actions
    samples on the device, so it is the device generator that a default rollout advances)."""
    return torch.cat([torch.get_rng_state(), torch.cuda.get_rng_state(dev())])


def _flat_state(agent):
    return np.concatenate([p.detach().cpu().numpy().ravel() for p in agent.network.parameters()])


def _oracle_params(agent):
    return {n: p.detach().cpu().numpy().copy() for n, p in agent.network.named_parameters()}


def test_wide_ppo_rollout_samples_with_the_kernel_only_on_request():
    import gym_stub
    Hd, D, A, Nn, T = 128, 8, 4, 32, 4
    torch.manual_seed(3)
    np.random.seed(3)
    envs = gym_stub.SyncVectorEnv([lambda: gym_stub.SyntheticEnv(D, A)] * Nn)
    agent = _agent(Hd, D, A, False, T, Nn, envs=envs)
    L = agent._learner
    assert L.shape_class == "wide" and not L.fused_act
    assert agent.fused_actions_wide is False
    # default: network.get_actions, which draws from torch's generator
    agent.current_observations, _ = agent.envs.reset(seed=5)
    st = _torch_rng()
    agent.rollout()
    assert not torch.equal(st, _torch_rng())
    assert not L.wide_act
    with pytest.raises(RuntimeError):
        L.act(np.zeros((Nn, D), np.float32), 1)
    # opted in: the Philox stream, torch's generator untouched
    agent.fused_actions_wide = True
    obs0, _ = agent.envs.reset(seed=6)
    agent.current_observations = obs0
    obs0 = np.array(obs0, np.float32)
    params = _oracle_params(agent)
    before = _flat_state(agent)
    st = _torch_rng()
    exp = agent.rollout()
    assert torch.equal(st, _torch_rng())
    assert L.wide_act and L._act_counter == T
    act0 = exp[0][2]
    assert act0.dtype == np.int64 and act0.shape == (Nn,)
    want, clear = W.categorical_oracle(P.forward(params, obs0, False)["out"], agent._act_seed, 0,
                                       philox4x32_10, u01)
    assert clear.mean() >= W.MIN_CLEAR
    assert np.array_equal(act0[clear], want[clear])
    assert all(0 <= row[2].min() and row[2].max() < A for row in exp)
    agent.learn(exp)
    torch.cuda.synchronize()
    after = _flat_state(agent)
    assert np.all(np.isfinite(after)) and not np.array_equal(before, after)


def test_wide_continuous_rollout_squashes_in_the_kernel_on_request():
    import gym_stub
    Hd, D, A, Nn, T = 64, 40, 3, 32, 4
    lo, hi = _bounds(A)

    def make_env():
        e = gym_stub.SyntheticEnv(D, continuous=True, act_dim=A)
        e.action_space = gym_stub.Box(low=lo, high=hi, shape=(A,))
        return e

    torch.manual_seed(4)
    np.random.seed(4)
    envs = gym_stub.SyncVectorEnv([make_env] * Nn)
    agent = _agent(Hd, D, A, True, T, Nn, envs=envs, tanh_squash=True)
    L = agent._learner
    assert L.shape_class == "wide" and not L.fused_act
    agent.fused_actions_wide = True
    received = []
    step = envs.step
    envs.step = lambda a: (received.append(np.array(a)), step(a))[1]
    obs0, _ = agent.envs.reset(seed=7)
    agent.current_observations = obs0
    obs0 = np.array(obs0, np.float32)
    params = _oracle_params(agent)
    before = _flat_state(agent)
    st = _torch_rng()
    exp = agent.rollout()
    assert torch.equal(st, _torch_rng())
    assert len(received) == T and L._act_counter == T
    u0 = exp[0][2]
    assert u0.dtype == np.float32 and u0.shape == (Nn, A)
    want = oracle_gaussian_draws(P.forward(params, obs0, True)["out"].astype(np.float64),
                                 params["actor_log_std"], agent._act_seed, 0)
    np.testing.assert_allclose(u0, want, rtol=1e-4, atol=1e-4)   # the experience keeps u
    for t in range(T):                                            # the env got the squashed ones
        env_own = P.squash_action(exp[t][2], lo.astype(np.float64), hi.astype(np.float64))
        np.testing.assert_allclose(received[t], env_own, rtol=0,
                                   atol=float(4e-7 * (1 + np.abs(lo).max())))
        assert np.all(received[t] >= lo) and np.all(received[t] <= hi)
    agent.learn(exp)
    torch.cuda.synchronize()
    after = _flat_state(agent)
    assert np.all(np.isfinite(after)) and not np.array_equal(before, after)


# ---- 7: unsupported shapes --------------------------------------------------------------------
@pytest.mark.parametrize("Hd,D", [(256, 8), (128, 129)])
def test_actor_forward_stays_unsupported_outside_both_classes(Hd, D):
    n, A = 33, 4
    h = N.Handle(0, W.dims(Hd, D, A, False))
    pd = torch.zeros(h.layout.total, device=dev())
    od = torch.zeros((n, D), device=dev())
    out = torch.empty((n, A), device=dev())
    with pytest.raises(NotImplementedError):
        N.check(h.lib.dppo_actor_forward_f32(h.h, pd.data_ptr(), od.data_ptr(), n, out.data_ptr(),
                                             stream()))
