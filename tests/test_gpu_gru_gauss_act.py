"""RecurrentContinuousPPO's fused policy step (csrc/gruact.hip's gru_act_kernel<G, OBS, true> behind
dppo_gru_gauss_act_f32; dppo_gru_value_f32 is shared with the categorical agent).

Yardstick: ``RecurrentContinuousActorCriticNetwork(...).double()`` on the CPU with the agent's
parameters (tests/test_gru_gauss_cpu.py pins tests/gru_gauss_oracle.py to it).  Means, values and
the new hidden state: atol 2e-5, rtol 1e-5, the bound of tests/test_gpu_gru_act.py.  The draws
against ``oracle_gaussian_draws`` (tests/test_gpu_rollout_ckpt.py) at the oracle's means,
rtol = atol = 1e-4, that test's bound.  The log-prob against the float64 Normal log-density at the
kernel's own stored action and the oracle's mean: atol 2e-5, rtol 1e-5, or, where the float32
evaluation of the same expression is itself further off, 4x that (which applied is printed)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diamond
from diamond import _native as N
from diamond.recurrent_continuous_ppo import RecurrentContinuousActorCriticNetwork

from test_gpu_rollout_ckpt import oracle_gaussian_draws

ATOL, RTOL = 2e-5, 1e-5
WIDTHS = (16, 32, 64)
SHAPES = [(4, 1, False), (17, 6, False), (32, 16, False), (65, 4, True)]   # (D, A, wide_obs)
SIZES = (1, 5, 4 * 3 + 1)   # 4 envs per workgroup: one, a boundary crossed, three and one over
HALF_LOG_2PI = 0.5 * np.log(2 * np.pi)


def _agent(D, A, G, regime="zero", wide=False, T=2, Nn=4, **kw):
    import gym_stub
    np.random.seed(0)
    torch.manual_seed(0)
    envs = gym_stub.SyncVectorEnv(
        [lambda: gym_stub.SyntheticEnv(D, continuous=True, act_dim=A)] * Nn)
    cfg = diamond.RecurrentContinuousPPOConfig(rollout_steps=T, num_envs=Nn, verbose=False,
                                               gru_hidden_dim=G, wide_observations=wide, **kw)
    agent = diamond.RecurrentContinuousPPO(None, cfg, envs=envs)
    assert agent.gru is not None and agent.gru.gauss
    torch.manual_seed(1)
    with torch.no_grad():   # spread the weights so gates and heads leave their linear range
        for n, p in agent.network.named_parameters():
            if n != "actor_log_std":
                p.add_(torch.randn_like(p) * 0.3)
        if regime == "spread":
            ls = np.random.default_rng(A).uniform(-1.5, 0.5, (1, A)).astype(np.float32)
            agent.network.actor_log_std.copy_(torch.from_numpy(ls))
    return agent


def _oracle_net(agent):
    net = RecurrentContinuousActorCriticNetwork(agent.envs.single_observation_space,
                                                agent.envs.single_action_space,
                                                cfg=agent.cfg).double()
    net.load_state_dict({k: v.detach().cpu().double()
                         for k, v in agent.network.state_dict().items()})
    return net


def _inputs(n, D, G, seed, done_frac=0.3):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, D)).astype(np.float32), rng.random(n) < done_frac,
            (rng.standard_normal((n, G)) * 0.5).astype(np.float32))


def _dev(agent, x, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(x)).to(agent.device)
    return t if dt is None else t.to(dt)


def run_act(agent, obs, dones, hx, seed=1, counter=0, means=True):
    """One dppo_gru_gauss_act_f32 call on host arrays -> dict of host arrays."""
    n, A, G, dev = obs.shape[0], agent.gru.dims.act_dim, agent.gru.dims.gru_hidden, agent.device
    o, d, h = _dev(agent, obs), _dev(agent, dones, torch.uint8), _dev(agent, hx)
    out = dict(hx_out=torch.empty((n, G), device=dev), actions=torch.empty((n, A), device=dev),
               log_probs=torch.empty(n, device=dev), values=torch.empty(n, device=dev),
               means=torch.empty((n, A), device=dev) if means else None)
    step = N.GruGaussStep(o.data_ptr(), d.data_ptr(), h.data_ptr(), out["hx_out"].data_ptr(),
                          out["actions"].data_ptr(), out["log_probs"].data_ptr(),
                          out["values"].data_ptr(), out["means"].data_ptr() if means else None)
    N.check(agent.gru.lib.dppo_gru_gauss_act_f32(
        agent.gru.h, agent.flat.flat.data_ptr(), ctypes.byref(step), n, seed, counter,
        torch.cuda.current_stream().cuda_stream), "dppo_gru_gauss_act_f32")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def oracle_step(net, obs, dones, hx):
    """float64: means [n, A], values [n], new hidden state [n, G]."""
    with torch.no_grad():
        mean, _, v, h = net.get_means_log_stds_values_and_hx(
            torch.from_numpy(obs).double()[None], torch.from_numpy(hx).double()[None],
            torch.from_numpy(np.asarray(dones, bool))[None])
    return mean[0].numpy(), v[0].numpy(), h[0].numpy()


def _log_density(u, mean, ls, dt):
    u, mean, ls = (np.asarray(x, dt) for x in (u, mean, ls))
    z = (u - mean) * np.exp(-ls)
    return (dt(-0.5) * z * z - ls - dt(HALF_LOG_2PI)).sum(-1, dtype=dt)


@pytest.mark.parametrize("regime", ["zero", "spread"])
@pytest.mark.parametrize("D,A,wide", SHAPES)
@pytest.mark.parametrize("G", WIDTHS)
def test_one_step_matches_float64_module(G, D, A, wide, regime):
    agent = _agent(D, A, G, regime, wide)
    assert agent.gru.dims.wide_obs == int(wide)
    net = _oracle_net(agent)
    ls = agent.network.actor_log_std.detach().cpu().numpy().reshape(A)
    close = lambda got, want, what: np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL,
                                                               err_msg=what)
    seed, counter = 0x1234_5678_9ABC_DEF1, 77
    for n in SIZES:
        obs, dones, hx = _inputs(n, D, G, seed=n * 10 + A)
        got = run_act(agent, obs, dones, hx, seed, counter)
        mean, v, h = oracle_step(net, obs, dones, hx)
        close(got["means"], mean, "means")
        close(got["values"], v, "values")
        close(got["hx_out"], h, "hx_out")
        assert got["actions"].dtype == np.float32 and got["actions"].shape == (n, A)
        want = oracle_gaussian_draws(mean, ls, seed, counter)
        np.testing.assert_allclose(got["actions"], want, rtol=1e-4, atol=1e-4)
        lp64 = _log_density(got["actions"], mean, ls, np.float64)
        lp32 = _log_density(got["actions"], mean.astype(np.float32), ls, np.float32)
        d_kernel = np.abs(got["log_probs"] - lp64)
        d_f32 = np.abs(lp32.astype(np.float64) - lp64)
        bound = np.maximum(ATOL + RTOL * np.abs(lp64), 4 * d_f32)
        rule = "4x float32" if np.any(4 * d_f32 > ATOL + RTOL * np.abs(lp64)) else "atol/rtol"
        print(f"G {G} D {D} A {A} {regime} n {n}: log-prob max|diff| {d_kernel.max():.2e}, "
              f"float32 expression {d_f32.max():.2e}, bound by {rule}")
        assert np.all(d_kernel <= bound), (d_kernel.max(), d_f32.max())
        lean = run_act(agent, obs, dones, hx, seed, counter, means=False)
        for k in ("hx_out", "actions", "log_probs", "values"):
            assert np.array_equal(lean[k], got[k]), k


@pytest.mark.parametrize("G", WIDTHS)
def test_outputs_do_not_depend_on_batch_size_or_position(G):
    n, D, A = 4101, 17, 6
    agent = _agent(D, A, G, "spread")
    obs, dones, hx = _inputs(n, D, G, seed=21)
    big = run_act(agent, obs, dones, hx, seed=2, counter=5)
    small = run_act(agent, obs[:3], dones[:3], hx[:3], seed=2, counter=5)
    for k in big:   # same sample indices: the draw and its log-prob agree too
        assert np.array_equal(big[k][:3], small[k]), k
    obs2, dones2, hx2 = obs.copy(), dones.copy(), hx.copy()
    obs2[4098:], dones2[4098:], hx2[4098:] = obs[:3], dones[:3], hx[:3]
    moved = run_act(agent, obs2, dones2, hx2, seed=2, counter=5)
    for k in ("hx_out", "values", "means"):
        assert np.array_equal(moved[k][4098:], small[k]), k
    assert not np.array_equal(moved["actions"][4098:], small["actions"])
    # the same (seed, counter): the same bits; another counter: other draws, nothing else
    again = run_act(agent, obs, dones, hx, seed=2, counter=5)
    for k in big:
        assert np.array_equal(big[k], again[k]), k
    nxt = run_act(agent, obs, dones, hx, seed=2, counter=6)
    assert not np.array_equal(big["actions"], nxt["actions"])
    for k in ("hx_out", "values", "means"):
        assert np.array_equal(big[k], nxt[k]), k
    # the draws are standard normal around the mean
    ls = agent.network.actor_log_std.detach().cpu().numpy().reshape(A)
    z = (big["actions"] - big["means"]) / np.exp(ls)
    assert abs(z.mean()) < 5 / np.sqrt(z.size) and abs(z.std() - 1) < 0.02


def _categorical_agent(D, A, G):
    import gym_stub
    envs = gym_stub.SyncVectorEnv([lambda: gym_stub.SyntheticEnv(D, A)] * 4)
    cfg = diamond.RecurrentPPOConfig(rollout_steps=2, num_envs=4, verbose=False, gru_hidden_dim=G)
    agent = diamond.RecurrentPPO(None, cfg, envs=envs)
    assert agent.gru is not None and not agent.gru.gauss
    return agent


def test_argument_checks_on_a_live_handle():
    n, D, A, G = 5, 4, 2, 16
    agent = _agent(D, A, G, Nn=5, T=1)
    obs, dones, hx = _inputs(n, D, G, seed=1)
    o, d, h = _dev(agent, obs), _dev(agent, dones, torch.uint8), _dev(agent, hx)
    dev = agent.device
    hx_out = torch.full((n, G), 7.0, device=dev)
    act = torch.full((n, A), -3.0, device=dev)
    lp, v = torch.full((n,), 7.0, device=dev), torch.full((n,), 7.0, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    lib = agent.gru.lib
    params = agent.flat.flat.data_ptr()
    call = lambda step, m, p=params, handle=agent.gru.h: N.check(lib.dppo_gru_gauss_act_f32(
        handle, p, ctypes.byref(step), m, 1, 0, stream), "dppo_gru_gauss_act_f32")
    good = N.GruGaussStep(o.data_ptr(), d.data_ptr(), h.data_ptr(), hx_out.data_ptr(),
                          act.data_ptr(), lp.data_ptr(), v.data_ptr(), None)
    alias = N.GruGaussStep(o.data_ptr(), d.data_ptr(), h.data_ptr(), h.data_ptr(),
                           act.data_ptr(), lp.data_ptr(), v.data_ptr(), None)
    missing = N.GruGaussStep(o.data_ptr(), d.data_ptr(), h.data_ptr(), hx_out.data_ptr(),
                             act.data_ptr(), None, v.data_ptr(), None)
    for step, m, p in ((alias, n, params), (good, -1, params), (missing, n, params),
                       (good, n, params + 4)):
        with pytest.raises(ValueError):
            call(step, m, p)
    # the other head's entry points refuse the handle, and the Gaussian ones a categorical handle
    cat = _categorical_agent(D, A, G)
    cstep = N.GruStep(o.data_ptr(), d.data_ptr(), h.data_ptr(), hx_out.data_ptr(),
                      torch.zeros(n, dtype=torch.int32, device=dev).data_ptr(), lp.data_ptr(),
                      v.data_ptr(), None)
    with pytest.raises(ValueError, match="Gaussian"):
        N.check(lib.dppo_gru_act_f32(agent.gru.h, params, ctypes.byref(cstep), n, 1, 0, stream))
    with pytest.raises(ValueError, match="categorical"):
        call(good, n, cat.flat.flat.data_ptr(), cat.gru.h)
    z = torch.zeros(n, device=dev)
    zi = torch.zeros(n, dtype=torch.int32, device=dev)
    hp = N.HParams(gamma=0.99, gae_lambda=0.95, ppo_clip=0.15, value_loss_weight=1.0,
                   entropy_beta=0.01, grad_norm_clip=0.5, adam_beta1=0.9, adam_beta2=0.999,
                   adam_eps=1e-5, advantage_norm=1, lr=3e-4, adam_step=0)
    grad = torch.full((agent.flat.total + 8,), 7.0, device=dev)
    cb = N.GruBatch(o.data_ptr(), zi.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                    d.data_ptr(), h.data_ptr())
    with pytest.raises(ValueError, match="Gaussian"):
        N.check(lib.dppo_gru_minibatch_grad_f32(agent.gru.h, params, ctypes.byref(cb),
                                                zi.data_ptr(), n, n, ctypes.byref(hp),
                                                grad.data_ptr(), stream))
    gb = N.GruGaussBatch(o.data_ptr(), act.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(),
                         d.data_ptr(), h.data_ptr())
    cgrad = torch.full((cat.flat.total + 8,), 7.0, device=dev)
    with pytest.raises(ValueError, match="categorical"):
        N.check(lib.dppo_gru_gauss_minibatch_grad_f32(cat.gru.h, cat.flat.flat.data_ptr(),
                                                      ctypes.byref(gb), zi.data_ptr(), 1, 1,
                                                      ctypes.byref(hp), cgrad.data_ptr(), stream))
    call(good, 0)                                     # OK, no launch
    torch.cuda.synchronize()
    assert torch.all(hx_out == 7.0) and torch.all(act == -3.0)
    assert torch.all(lp == 7.0) and torch.all(v == 7.0)
    assert torch.all(grad == 7.0) and torch.all(cgrad == 7.0)
    # the handle still works
    call(good, n)
    torch.cuda.synchronize()
    mean, val, hn = oracle_step(_oracle_net(agent), obs, dones, hx)
    np.testing.assert_allclose(v.cpu().numpy(), val, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(hx_out.cpu().numpy(), hn, rtol=RTOL, atol=ATOL)
    assert torch.all(act != -3.0)
