"""Host-side surface of RecurrentContinuousPPO's fused kernels (csrc/gru.hip's gauss entry points,
diamond/recurrent_continuous_ppo.py): the predicate and plan (the categorical ones'), the 15-tensor
flat layout, the config, exports and network, the float64 yardstick tests/gru_gauss_oracle.py
against the package's own network and loss on the CPU, and the clip-regime guards of every case of
tests/gru_gauss_cases.py on the oracle alone.
The kernels themselves: tests/test_gpu_gru_gauss.py, test_gpu_gru_gauss_act.py,
test_gpu_gru_gauss_learn.py."""
import ctypes
import dataclasses
import itertools

import numpy as np
import pytest
import torch

import diamond
import gru_gauss_cases as C
import gru_gauss_oracle as GO
from diamond import _native as N
from diamond.continuous_ppo import JointNormal
from diamond.engine import FlatParams, torch_ppo_terms
from diamond.recurrent_continuous_ppo import (RecurrentContinuousActorCriticNetwork,
                                              RecurrentContinuousPPOConfig)
from diamond.recurrent_ppo import RecurrentPPOConfig


def _dims(G, D, A, wide_obs, T=4, Nn=9, hidden=64):
    return N.GruDims(rollout_steps=T, num_envs=Nn, obs_dim=D, act_dim=A, hidden=hidden,
                     gru_hidden=G, wide_obs=wide_obs)


def test_gauss_plan_accepts_what_the_categorical_plan_accepts():
    lib = N.load()
    cat, gau = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    ok = 0
    # the native grid of test_gru_obs_cpu.py::test_predicate_without_and_with_the_flag
    for H, G, D, A in itertools.product((32, 64, 128), (8, 16, 17, 32, 48, 64, 128),
                                        (1, 32, 33, 128, 129), (1, 16, 17)):
        for flag in (0, 1):
            d = _dims(G, D, A, flag, hidden=H)
            rc_c = lib.dppo_gru_plan(ctypes.byref(d), cat)
            rc_g = lib.dppo_gru_gauss_plan(ctypes.byref(d), gau)
            assert rc_c == rc_g, (H, G, D, A, flag, rc_c, rc_g)
            if rc_c == 0:
                ok += 1
                assert (gau[0], gau[1], gau[3]) == (cat[0], cat[1], cat[3])
                # exp(-log_std) and log_std, 16 floats each, behind the categorical image
                assert gau[2] - cat[2] == 2 * 16 * 4 and gau[2] <= 160 * 1024
    assert ok == 3 * (2 * 2 + 4 * 2)
    assert lib.dppo_gru_gauss_plan(ctypes.byref(_dims(16, 4, 1, 0)), None) == N.DPPO_EINVAL


@pytest.mark.parametrize("G", C.WIDTHS)
@pytest.mark.parametrize("D,A,wide", [(4, 1, 0), (17, 6, 0), (32, 16, 0), (100, 6, 1)])
def test_gauss_param_layout_is_flatparams_layout(G, D, A, wide):
    import gym_stub
    L = N.Layout()
    N.check(N.load().dppo_gru_gauss_param_layout(ctypes.byref(_dims(G, D, A, wide)),
                                                 ctypes.byref(L)), "layout")
    net = RecurrentContinuousActorCriticNetwork(gym_stub.Box(shape=(D,)), gym_stub.Box(shape=(A,)),
                                                cfg=C.config(G))
    assert [n for n, _ in net.named_parameters()] == GO.PARAM_NAMES
    flat = FlatParams(net, torch.device("cpu"))
    assert L.count == len(flat.offsets) == 15
    assert (L.offset[0], L.rows[0], L.cols[0], L.numel[0]) == (0, 1, A, A)
    assert L.total == flat.total and L.n_real == sum(flat.numels)
    for i, (o, n, s) in enumerate(zip(flat.offsets, flat.numels, flat.shapes)):
        assert (L.offset[i], L.numel[i]) == (o, n) and o % 16 == 0, i
        assert (L.rows[i], L.cols[i]) == (s[0], s[1] if len(s) > 1 else 1), i


def test_config_and_exports():
    base = [(f.name, f.type, f.default) for f in dataclasses.fields(RecurrentPPOConfig)]
    mine = [(f.name, f.type, f.default) for f in dataclasses.fields(RecurrentContinuousPPOConfig)]
    assert mine == base and mine[-1][0] == "wide_observations"
    old = ["PPO", "PPOConfig", "RecurrentPPO", "RecurrentPPOConfig", "ContinuousPPO",
           "ContinuousPPOConfig"]
    assert diamond.__all__[:6] == old
    assert {"RecurrentContinuousPPO", "RecurrentContinuousPPOConfig"} <= set(diamond.__all__)
    for n in diamond.__all__:
        assert hasattr(diamond, n)
    R = diamond.RecurrentContinuousPPO
    assert (R.fused_gru, R.fused_rollout, R.fused_loss, R.fused_core) == (True, False, False, False)
    for n in ("rollout", "calculate_advantage", "learn", "train"):
        assert callable(getattr(R, n))
    for s in ("dppo_gru_gauss_param_layout", "dppo_gru_gauss_plan", "dppo_gru_gauss_create",
              "dppo_gru_gauss_minibatch_grad_f32", "dppo_gru_gauss_act_f32"):
        assert s in N.EXPORTED and hasattr(N.load(), s)


def test_network_asserts_and_init():
    import gym_stub
    with pytest.raises(AssertionError):
        RecurrentContinuousActorCriticNetwork(gym_stub.Box(shape=(4,)), gym_stub.Discrete(3),
                                              cfg=C.config(16))
    net = C.network(8, 3, 16)
    assert torch.count_nonzero(net.actor_log_std).item() == 0
    assert tuple(net.actor_log_std.shape) == (1, 3)
    # orthogonal at gain sqrt(2), not the categorical agent's 0.01 output layer
    w = net.actor_mean_head[-1].weight.detach()
    np.testing.assert_allclose((w @ w.t()).numpy(), 2.0 * np.eye(3), atol=1e-5)
    assert all(torch.count_nonzero(m.bias).item() == 0 for m in net.modules()
               if isinstance(m, torch.nn.Linear))


def _small(seed=3, T=3, Nn=2, D=5, A=3, G=16):
    case = C.Case("cpu", (T, Nn, D, A), G=G, regime="spread", seed_shift=seed)
    return case, C.build(case)


def test_oracle_log_prob_and_entropy_equal_jointnormal_on_the_package_network():
    case, (params, x, _, _) = _small()
    T, Nn, D, A = case.shape
    net = C.network(D, A, case.G).double()
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(params[n]).double())
        hx = torch.from_numpy(x["hx0"]).double()[None]
        mean, ls, values, _ = net.get_means_log_stds_values_and_hx(
            torch.from_numpy(x["obs"]).double(), hx, torch.from_numpy(x["prev_dones"]))
        dist = JointNormal(loc=mean, scale=ls.exp())
        want_lp = dist.log_prob(torch.from_numpy(x["actions"]).double()).numpy()
        want_en = dist.entropy().numpy()
    assert mean.shape == (T, Nn, A) and ls.shape == mean.shape and values.shape == (T, Nn)
    lp, en = GO.log_probs(params, x["obs"], x["actions"], x["prev_dones"], x["hx0"], entropy=True)
    np.testing.assert_allclose(lp, want_lp, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(en, want_en, rtol=1e-12, atol=1e-12)
    m, v = GO.forward(params, x["obs"], x["prev_dones"], x["hx0"])
    np.testing.assert_allclose(m, mean.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(v, values.numpy(), rtol=1e-12, atol=1e-12)


def test_oracle_minibatch_grads_equal_backward_through_the_package_network():
    case, (params, x, _, _) = _small(seed=5, T=4, Nn=3)
    T, Nn, D, A = case.shape
    mb_idx = np.array([0, 3, 4, 7, 10, 11], np.int64)
    clip, vf, ent = 0.15, 0.7, 0.03
    sums, ref = GO.minibatch_grads(params, x["obs"], x["actions"], x["old_log_probs"],
                                   x["advantages"], x["returns"], x["prev_dones"], x["hx0"],
                                   mb_idx, len(mb_idx), clip, vf, ent)
    net = C.network(D, A, case.G).double()
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(params[n]).double())
    d = lambda k: torch.from_numpy(np.asarray(x[k])).double()
    mean, ls, values, _ = net.get_means_log_stds_values_and_hx(
        d("obs"), d("hx0")[None], torch.from_numpy(x["prev_dones"]))
    idx = torch.from_numpy(mb_idx)
    flat = lambda t: t.reshape(-1, *t.shape[2:])[idx]
    loss, l_pi, l_v, en, _ = torch_ppo_terms(
        flat(mean), flat(values), flat(ls), flat(d("actions")), flat(d("old_log_probs")),
        flat(d("advantages")), flat(d("returns")), clip, vf, ent, True)
    loss.backward()
    m = len(mb_idx)
    np.testing.assert_allclose(sums / m, [l_pi.item(), l_v.item(), en.item()], rtol=1e-12)
    scale = max(np.abs(g).max() for g in ref.values())
    for n, p in net.named_parameters():
        assert np.abs(p.grad.numpy() - ref[n]).max() <= 1e-12 * scale, n
    assert np.abs(ref["actor_log_std"]).min() > 0


def test_case_list_covers_the_issue():
    names = [str(c) for c in C.CASES]
    assert len(set(names)) == len(names)
    for G in C.WIDTHS:
        E = 256 // G
        want = [(5, 3, 4, 1), (7, E + 1, 8, 3), (3, 5, 5, 6), (6, 2 * E + 1, 17, 6), (4, 9, 32, 16)]
        assert C.shapes(G) == want
        for regime in C.REGIMES:
            cs = [c for c in C.CASES if c.G == G and c.regime == regime
                  and c.m_total_mul == 1 and c.dones == "random" and c.clip == 0.15]
            for s in want + [(3, 5, 65, 4)]:
                runs = {(c.frac, c.on_policy) for c in cs if c.shape == s and not c.tail}
                both = {(1.0, False), (0.4, False)}
                assert runs == both | ({(1.0, True)} if s in (want[1], want[4]) else set()), (G, s)
            assert all(c.wide_obs == (c.shape[2] > 32) for c in cs)
            assert sum(c.tail for c in cs) == 1
        rest = [c for c in C.CASES if c.G == G]
        assert any(c.m_total_mul == 2 for c in rest)
        assert any((c.clip, c.vf, c.ent) != (0.15, 1.0, 0.01) for c in rest)
        assert {c.dones for c in rest if c.shape == want[3]} == {"random", "env_always", "last"}


@pytest.mark.parametrize("case", C.CASES, ids=str)
def test_gauss_gradient_case_guards_hold(case):
    params, x, mb_idx, m_total = C.build(case)
    T, Nn, D, A = case.shape
    assert x["actions"].shape == (T, Nn, A) and x["actions"].dtype == np.float32
    assert params["actor_log_std"].shape == (1, A)
    if case.regime == "zero":
        assert not params["actor_log_std"].any()
    else:
        ls = params["actor_log_std"]
        assert ls.min() >= -1.5 and ls.max() <= 0.5 and np.abs(ls).min() > 0
    if case.tail:
        mean, _ = GO.forward(params, x["obs"], x["prev_dones"], x["hx0"])
        z = (x["actions"] - mean) / np.exp(params["actor_log_std"].astype(np.float64))
        np.testing.assert_allclose(np.abs(z), 4.0, rtol=1e-5)
    assert m_total == case.m_total_mul * len(mb_idx)
    edge, share = C.guards(case, params, x, mb_idx)
    print(f"{case}: m={len(mb_idx)} nearest edge {edge:.3e} zero-policy-gradient share {share:.2f}")
