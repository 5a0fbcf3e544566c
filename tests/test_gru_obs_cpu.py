"""Host-side surface of the fused GRU kernels' wide-observation range (33 <= obs_dim <= 128,
asked for with RecurrentPPOConfig.wide_observations / dppo_gru_dims.wide_obs; csrc/gru.hip,
diamond.recurrent_ppo.fused_gru_shape): without the flag the predicate is what it was, with it the
documented set; the flat layout and the plan at the new widths; and the clip-regime guards of
every case of tests/gru_obs_cases.py on the float64 oracle alone.
The kernels themselves: tests/test_gpu_gru_obs.py, test_gpu_gru_obs_act.py, test_gpu_gru_obs_learn.py."""
import ctypes
import dataclasses
import itertools

import pytest
import torch

import gru_obs_cases as O
import gru_wide_cases as W
from diamond import _native as N
from diamond.engine import FlatParams
from diamond.recurrent_ppo import (RecurrentActorCriticNetwork, RecurrentPPOConfig,
                                   fused_gru_shape)


def _dims(G, D, A, wide_obs, T=4, Nn=9, hidden=64):
    return N.GruDims(rollout_steps=T, num_envs=Nn, obs_dim=D, act_dim=A, hidden=hidden,
                     gru_hidden=G, wide_obs=wide_obs)


def test_predicate_without_and_with_the_flag(monkeypatch):
    monkeypatch.delenv("DPPO_GRU_WIDE", raising=False)
    narrow = lambda H, G, D, A: H == 64 and G in (16, 32, 64) and 1 <= D <= 32 and 1 <= A <= 16
    wide = lambda H, G, D, A: H == 64 and G in (16, 32, 64) and 1 <= D <= 128 and 1 <= A <= 16
    # the grid of test_gru_wide_cpu.py::test_predicate_is_the_documented_set, D probed further
    grid = list(itertools.product(
        (32, 63, 64, 65, 128), (0, 8, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 128),
        (0, 1, 2, 31, 32, 33, 64, 128, 129), (0, 1, 2, 15, 16, 17)))
    n_wide = 0
    for H, G, D, A in grid:
        assert fused_gru_shape(H, G, D, A) is narrow(H, G, D, A), (H, G, D, A)
        assert fused_gru_shape(H, G, D, A, False) is narrow(H, G, D, A), (H, G, D, A)
        assert fused_gru_shape(H, G, D, A, wide_obs=True) is wide(H, G, D, A), (H, G, D, A)
        n_wide += wide(H, G, D, A)
    assert n_wide == 3 * 7 * 4
    # the native twin (gru_validate through dppo_gru_plan: no device needed)
    lib = N.load()
    out = (ctypes.c_int32 * 4)()
    for H, G, D, A in itertools.product((32, 64, 128), (8, 16, 17, 32, 48, 64, 128),
                                        (1, 32, 33, 128, 129), (1, 16, 17)):
        for flag, want in ((0, narrow), (1, wide), (7, wide)):
            rc = lib.dppo_gru_plan(ctypes.byref(_dims(G, D, A, flag, hidden=H)), out)
            assert (rc == 0) is want(H, G, D, A), (H, G, D, A, flag, rc)
    # the field is the struct's last and zero unless given
    assert N.GruDims._fields_[-1][0] == "wide_obs"
    assert N.GruDims(rollout_steps=1, num_envs=1, obs_dim=1, act_dim=1, hidden=64,
                     gru_hidden=16).wide_obs == 0


def test_width_switch_still_sends_32_and_64_to_torch(monkeypatch):
    monkeypatch.setenv("DPPO_GRU_WIDE", "0")
    for D in (8, 33, 128):
        assert fused_gru_shape(64, 16, D, 4, wide_obs=True) is True
        assert fused_gru_shape(64, 32, D, 4, wide_obs=True) is False
        assert fused_gru_shape(64, 64, D, 4, wide_obs=True) is False
    monkeypatch.setenv("DPPO_GRU_WIDE", "1")
    assert fused_gru_shape(64, 32, 128, 4, wide_obs=True) is True
    assert fused_gru_shape(64, 64, 128, 4, wide_obs=True) is True
    assert fused_gru_shape(64, 64, 128, 4) is False


@pytest.mark.parametrize("G", O.WIDTHS)
@pytest.mark.parametrize("D,A", [(33, 2), (100, 6), (128, 16)])
def test_param_layout_is_flatparams_layout(G, D, A):
    import gym_stub
    lib = N.load()
    L = N.Layout()
    N.check(lib.dppo_gru_param_layout(ctypes.byref(_dims(G, D, A, 1)), ctypes.byref(L)),
            "dppo_gru_param_layout")
    net = RecurrentActorCriticNetwork(gym_stub.Box(shape=(D,)), gym_stub.Discrete(A),
                                      cfg=W.config(G))
    flat = FlatParams(net, torch.device("cpu"))
    assert L.count == len(flat.offsets) == 14
    assert L.total == flat.total and L.n_real == sum(flat.numels)
    for i, (o, n, s) in enumerate(zip(flat.offsets, flat.numels, flat.shapes)):
        assert (L.offset[i], L.numel[i]) == (o, n), i
        assert (L.rows[i], L.cols[i]) == (s[0], s[1] if len(s) > 1 else 1), i


@pytest.mark.parametrize("G", O.WIDTHS)
def test_plan_at_the_full_width(G):
    lib = N.load()
    E = W.ENVS_PER_WG[G]
    narrow, wide = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    for Nn in (1, E, 2 * E + 1, 8192):
        N.check(lib.dppo_gru_plan(ctypes.byref(_dims(G, 32, 16, 0, Nn=Nn)), narrow), "plan")
        N.check(lib.dppo_gru_plan(ctypes.byref(_dims(G, 128, 16, 1, Nn=Nn)), wide), "plan")
        assert (wide[0], wide[1], wide[3]) == (narrow[0], narrow[1], narrow[3])
        assert (wide[0], wide[1], wide[3]) == (E, -(-Nn // E), 4)
        assert 0 < narrow[2] < wide[2] <= 160 * 1024
        # phase A holds Wb [64][D] beside Wih: 96 more columns of 64 floats
        assert wide[2] - narrow[2] == 64 * 96 * 4
    # D <= 32 plans the same with the flag on
    N.check(lib.dppo_gru_plan(ctypes.byref(_dims(G, 32, 16, 1)), wide), "plan")
    N.check(lib.dppo_gru_plan(ctypes.byref(_dims(G, 32, 16, 0)), narrow), "plan")
    assert list(wide) == list(narrow)


def test_config_field():
    assert RecurrentPPOConfig().wide_observations is False
    names = [f.name for f in dataclasses.fields(RecurrentPPOConfig)]
    assert names.index("wide_observations") > names.index("gae_bitexact")
    assert names[-1] == "wide_observations"
    assert RecurrentPPOConfig(wide_observations=True).wide_observations is True


def test_case_list_covers_the_issue():
    names = [str(c) for c in O.CASES + O.LONG_CASES]
    assert len(set(names)) == len(names)
    assert not set(names) & {str(c) for c in W.CASES + W.LONG_CASES}
    for G in O.WIDTHS:
        E = W.ENVS_PER_WG[G]
        want = [(5, 3, 33, 2), (7, E + 1, 64, 3), (3, 5, 65, 4), (6, 2 * E + 1, 100, 6),
                (4, 9, 127, 16), (9, 18, 128, 16)]
        cases = [c for c in O.CASES if c.G == G]
        assert all(c.seed_shift == 0 and c.dones == "random" for c in cases)
        plain = [c for c in cases if c.obs_scale == 1.0]
        for s in want:
            runs = {(c.frac, c.on_policy) for c in plain if c.shape == s}
            both = {(1.0, False), (0.4, False)}
            assert runs == both | ({(1.0, True)} if s in (want[1], want[5]) else set()), (G, s)
        assert {c.shape for c in plain} == set(want)
        linear = [c for c in cases if c.obs_scale != 1.0]
        assert all(c.obs_scale == 0.25 and not c.on_policy for c in linear)
        assert {(c.shape, c.frac) for c in linear} == {(s, f) for s in (want[1], want[5])
                                                       for f in (1.0, 0.4)}
        long = [c for c in O.LONG_CASES if c.G == G]
        assert {c.shape for c in long} == {O.LONG_SHAPE[G]} and O.LONG_SHAPE[G][2:] == (128, 3)
        assert {(c.frac, c.dones) for c in long} == {(1.0, "random"), (0.4, "random"),
                                                     (1.0, "env_always"), (1.0, "last")}
        assert all(c.seed_shift == 0 for c in long)
        # more than one pass of the kernel's 256 threads in a full workgroup
        for c in long:
            ne, S = W.workgroups(c)[0]
            assert ne == E and S > 256, (G, S)
    assert O.LONG_SHAPE == {16: (20, 29, 128, 3), 32: (40, 15, 128, 3), 64: (72, 7, 128, 3)}


@pytest.mark.parametrize("case", O.CASES + O.LONG_CASES, ids=str)
def test_obs_gradient_case_guards_hold(case):
    params, x, mb_idx, m_total = O.build(case)
    T, Nn, D, A = case.shape
    assert 32 < D <= 128 and x["obs"].shape == (T, Nn, D)
    assert params["base.0.weight"].shape == (64, D)
    assert x["hx0"].shape == (Nn, case.G)
    assert m_total == len(mb_idx) and len(set(mb_idx.tolist())) == len(mb_idx)
    edge, share = O.guards(case, params, x, mb_idx)
    print(f"{case}: m={len(mb_idx)} nearest edge {edge:.3e} zero-policy-gradient share {share:.2f}")
