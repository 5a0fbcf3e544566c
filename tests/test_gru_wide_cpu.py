"""Host-side surface of the fused GRU kernels at gru_hidden_dim 16, 32 and 64 (csrc/gru.hip,
diamond.recurrent_ppo.fused_gru_shape): the flat layout libdppo reports for a G is
FlatParams' for the network with that G, the Python predicate is the documented set, and the
clip-regime guards of every per-width gradient case (tests/gru_wide_cases.py, the long ones and
the G = 16 ones included) hold on the float64 oracle alone, and the long cases reach the
multi-pass and many-slab code.
The kernels themselves: tests/test_gpu_gru_wide.py, tests/test_gpu_gru_wide_act.py."""
import ctypes
import itertools

import pytest
import torch

import gru_cases
import gru_wide_cases as W
from diamond import _native as N
from diamond.engine import FlatParams
from diamond.recurrent_ppo import RecurrentActorCriticNetwork, fused_gru_shape


def _dims(G, D, A, T=4, Nn=9, hidden=64):
    return N.GruDims(rollout_steps=T, num_envs=Nn, obs_dim=D, act_dim=A, hidden=hidden,
                     gru_hidden=G)


@pytest.mark.parametrize("G", [16, 32, 64])
@pytest.mark.parametrize("D,A", [(1, 1), (5, 3), (17, 6), (32, 16)])
def test_param_layout_is_flatparams_layout(G, D, A):
    import gym_stub
    lib = N.load()
    L = N.Layout()
    N.check(lib.dppo_gru_param_layout(ctypes.byref(_dims(G, D, A)), ctypes.byref(L)),
            "dppo_gru_param_layout")
    net = RecurrentActorCriticNetwork(gym_stub.Box(shape=(D,)), gym_stub.Discrete(A),
                                      cfg=W.config(G))
    flat = FlatParams(net, torch.device("cpu"))
    assert L.count == len(flat.offsets) == 14
    assert L.total == flat.total and L.n_real == sum(flat.numels)
    for i, (o, n, s) in enumerate(zip(flat.offsets, flat.numels, flat.shapes)):
        assert (L.offset[i], L.numel[i]) == (o, n), i
        assert (L.rows[i], L.cols[i]) == (s[0], s[1] if len(s) > 1 else 1), i


def test_predicate_is_the_documented_set(monkeypatch):
    monkeypatch.delenv("DPPO_GRU_WIDE", raising=False)
    want = lambda H, G, D, A: H == 64 and G in (16, 32, 64) and 1 <= D <= 32 and 1 <= A <= 16
    grid = itertools.product((32, 63, 64, 65, 128), (0, 8, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 128),
                             (0, 1, 2, 31, 32, 33, 64), (0, 1, 2, 15, 16, 17))
    n_true = 0
    for H, G, D, A in grid:
        assert fused_gru_shape(H, G, D, A) is want(H, G, D, A), (H, G, D, A)
        n_true += want(H, G, D, A)
    assert n_true == 3 * 4 * 4
    # the native twin (gru_validate, through dppo_gru_plan: no device needed) on the same grid,
    # where the dims are valid at all
    lib = N.load()
    out = (ctypes.c_int32 * 4)()
    for H, G, D, A in itertools.product((32, 64, 128), (8, 16, 17, 32, 48, 64, 128), (1, 32, 33),
                                        (1, 16, 17)):
        rc = lib.dppo_gru_plan(ctypes.byref(_dims(G, D, A, hidden=H)), out)
        assert (rc == 0) is want(H, G, D, A), (H, G, D, A, rc)


def test_wide_switch_sends_32_and_64_to_torch(monkeypatch):
    monkeypatch.setenv("DPPO_GRU_WIDE", "0")
    assert fused_gru_shape(64, 16, 8, 4) is True
    assert fused_gru_shape(64, 32, 8, 4) is False
    assert fused_gru_shape(64, 64, 8, 4) is False
    monkeypatch.setenv("DPPO_GRU_WIDE", "1")
    assert fused_gru_shape(64, 32, 8, 4) is True and fused_gru_shape(64, 64, 8, 4) is True


def test_envs_per_workgroup():
    """The figures the case shapes are built around are the kernel's own; slabs follow them."""
    lib = N.load()
    assert "dppo_gru_plan" in N.EXPORTED
    out = (ctypes.c_int32 * 4)()
    assert set(W.ENVS_PER_WG) == {16, *W.WIDTHS}
    for G, E in W.ENVS_PER_WG.items():
        for Nn in (1, E - 1, E, E + 1, 2 * E + 1, 8192):
            if Nn < 1:
                continue
            N.check(lib.dppo_gru_plan(ctypes.byref(_dims(G, 32, 16, Nn=Nn)), out), "dppo_gru_plan")
            assert out[0] == E and out[1] == -(-Nn // E)
            assert 0 < out[2] <= 160 * 1024 and out[3] == 4
    with pytest.raises(ValueError):
        N.check(lib.dppo_gru_plan(ctypes.byref(_dims(32, 4, 2)), None), "dppo_gru_plan")


def test_case_list_covers_the_issue():
    names = {str(c) for c in W.CASES}
    assert len(names) == len(W.CASES)
    for G in W.WIDTHS:
        E = W.ENVS_PER_WG[G]
        shapes = {c.shape for c in W.CASES if c.G == G}
        assert {(7, n, 5, 3) for n in (E - 1, E, E + 1, 2 * E + 1)} <= shapes
        assert set(W.KTAIL_SHAPES) <= shapes
        assert all(c.shape[0] <= 12 and c.shape[1] <= 70 for c in W.CASES)
    # G = 16: the env-count edges only (the rest are gru_cases.CASES), E + 1 among the latter
    E = W.ENVS_PER_WG[16]
    edge = [c for c in W.CASES if c.G == 16]
    assert not {c.shape for c in edge} & {c.shape for c in gru_cases.CASES}
    assert (7, E + 1, 5, 3) in {c.shape for c in gru_cases.CASES}
    for n in (E - 1, E, 2 * E + 1):
        runs = {(c.frac, c.on_policy) for c in edge if c.shape == (7, n, 5, 3)}
        assert runs == {(1.0, False), (0.4, False), (1.0, True)}, (n, runs)


@pytest.mark.parametrize("case", W.CASES, ids=str)
def test_wide_gradient_case_guards_hold(case):
    params, x, mb_idx, m_total = W.build(case)
    assert x["hx0"].shape == (case.shape[1], case.G)
    assert params["gru.weight_hh_l0"].shape == (3 * case.G, case.G)
    assert m_total == case.m_total_mul * len(mb_idx) and len(set(mb_idx.tolist())) == len(mb_idx)
    edge, share = W.guards(case, params, x, mb_idx)
    print(f"{case}: m={len(mb_idx)} nearest edge {edge:.3e} zero-policy-gradient share {share:.2f}")


@pytest.mark.parametrize("case", W.LONG_CASES, ids=str)
def test_long_gradient_case_guards_hold(case):
    test_wide_gradient_case_guards_hold(case)


def test_long_case_list_reaches_multi_pass_and_many_slabs():
    """What LONG_CASES is for, derived from ENVS_PER_WG and the kernel's 256 threads: per G a
    full and a partial workgroup whose S = T * ne samples need a second pass, one that needs a
    third, more than 100 gradient slabs (more than 64 at G = 16), and the class default shape (at
    8 envs per workgroup S = 256 exactly: the last size of one pass; at G = 16 that is the
    (16, 16) case, and the default shape is tests/test_gpu_gru_learn.py's) -- and the slab count
    is the plan's."""
    names = {str(c) for c in W.LONG_CASES}
    assert len(names) == len(W.LONG_CASES) and not names & {str(c) for c in W.CASES}
    known = {s[2:] for s in W.KTAIL_SHAPES}
    lib = N.load()
    out = (ctypes.c_int32 * 4)()
    assert {c.G for c in W.LONG_CASES} == set(W.ENVS_PER_WG)
    for G in W.ENVS_PER_WG:
        E = W.ENVS_PER_WG[G]
        many = 64 if G == 16 else 100
        cases = [c for c in W.LONG_CASES if c.G == G]
        assert all(c.shape[2:] in known for c in cases)
        full, partial, three, exact, slabs = set(), set(), set(), set(), set()
        for c in cases:
            T, Nn, D, A = c.shape
            wgs = W.workgroups(c)
            N.check(lib.dppo_gru_plan(ctypes.byref(_dims(G, D, A, T=T, Nn=Nn)), out),
                    "dppo_gru_plan")
            assert out[0] == E and out[1] == len(wgs) and sum(ne for ne, _ in wgs) == Nn
            full |= {c.shape for ne, S in wgs if ne == E and S > 256}
            partial |= {c.shape for ne, S in wgs if ne < E and S > 256}
            three |= {c.shape for ne, S in wgs if S > 512}
            exact |= {c.shape for ne, S in wgs if S == 256}
            slabs |= {c.shape for _ in wgs[many:]}
        default = W.config(G)
        if G in W.WIDTHS:
            assert (default.rollout_steps, default.num_envs) in {c.shape[:2] for c in cases}
            assert bool(exact) == (default.rollout_steps * E == 256)
        else:
            assert exact == {(16, 16, 4, 2)}
        for what in (full, partial, three, slabs):
            assert what, (G, full, partial, three, slabs)
            for shape in what:   # each off-policy at both fractions and on-policy at 1.0
                runs = {(c.frac, c.on_policy) for c in cases
                        if c.shape == shape and c.dones == "random"}
                assert runs == {(1.0, False), (0.4, False), (1.0, True)}, (G, shape, runs)
        assert W.MANY_ENVS in slabs and W.MANY_ENVS_HEAD % E == 0 and W.MANY_ENVS[1] % E != 0
        # the carry reset and the prefetch clamps at a T of more than one pass
        for d in ("env_always", "last"):
            hit = [c for c in cases if c.dones == d]
            assert hit and all(S > 256 for c in hit for _, S in W.workgroups(c)[:1])
            assert all(gru_cases.DONE_ENV < c.shape[1] for c in hit)
