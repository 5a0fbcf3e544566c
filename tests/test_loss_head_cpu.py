"""Loss head (csrc/losshead.hip): what can be checked without a device -- the opt-in flag, the
C ABI's argument validation and plan, and the case builder / float64 yardstick the GPU tests use
(tests/loss_head_cases.py)."""
import ctypes

import numpy as np
import pytest

import diamond
from diamond import _native as N

import loss_head_cases as C


def _cap():
    return N.ppo_loss_plan(1, 1)[2]


def test_flag_is_off_by_default():
    for cls in (diamond.PPO, diamond.ContinuousPPO, diamond.RecurrentPPO):
        assert cls.fused_loss is False, cls


def test_plan_is_monotone_and_cap_at_least_64():
    cap = _cap()
    assert cap >= 64
    for A in (1, 3, 4, 17, 64, cap):
        last_ws, last_grid = 0, 0
        for m in (1, 2, 63, 64, 65, 257, 4099, 65536, 1 << 20, 1 << 33):
            ws, grid, cap2 = N.ppo_loss_plan(m, A)
            assert cap2 == cap
            assert ws >= last_ws and grid >= last_grid and ws >= 1 and grid >= 1, (A, m)
            last_ws, last_grid = ws, grid
    # the grid is capped: from some m on a block takes further passes
    assert N.ppo_loss_plan(1 << 33, 64)[1] == N.ppo_loss_plan(1 << 20, 64)[1]


def _args(**over):
    """A dppo_loss_args whose pointers are non-null but never dereferenced: every call below must
    be refused before any HIP call."""
    p = 0x1000
    kw = dict(logits=p, log_std=p, values=p, idx=None, actions=p, old_log_probs=p, advantages=p,
              returns=p, d_logits=p, d_log_std=p, d_values=p, out=p, workspace=p, m=8,
              rollout_len=8, workspace_floats=N.ppo_loss_plan(8, 4)[0], act_dim=4, continuous=0,
              log_std_stride=0, ppo_clip=0.2, value_loss_weight=1.0, entropy_beta=0.01, scale=1.0)
    kw.update(over)
    return N.LossArgs(**kw)


@pytest.mark.parametrize("over, word", [
    (dict(logits=None), "NULL"), (dict(values=None), "NULL"), (dict(actions=None), "NULL"),
    (dict(old_log_probs=None), "NULL"), (dict(advantages=None), "NULL"),
    (dict(returns=None), "NULL"), (dict(d_logits=None), "NULL"), (dict(d_values=None), "NULL"),
    (dict(out=None), "NULL"), (dict(workspace=None), "NULL"),
    (dict(continuous=1, log_std=None), "NULL"), (dict(continuous=1, d_log_std=None), "NULL"),
    (dict(m=0), "m = 0"), (dict(m=-3), "m = -3"),
    (dict(act_dim=0), "act_dim"), (dict(act_dim=-1), "act_dim"),
    (dict(continuous=1, log_std_stride=3), "log_std_stride"),
    (dict(continuous=1, log_std_stride=-4), "log_std_stride"),
    (dict(workspace_floats=0), "workspace"),
])
def test_loss_arguments_are_refused_before_any_launch(over, word):
    lib = N.load()
    rc = lib.dppo_ppo_loss_f32(ctypes.byref(_args(**over)), None)
    assert rc == N.DPPO_EINVAL
    assert word in lib.dppo_last_error().decode()
    with pytest.raises(ValueError):
        N.check(rc, "dppo_ppo_loss_f32")


def test_act_dim_past_the_cap_and_short_workspace_are_refused():
    lib = N.load()
    cap = _cap()
    assert lib.dppo_ppo_loss_f32(ctypes.byref(_args(act_dim=cap + 1)), None) == N.DPPO_EINVAL
    assert str(cap) in lib.dppo_last_error().decode()
    need = N.ppo_loss_plan(4099, 64)[0]
    a = _args(m=4099, act_dim=64, rollout_len=4099, workspace_floats=need - 1)
    assert lib.dppo_ppo_loss_f32(ctypes.byref(a), None) == N.DPPO_EINVAL
    assert str(need) in lib.dppo_last_error().decode()
    assert lib.dppo_ppo_loss_f32(None, None) == N.DPPO_EINVAL
    with pytest.raises(ValueError):
        N.ppo_loss_plan(0, 4)
    with pytest.raises(ValueError):
        N.ppo_loss_plan(8, cap + 1)


@pytest.mark.parametrize("over", [
    dict(logits=None), dict(actions=None), dict(logp=None), dict(cont=1, log_std=None),
    dict(m=0), dict(A=0), dict(A=100000), dict(cont=1, stride=5), dict(B=0)])
def test_logp_arguments_are_refused_before_any_launch(over):
    p = 0x1000
    kw = dict(logits=p, log_std=p, stride=0, idx=None, actions=p, m=8, B=8, A=4, cont=0, logp=p)
    kw.update(over)
    lib = N.load()
    rc = lib.dppo_policy_logp_f32(kw["logits"], kw["log_std"], kw["stride"], kw["idx"],
                                  kw["actions"], kw["m"], kw["B"], kw["A"], kw["cont"],
                                  kw["logp"], None)
    assert rc == N.DPPO_EINVAL and lib.dppo_last_error()


CASES = C.sweep_cases(256)


def test_sweep_covers_the_listed_sizes():
    assert _cap() == 256  # the sweep above is built for this cap
    ms = {kw["m"] for _, kw in CASES}
    As = {kw["A"] for _, kw in CASES}
    assert set(C.M_SIZES) <= ms and set(C.A_SIZES) | {256} <= As
    assert {kw.get("hyper", 0) for _, kw in CASES} == {0, 1, 2}
    assert any(kw.get("use_idx") is False for _, kw in CASES)
    assert any(kw.get("scale") == 0.125 for _, kw in CASES)
    assert {kw.get("regime", "plain") for _, kw in CASES} == set(C.REGIMES)


@pytest.mark.parametrize("label, kw", CASES, ids=[c[0] for c in CASES])
def test_case_meets_branch_condition_and_analytic_backward_is_autograd(label, kw):
    c = C.make_case(**kw)
    # no sample within NEAR_BOUND of a clip bound, none left out
    assert C.branch_margin(c) >= C.NEAR_BOUND, (label, C.branch_margin(c))
    if c.m >= 6:
        i = c.gather
        for t in range(3):
            a = c.adv[i][c.third == t]
            if kw.get("regime") != "adv0":
                assert (a > 0).any() and (a < 0).any(), (label, t)
    if kw.get("regime") == "adv0":
        assert (c.adv[c.gather] == 0).any()
    if kw.get("regime") == "gaps":
        assert np.ptp(c.logits, axis=1).max() == 230.0
    parts64, g64 = C.torch_loss(c, __import__("torch").float64)
    parts_a, g_a = C.analytic(c)
    np.testing.assert_allclose(parts_a, parts64, rtol=1e-12, atol=1e-12)
    for k in g64:
        s = max(np.abs(g64[k]).max(), 1e-300)
        assert np.abs(g_a[k] - g64[k]).max() <= 1e-12 * max(s, 1.0), (label, k)


def test_sweep_covers_the_data_parallel_scales():
    for cont in (False, True):
        got = {(kw["scale"], kw["m"]) for _, kw in CASES if kw["cont"] == cont and "scale" in kw}
        assert {(s, m) for _, s in C.DP_SCALES for m in C.DP_M_SIZES} <= got
    assert [s for _, s in C.DP_SCALES] == [1 / 3, 5 / 7, 1 / 8] and C.DP_M_SIZES == [1, 2, 5, 65]


@pytest.mark.parametrize("cont, rows", C.PARTITION_HEADS, ids=C.PARTITION_HEAD_IDS)
@pytest.mark.parametrize("m, k", C.PARTITIONS)
def test_shares_of_a_minibatch_sum_to_the_whole_in_float64(m, k, cont, rows):
    """What the GPU partition test assumes: with scale = share / m the shares' gradient rows are
    the whole minibatch's rows and their losses add up to its loss (float64 autograd)."""
    torch = __import__("torch")
    c = C.partition_case(m, cont, rows)
    assert C.branch_margin(c) >= C.NEAR_BOUND and c.scale == 1.0
    parts, g = C.torch_loss(c, torch.float64)
    shares = [C.share(c, 0, k), C.share(c, k, m)]
    assert [s.m for s in shares] == [k, m - k] and abs(sum(s.scale for s in shares) - 1) < 1e-15
    got = [C.torch_loss(s, torch.float64) for s in shares]
    assert abs(sum(p[0] for p, _ in got) - parts[0]) <= 1e-12 * max(1.0, abs(parts[0]))
    for key in g:
        cat = np.concatenate([gs[key] for _, gs in got])
        assert np.abs(cat - g[key]).max() <= 1e-12 * max(1.0, np.abs(g[key]).max()), key


def test_on_policy_case_has_unit_ratio_in_float64():
    c = C.make_case(m=65, A=5, cont=False, on_policy=True, seed=2)
    lp = C._logp64(c.logits, c.log_std, c.actions[c.gather], c.cont)
    np.testing.assert_allclose(np.exp(lp - c.old_logp[c.gather]), 1.0, atol=1e-6)
