"""The cases of tests/test_gpu_wide_large.py, examined without a GPU (tests/wide_large_cases.py).

1. The shape predicate, both ways: the large heads (hidden 64, obs_dim <= 384, act_dim <= 32, past
   one of the earlier limits, one rank) are "wide", DPPO_WIDE=0 turns them off, and the shapes the
   earlier tests pin to the generic path stay there.
2. The tables' coverage: every new wide_mb_kernel<64, CONT, NB1, false, AB> once, a 16-column
   block boundary on each side of every new NB1, the Humanoid widths, the action counts around the
   second block.
3. On the inputs of every gradient case (on-policy, off-policy, the m = 7 tile) the float32 oracle
   alone is within the GPU module's bounds of the float64 oracle (wide_mb_cases.check_gradient):
   a correct float32 kernel meets them.  The records are the float32 oracle's here and the
   kernel's own on the GPU.
4. The bounds see what the new code could leave out.  On every width and action case the float32
   oracle's gradient is turned down with
     a. dW1's columns from 128 on zero (an NB1 that stops at the old eight blocks),
     b. rows from 16 on of dWo, d bo and d log_std zero (the second action block not stored),
     c. the last action's row of dWo zero (a slab guard one action short),
   wherever the mutation changes anything: a needs D > 128 and b needs A > 16, which leaves out
   the D = 8 action cases for a and A = 15, 16 for b (asserted below).
5. The discrete draws of the new sampler inputs stay decided: the share of samples farther than
   CLEAR_MARGIN from every CDF boundary is at least wide_act_cases.MIN_CLEAR in the NumPy
   restatement alone.
"""
import os

import numpy as np
import pytest

import gpu_helpers as G
import wide_act_cases as W
import wide_large_cases as LC
import wide_mb_cases as C
from diamond.engine import fused_shape_class
from oracle import ppo_np as P
from test_gpu_rollout_ckpt import philox4x32_10, u01


# ---------------------------------------------------------------------------------------------
# 1. the predicate
# ---------------------------------------------------------------------------------------------
NEW_WIDE = [(64, 129, 1), (64, 129, 16), (64, 348, 17), (64, 376, 17), (64, 384, 32), (64, 384, 1),
            (64, 8, 17), (64, 1, 32), (64, 32, 17), (64, 33, 17), (64, 128, 32), (64, 40, 17)]
# (hidden, D, A, world, wide_ranks)
PINNED_NONE = [(128, 129, 2, 1, False), (128, 8, 17, 1, False), (128, 129, 4, 2, True),
               (128, 8, 17, 2, True), (256, 8, 4, 1, False), (256, 8, 4, 2, True),
               (64, 385, 2, 1, False), (64, 8, 33, 1, False), (64, 385, 33, 1, False),
               (64, 129, 4, 2, False), (64, 129, 4, 2, True), (64, 40, 17, 2, True),
               (64, 8, 17, 2, False), (64, 8, 17, 8, True), (64, 376, 17, 2, True),
               (96, 200, 4, 1, False), (64, 0, 4, 1, False), (64, 200, 0, 1, False)]


def test_large_heads_are_wide_on_one_rank():
    for Hd, D, A in NEW_WIDE:
        assert LC.is_large(Hd, D, A)
        assert fused_shape_class(Hd, D, A) == "wide", (Hd, D, A)
        assert fused_shape_class(Hd, D, A, 1, wide_ranks=True) == "wide", (Hd, D, A)
    for D, A, _cont in LC.INSTANTIATIONS + LC.width_shapes() + LC.action_shapes():
        assert fused_shape_class(LC.HID, D, A) == "wide", (D, A)


def test_pinned_shapes_stay_generic():
    for Hd, D, A, world, wr in PINNED_NONE:
        assert fused_shape_class(Hd, D, A, world, wide_ranks=wr) is None, (Hd, D, A, world, wr)
    # the earlier classes are what they were
    assert fused_shape_class(64, 32, 16) == "tuned" and fused_shape_class(64, 32, 16, 8) == "tuned"
    assert fused_shape_class(64, 128, 16) == "wide" and fused_shape_class(128, 128, 16) == "wide"
    assert fused_shape_class(64, 128, 16, 2, wide_ranks=True) == "wide"
    assert fused_shape_class(64, 128, 16, 2) is None


def test_dppo_wide_0_turns_the_large_heads_off(monkeypatch):
    monkeypatch.setenv("DPPO_WIDE", "0")
    for Hd, D, A in NEW_WIDE:
        assert fused_shape_class(Hd, D, A) is None
    assert fused_shape_class(64, 32, 16) == "tuned"
    assert os.environ["DPPO_WIDE"] == "0"


# ---------------------------------------------------------------------------------------------
# 2. coverage of the tables
# ---------------------------------------------------------------------------------------------
def test_every_new_instantiation_once():
    got = [LC.instantiation_of(c[3:6]) for c in LC.cases_of("I")]
    assert set(got) == LC.NEW and len(got) == len(LC.NEW) == 18
    assert all(c[9] == 379 and c[2] == 64 for c in LC.cases_of("I"))
    # none of them is an instantiation the earlier tests reach
    assert all(LC.is_large(*c[2:5]) for c in LC.small_cases())
    # 12 tiles on 6 workgroups of two tiles, the last tile partial
    assert C.wide_grid(379, C.MI355X_CUS) == 6 and C.tiles_per_group(379, C.S, 6) == (2, 2)
    assert LC.T * LC.NN == 384 and 379 % C.S != 0


def test_width_table():
    ds = [c[3] for c in LC.cases_of("W")]
    assert ds == [129, 143, 144, 145, 191, 192, 193, 255, 256, 257, 348, 376, 383, 384]
    # a D16 boundary on each side of every new NB1, and the block counts in between
    assert {LC.nb1(d) for d in ds} == {12, 16, 24}
    for lo, hi in ((128, 129), (192, 193), (256, 257)):
        assert LC.nb1(lo) < LC.nb1(hi) and hi in ds
    assert LC.nb1(192) == 12 and LC.nb1(256) == 16 and LC.nb1(384) == 24
    assert {C.ncb1(d) for d in ds} == {9, 10, 12, 13, 16, 17, 22, 24}
    assert all(c[4] == 17 for c in LC.cases_of("W"))
    assert [c[3:6] for c in LC.cases_of("W") if c[5]] == [(348, 17, True), (376, 17, True)]
    assert C.wide_grid(71, C.MI355X_CUS) == 1 and C.tiles_per_group(71, C.S, 1) == (3, 3)


def test_action_table():
    c = LC.cases_of("C")
    for cont in (False, True):
        assert sorted(x[4] for x in c if x[3] == 136 and x[5] == cont) == [15, 16, 17, 20, 31, 32]
        assert sorted(x[4] for x in c if x[3] == 8 and x[5] == cont) == [17, 32]
    assert len(c) == 16
    grid = C.wide_grid(135, C.MI355X_CUS)
    assert grid == 2 and C.tiles_per_group(135, C.S, grid) == (2, 3)
    assert C.wide_grid(7, C.MI355X_CUS) == 1


def test_seeds_are_distinct():
    seeds = [c[1] for c in LC.small_cases()]
    assert len(set(seeds)) == len(seeds)
    assert not set(seeds) & {c[1] for c in C.small_cases()}


# ---------------------------------------------------------------------------------------------
# 3. the float32 oracle meets the bounds
# ---------------------------------------------------------------------------------------------
def _oracles(case, mb=None, params=None, idx=None):
    _grp, seed, Hd, D, A, cont, T, Nn, M, m = case
    L, names, own, _flat, host = C.inputs(seed, Hd, D, A, cont, T, Nn, M)
    rec = C.oracle_records(own, host, cont)
    if idx is None:
        idx = C.minibatch_idx(seed, T * Nn, m if mb is None else mb)
    p = own if params is None else params
    ref64 = C.oracle_gradient(p, host, cont, rec, idx, np.float64)
    ref32 = C.oracle_gradient(p, host, cont, rec, idx, np.float32)
    return L, names, ref64, ref32, rec


def _within(case, what, **kw):
    L, names, ref64, ref32, _ = _oracles(case, **kw)
    return C.check_gradient(L, names, G.flat_of(L, names, ref32[2]), C.loss_terms(ref32), ref64,
                            f"float32 oracle {what} {LC.case_id(case)}")


_ALL = LC.small_cases()
_SWEEP = LC.sweep_cases()


@pytest.mark.parametrize("case", _ALL, ids=[LC.case_id(c) for c in _ALL])
def test_float32_oracle_within_the_gradient_bounds(case):
    _within(case, "on-policy")


@pytest.mark.parametrize("case", LC.cases_of("I"), ids=[LC.case_id(c) for c in LC.cases_of("I")])
def test_float32_oracle_within_the_gradient_bounds_off_policy(case):
    """The off-policy recipe is not vacuous (a full minibatch clear of the clip bounds, ratios on
    both sides of them) and the float32 oracle meets the bounds on it."""
    _L, _names, _r64, _r32, rec = _oracles(case)
    new, _flat = LC.offpolicy_params(case)
    idx, reg = LC.offpolicy_idx(case, new, rec)
    assert idx.size == case[9] and len(np.unique(idx)) == idx.size and (reg >= 0).all()
    assert (reg == 0).any() and (reg > 0).any(), np.bincount(reg, minlength=5)
    _within(case, "off-policy", params=new, idx=idx)


@pytest.mark.parametrize("case", _SWEEP, ids=[LC.case_id(c) for c in _SWEEP])
def test_float32_oracle_within_the_gradient_bounds_one_partial_tile(case):
    _within(case, "m=7", mb=LC.TINY_MB)


# ---------------------------------------------------------------------------------------------
# 4. the bounds resolve what the new code could leave out
# ---------------------------------------------------------------------------------------------
def _rejected(L, names, grads, ref32, ref64, what):
    try:
        C.check_gradient(L, names, G.flat_of(L, names, grads), C.loss_terms(ref32), ref64, what)
    except AssertionError:
        return True
    return False


def _head(cont):
    return "actor_mean_head" if cont else "actor_head"


def _mutations(case, ref32):
    """{name: mutated float32-oracle gradient} of the mutations that change anything at the case"""
    _grp, _seed, _Hd, D, A, cont, *_ = case
    head = _head(cont)
    out = {}
    if D > 128:
        g = {n: np.array(v) for n, v in ref32[2].items()}
        g["base.0.weight"][:, 128:] = 0
        out["a: dW1 columns >= 128"] = g
    if A > 16:
        g = {n: np.array(v) for n, v in ref32[2].items()}
        g[f"{head}.2.weight"][16:, :] = 0
        g[f"{head}.2.bias"][16:] = 0
        if cont:
            g["actor_log_std"][..., 16:] = 0
        out["b: head rows >= 16"] = g
    g = {n: np.array(v) for n, v in ref32[2].items()}
    g[f"{head}.2.weight"][-1, :] = 0
    out["c: last action row"] = g
    return out


@pytest.mark.parametrize("case", _SWEEP, ids=[LC.case_id(c) for c in _SWEEP])
def test_bounds_resolve_the_mutations(case):
    L, names, ref64, ref32, _ = _oracles(case)
    muts = _mutations(case, ref32)
    assert ("a: dW1 columns >= 128" in muts) == (case[3] > 128)
    assert ("b: head rows >= 16" in muts) == (case[4] > 16)
    for what, g in muts.items():
        assert _rejected(L, names, g, ref32, ref64, f"{what} {LC.case_id(case)}"), what


def test_mutations_cover_the_tables():
    """a runs at every width case and every D = 136 action case, b at every width case and every
    action count above 16, c everywhere."""
    a = [c for c in _SWEEP if c[3] > 128]
    b = [c for c in _SWEEP if c[4] > 16]
    assert set(LC.cases_of("W")) <= set(a) and set(LC.cases_of("W")) <= set(b)
    assert {c[3:6] for c in _SWEEP} - {c[3:6] for c in a} == \
        {(8, A, cont) for A in (17, 32) for cont in (False, True)}
    assert {c[3:6] for c in _SWEEP} - {c[3:6] for c in b} == \
        {(136, A, cont) for A in (15, 16) for cont in (False, True)}


# ---------------------------------------------------------------------------------------------
# 5. the discrete draws stay decided
# ---------------------------------------------------------------------------------------------
def _clear_share(params, obs):
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    logits = P.forward(p64, obs, False, np.float64)["out"]
    want, clear = W.categorical_oracle(logits, LC.SEED, LC.COUNTER, philox4x32_10, u01)
    return want, float(clear.mean())


@pytest.mark.parametrize("shape", [s for s in LC.ACT_SHAPES if not s[2]], ids=LC.shape_id)
def test_discrete_draws_stay_clear(shape):
    params, _flat, obs = LC.act_inputs(*shape)
    _want, share = _clear_share(params, obs)
    assert share >= W.MIN_CLEAR, share


def test_discrete_draws_stay_clear_grid_stride():
    shape = next(s for s in LC.GRID_STRIDE_SHAPES if not s[2])
    n = W.real_n(W.BIG, W.MI355X_CUS)
    assert n == 32 * 256 + 7
    params, _flat, obs = LC.act_inputs(*shape, n)
    want, share = _clear_share(params, obs)
    assert share >= W.MIN_CLEAR, share
    assert set(want.tolist()) == set(range(shape[1]))   # every action is drawn


def test_peaked_last_action_inputs_reach_the_second_block():
    params, _flat, obs = LC.peaked_last_inputs()
    want, share = _clear_share(params, obs)
    A = LC.CAT_DRAW_SHAPE[1]
    assert share >= W.MIN_CLEAR, share
    last = float((want == A - 1).mean())
    assert 0.25 <= last <= 0.75, last                      # the remainder branch
    assert ((want >= 16) & (want < A - 1)).sum() >= 5      # stops inside the second block
    assert (want < 16).sum() >= 5                          # and inside the first


def test_peaked_regime_inputs():
    params, _flat, obs, cont = LC.regime_sampler_inputs("peaked")
    assert not cont
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    out = P.forward(p64, obs, False, np.float64)["out"]
    gap = (out.max(1) - out.min(1)).max()
    assert abs(gap - LC.PEAKED_GAP) <= 1e-3 * LC.PEAKED_GAP, gap
    _want, share = _clear_share(params, obs)
    assert share >= W.MIN_CLEAR, share


@pytest.mark.parametrize("name", sorted(LC.SIGMA_LOG_STD))
def test_sigma_regime_inputs(name):
    params, _flat, _obs, cont = LC.regime_sampler_inputs(name)
    assert cont and params["actor_log_std"].shape[-1] == 17
    sigma = np.exp(params["actor_log_std"].astype(np.float64))
    want = {"sigma.05": 0.05, "sigma4.5": 4.5}[name]
    assert np.all(np.abs(sigma / want - 1) < 0.01)
