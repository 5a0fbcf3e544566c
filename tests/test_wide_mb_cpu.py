"""The cases of tests/test_gpu_wide_mb.py, examined without a GPU (tests/wide_mb_cases.py).

1. The case tables have the coverage the GPU module claims: all ten reachable
   wide_mb_kernel<H, CONT, NB1> on- and off-policy, every dW1 block count 1..8 and every width
   edge, every action count 1..16 under both heads.
2. With the compute-unit count taken as the MI355X's 256 and the tile as 32, the sizes of the
   groups D, E and F meet their stated conditions under a Python restatement of wide_grid and of
   launch_wide_pack's grid (the GPU module re-asserts D and E from dppo_fused_plan).
3. On the inputs of every case of the groups A to D and G, and of one shape each of E and F, the
   float32 oracle alone is within the GPU module's gradient bounds of the float64 oracle
   (wide_mb_cases.check_gradient): a correct float32 implementation meets them, so a kernel that
   misses them is wrong.  The old-policy records are the float32 oracle's here and the kernel's own
   on the GPU; the minibatch indices, parameters and rollouts are the same.
4. The bounds resolve what the guards and the slab count protect against: the float32 oracle's
   gradient with dW1's last column zero (every width of B), with dWo's last row zero (every
   action count of C) or without one of the capped grid's 256 slabs (E) is turned down.  The
   smallest such error is 2.7e-3 max|g| overall and 9.6e-2 of the tensor's scale, over 100 and
   900 times the bounds.

Largest float32-oracle errors (overall / max|g|, worst tensor / own scale): A 1.1e-6, 1.7e-5;
B 1.8e-7, 1.3e-6; C 7.4e-6, 2.8e-5; D 1.1e-6, 5.7e-6; E 9.5e-7, 3.4e-6; F 2.6e-6, 4.9e-6;
G 9.3e-8, 4.1e-7.  The largest per-tensor figures are the Gaussian head's actor_log_std and
output bias on-policy, where the policy term nearly cancels over the minibatch and the tensor's
scale is the 1e-3 max|g| floor.
"""
import numpy as np
import pytest

import gpu_helpers as G
import wide_mb_cases as C

CUS = C.MI355X_CUS


# ---------------------------------------------------------------------------------------------
# 1. coverage of the tables
# ---------------------------------------------------------------------------------------------
def test_all_ten_instantiations_on_and_off_policy():
    on = {C.instantiation_of(c[2:6]) for c in C.cases_of("A")}
    assert on == C.REACHABLE and len(on) == 10
    assert all(c[9] == C.SMALL_MB == 379 for c in C.cases_of("A"))
    off = {C.instantiation_of(s[1:5]) for s in G.OFFPOLICY_SHAPES if s[0] == "wide"}
    assert off == C.REACHABLE
    # the off-policy recipe is the same small one
    assert (G.OFFPOLICY_T, G.OFFPOLICY_M, G.OFFPOLICY_RAGGED) == \
        (C.SMALL_T, C.SMALL_M, C.SMALL_RAGGED)
    assert {s[5] for s in G.OFFPOLICY_SHAPES if s[0] == "wide"} == {C.SMALL_N}


def test_every_first_layer_block_count_and_edge():
    b = C.cases_of("B")
    assert {C.ncb1(c[3]) for c in b if c[2] == 128} == set(range(1, 9))
    assert {C.ncb1(c[3]) for c in b if c[2] == 64} == set(range(3, 9))
    for Hd in (128, 64):
        ds = {c[3] for c in b if c[2] == Hd}
        for edge in range(16 if Hd == 128 else 48, 129, 16):
            assert {edge - 1, edge, edge + 1} - {129} <= ds, (Hd, edge)
        assert (33 in ds) and ((32 in ds) == (Hd == 128))
    # the three roundings of D part ways: D8 < D16 (D = 8k + 1 .. 16k - 8) and D < D8 both occur
    assert any((c[3] + 7) // 8 * 8 < C.d16(c[3]) for c in b)
    assert any(c[3] < (c[3] + 7) // 8 * 8 for c in b)
    assert any(c[3] == C.d16(c[3]) for c in b)
    assert all((c[4], c[5], c[9]) == (4, False, 71) for c in b)


def test_every_action_count_under_both_heads():
    c = C.cases_of("C")
    for Hd, D in C.ACTION_BASES:
        for cont in (False, True):
            assert sorted(x[4] for x in c if x[2:4] == (Hd, D) and x[5] == cont) == \
                list(range(1, 17))
    assert len(c) == 64 and all(x[9] == 71 for x in c)


def test_seeds_are_distinct():
    seeds = [c[1] for c in C.small_cases()] + [C.capped_case(j, CUS)[1] for j in range(3)]
    assert len(set(seeds)) == len(seeds)


# ---------------------------------------------------------------------------------------------
# 2. the sizes meet their conditions
# ---------------------------------------------------------------------------------------------
def test_small_recipe_is_twelve_tiles_on_six_workgroups():
    assert C.wide_grid(C.SMALL_MB, CUS) == 6
    assert C.tiles_per_group(C.SMALL_MB, C.S, 6) == (2, 2) and C.SMALL_MB % C.S != 0
    assert C.wide_grid(71, CUS) == 1 and C.tiles_per_group(71, C.S, 1) == (3, 3)


def test_unequal_tile_counts():
    want = {71: (1, 3, 3), 135: (2, 2, 3), 199: (3, 2, 3)}
    for mb in C.UNEQUAL_MB:
        grid = C.wide_grid(mb, CUS)
        lo, hi = C.tiles_per_group(mb, C.S, grid)
        assert (grid, lo, hi) == want[mb]
        assert hi > lo or (grid == 1 and hi == 3)
        assert mb <= C.SMALL_T * C.SMALL_N // C.SMALL_M   # the handle's own grid is no smaller


def test_capped_grid_size():
    mb, Nn = C.capped_mb(CUS), C.capped_envs(CUS)
    B = C.CAPPED_T * Nn
    assert mb == 16423 and C.wide_grid(mb, CUS) == CUS
    assert C.tiles_per_group(mb, C.S, CUS) == (2, 3) and mb % C.S != 0
    # the smallest such: one tile fewer and the cap does not bind
    assert ((mb - C.S + C.S - 1) // C.S) // 2 <= CUS < ((mb + C.S - 1) // C.S) // 2
    # prepare() runs wide_eval_kernel over more than one tile per workgroup, the last partial
    assert mb < B <= mb + C.CAPPED_T and B % C.S != 0 and B > C.S * CUS
    # the grids taken afterwards on the same handle are smaller
    assert [C.wide_grid(m, CUS) for m in C.CAPPED_AFTER] == [1, 6]
    # slab_sum's batched loop (optim.hip: 16 waves, batches of 16 slabs, so wave w takes it when
    # w + 240 < G) runs in every wave at G = CUs, and in none at the sizes taken afterwards
    assert all(w + 15 * 16 < CUS for w in range(16))


def test_pack_second_pass_size():
    Hd, D, A, cont = C.PACK_SHAPE
    R = C.record_floats(D, A, cont)
    assert R == 148
    B = C.PACK_T * C.PACK_N
    pieces = B * (R // 4)
    threads = C.PACK_BLOCKS * C.PACK_THREADS
    assert (pieces + C.PACK_THREADS - 1) // C.PACK_THREADS > C.PACK_BLOCKS   # the cap binds
    assert threads < pieces < 2 * threads                                    # exactly two passes
    first = C.pack_first_second_pass_sample()
    assert first == 28339 and first * (R // 4) <= threads < (first + 1) * (R // 4)
    assert 300 <= B - first <= 600
    idx = C.pack_idx(600, B, first)
    assert idx.size == 2 * (B - first) and len(np.unique(idx)) == idx.size
    assert set(range(first, B)) <= set(idx.tolist())
    assert idx.size % C.S != 0
    # a batch one env smaller than the smallest with a second pass would not do
    assert 28340 // C.PACK_T < C.PACK_N


def test_ragged_learn_size():
    B = C.LEARN_T * C.LEARN_N
    assert B == 105 and B % C.LEARN_M == 0 and B // C.LEARN_M == 35
    assert B % C.S != 0 and (B // C.LEARN_M) % C.S != 0


# ---------------------------------------------------------------------------------------------
# 3. the float32 oracle meets the bounds
# ---------------------------------------------------------------------------------------------
def _oracles(case, idx=None):
    """Layout, inputs, records, minibatch and the float64 and float32 oracle results of a case"""
    _grp, seed, Hd, D, A, cont, T, Nn, M, mb = case
    L, names, params, _flat, host = C.inputs(seed, Hd, D, A, cont, T, Nn, M)
    rec = C.oracle_records(params, host, cont)
    if idx is None:
        idx = C.minibatch_idx(seed, T * Nn, mb)
    ref64 = C.oracle_gradient(params, host, cont, rec, idx, np.float64)
    ref32 = C.oracle_gradient(params, host, cont, rec, idx, np.float32)
    return L, names, params, host, rec, idx, ref64, ref32


def _float32_oracle_within_bounds(case, idx=None, production=False):
    L, names, _params, _host, _rec, idx, ref64, ref32 = _oracles(case, idx)
    assert idx.size == case[9]
    return C.check_gradient(L, names, G.flat_of(L, names, ref32[2]), C.loss_terms(ref32), ref64,
                            "float32 oracle " + C.case_id(case), ref32 if production else None)


_SMALL = C.small_cases() + C.learn_first_minibatch_cases()


@pytest.mark.parametrize("case", _SMALL, ids=[C.case_id(c) for c in _SMALL])
def test_float32_oracle_within_the_gradient_bounds(case):
    _float32_oracle_within_bounds(case)


def test_float32_oracle_within_the_gradient_bounds_capped_grid():
    case = C.capped_case(0, CUS)
    _float32_oracle_within_bounds(case, production=True)
    for mb in C.CAPPED_AFTER:
        _float32_oracle_within_bounds((*case[:9], mb))


def test_float32_oracle_within_the_gradient_bounds_pack_second_pass():
    B = C.PACK_T * C.PACK_N
    idx = C.pack_idx(600, B, C.pack_first_second_pass_sample())
    _float32_oracle_within_bounds(("F", 600, *C.PACK_SHAPE, C.PACK_T, C.PACK_N, 1, idx.size), idx)


# ---------------------------------------------------------------------------------------------
# 4. the bounds resolve the errors the guards and the slab count protect against
# ---------------------------------------------------------------------------------------------
def _rejected(L, names, grads, ref32, ref64, what):
    """The bounds turn down the float32 oracle's gradient with `grads` in place of its own."""
    try:
        C.check_gradient(L, names, G.flat_of(L, names, grads), C.loss_terms(ref32), ref64, what)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("case", C.cases_of("B"), ids=[C.case_id(c) for c in C.cases_of("B")])
def test_bounds_resolve_a_dropped_first_layer_column(case):
    """What the slab write's `k < D` guard would leave out if it stopped one column early: the
    float32 oracle's gradient with dW1's last column zero is outside the bounds at every width."""
    L, names, _p, _h, _r, _i, ref64, ref32 = _oracles(case)
    g = {n: np.array(v) for n, v in ref32[2].items()}
    g["base.0.weight"][:, -1] = 0
    assert _rejected(L, names, g, ref32, ref64, "dropped column " + C.case_id(case))


@pytest.mark.parametrize("case", C.cases_of("C"), ids=[C.case_id(c) for c in C.cases_of("C")])
def test_bounds_resolve_a_dropped_head_row(case):
    """What `4 g + v < A` would leave out if it stopped one action early: dWo's last row zero is
    outside the bounds at every action count (but one categorical action, whose logit gradient
    is zero)."""
    L, names, _p, _h, _r, _i, ref64, ref32 = _oracles(case)
    head = "actor_mean_head" if case[5] else "actor_head"
    g = {n: np.array(v) for n, v in ref32[2].items()}
    g[f"{head}.2.weight"][-1, :] = 0
    if case[4] == 1 and not case[5]:
        assert not np.any(ref64[2][f"{head}.2.weight"])
    else:
        assert _rejected(L, names, g, ref32, ref64, "dropped row " + C.case_id(case))


def test_bounds_resolve_a_skipped_slab():
    """What slab_reduce would give if it left out one of the CUs slabs of the capped grid: the
    float32 oracle's sum without workgroup 0's tiles (0, CUs and 2 CUs) is outside the bounds."""
    case = C.capped_case(0, CUS)
    L, names, params, host, rec, idx, ref64, ref32 = _oracles(case)
    tile = np.arange(idx.size) // C.S
    kept = idx[tile % CUS != 0]
    assert idx.size - kept.size == 3 * C.S
    _, _, part = C.oracle_gradient(params, host, case[5], rec, kept, np.float32)
    g = {n: np.asarray(v) * np.float32(kept.size / idx.size) for n, v in part.items()}
    assert _rejected(L, names, g, ref32, ref64, "skipped slab")
