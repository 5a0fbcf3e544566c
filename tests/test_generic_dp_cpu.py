"""What tests/test_gpu_generic_dp.py rests on, from NumPy and the oracle alone
(tests/generic_dp_cases.py): the generic learn on two ranks.

1. The share conditions.  In the global-minibatch cases (B3, B4) a rank holds 0 to 4 of a global
   minibatch's 4 samples; empty, single-sample and full shares occur on both ranks in both learns
   at the seeds used, and the union of the ranks' local minibatches is a permutation.
2. Re-association does not eat the bound: the two-rank restatement (generic_dp_cases.
   two_rank_learns) stays within a quarter of the 2e-5 parameter bound of the oracle's learn of
   the union batch, in every case and after both learns.
3. The bound rejects the mistakes the GPU module exists to catch.  Each, applied to the
   restatement, puts the parameters at least 4x the bound (8e-5) from the oracle:
     weight 1 / world where global minibatches need k / mbp   -- caught by B3 and B4
     local instead of global advantage statistics             -- caught by B1 and B3
     the empty-share step skipped on the empty rank           -- caught by B3 and B4
     -beta of d_log_std left unweighted by the share          -- caught by B2 and B4
"""
import functools

import numpy as np
import pytest

import generic_dp_cases as G
import wide_dp_cases as C


@functools.lru_cache(maxsize=None)
def _oracle(case):
    return G.oracle(case)


@pytest.mark.parametrize("case", ["B3", "B4"])
def test_global_cases_have_empty_single_and_full_shares_on_both_ranks(case):
    g = G.CASES[case]["geom"]
    mbp = g["T"] * g["Nl"] * G.WORLD // g["M"]
    assert mbp == 4
    for k, perms in enumerate(G.drawn_perms(case)):
        counts = C.share_counts(perms, g["Nl"], g["M"], world=G.WORLD)
        assert counts.shape == (G.E, g["M"], G.WORLD) and (counts.sum(-1) == mbp).all()
        for r in range(G.WORLD):
            hist = np.bincount(counts[:, :, r].ravel(), minlength=mbp + 1)
            print(case, "learn", k, "rank", r, "shares of 0..4 samples:", hist.tolist())
            assert hist[0] > 0 and hist[1] > 0 and hist[mbp] > 0, (case, k, r, hist)
            assert G.nonempty_minibatches(case, k, r) == G.E * g["M"] - hist[0]


def test_first_global_draw_is_the_recorded_one():
    """RandomState(3) drawing four permutations of 32: rank 0's 32 shares."""
    g = G.GLOBAL_GEOM
    counts = C.share_counts(G.drawn_perms("B3")[0], g["Nl"], g["M"], world=G.WORLD)
    assert np.bincount(counts[:, :, 0].ravel(), minlength=5).tolist() == [3, 7, 11, 9, 2]


@pytest.mark.parametrize("case", ["B1", "B2"])
def test_union_of_local_minibatches_is_a_permutation(case):
    g = G.CASES[case]["geom"]
    Bg = g["T"] * g["Nl"] * G.WORLD
    for drawn, perms in zip(G.drawn_perms(case), G.oracle_perms(case)):
        assert perms.shape == (G.E, Bg)
        for e in range(G.E):
            assert np.array_equal(np.sort(perms[e]), np.arange(Bg))
        # the ranks drew different orders
        assert not np.array_equal(drawn[0], drawn[1])
        assert G.nonempty_minibatches(case, 0, 0) == G.E * g["M"]


def test_seeds_differ_between_learns_and_ranks_as_documented():
    assert G.perm_seed("B1", 0, 0) == 3 and G.perm_seed("B1", 0, 1) == 4
    assert G.perm_seed("B1", 1, 0) == 13 and G.perm_seed("B1", 1, 1) == 14
    assert G.perm_seed("B3", 0, 0) == G.perm_seed("B3", 0, 1) == 3
    assert G.perm_seed("B3", 1, 0) == G.perm_seed("B3", 1, 1) == 13
    for case in G.CASES:
        _, _, hosts = G.case_setup(case)
        assert len(hosts) == G.LEARNS and not np.array_equal(hosts[0][0], hosts[1][0])
        assert G.CASES[case]["fused_loss"][0] != G.CASES[case]["fused_loss"][1]


@pytest.mark.parametrize("case", list(G.CASES))
def test_reassociation_stays_within_a_quarter_of_the_bound(case):
    names = G.case_setup(case)[0]
    got = G.two_rank_learns(case)
    for k, (ranks, (_, ref_params)) in enumerate(zip(got, _oracle(case))):
        for n in names:   # replicated clip + Adam on one summed gradient
            assert np.array_equal(ranks[0][n], ranks[1][n]), (case, k, n)
        d = G.distance(ranks[0], ref_params, names)
        print(f"{case} learn {k}: two-rank restatement vs oracle: max |dparam| {d:.3g}")
        assert d <= G.BOUND / 4, (case, k, d)


CATCHES = [("weight_1_over_world", "B3"), ("weight_1_over_world", "B4"),
           ("local_stats", "B1"), ("local_stats", "B3"),
           ("skip_empty", "B3"), ("skip_empty", "B4"),
           ("beta_unweighted", "B2"), ("beta_unweighted", "B4")]


@pytest.mark.parametrize("mistake,case", CATCHES)
def test_bound_rejects_the_mistake(mistake, case):
    names = G.case_setup(case)[0]
    got = G.two_rank_learns(case, mistake)
    _, ref_params = _oracle(case)[-1]
    d = max(G.distance(p, ref_params, names) for p in got[-1])
    print(f"{mistake} in {case}: max |dparam| from the oracle {d:.3g}")
    assert d >= 4 * G.BOUND, (mistake, case, d)


def test_every_mistake_has_a_catching_case():
    assert {m for m, _ in CATCHES} == set(G.MISTAKES)


def test_statistics_entry_points_refuse_null_and_small_n_before_any_launch():
    """No handle, no device: every call below must return before its first HIP call."""
    from diamond import _native as N
    lib = N.load()
    p = 0x1000                      # never dereferenced
    assert lib.dppo_adv_sums(None, p, None) == N.DPPO_EINVAL
    assert b"dppo_adv_sums" in lib.dppo_last_error()
    assert lib.dppo_adv_stats_from_sums(None, 8.0, p, None) == N.DPPO_EINVAL
    assert lib.dppo_adv_stats_from_sums(p, 8.0, None, None) == N.DPPO_EINVAL
    for n_total in (0.0, 0.5, -3.0, float("nan")):
        assert lib.dppo_adv_stats_from_sums(p, n_total, p, None) == N.DPPO_EINVAL, n_total
        assert b"dppo_adv_stats_from_sums" in lib.dppo_last_error()


# ---- A.1: the restated statistics scheme ------------------------------------------------------
@pytest.mark.parametrize("regime", G.STATS_REGIMES)
@pytest.mark.parametrize("T,Nl", G.STATS_SHAPES)
def test_restated_sums_finalise_to_the_oracle_statistics(T, Nl, regime):
    """The restated float32-shifted / float64-folded sums of the two shards, finalised as
    csrc/gae.hip mean_std_from does, meet the bounds the device is held to (1e-6 on the mean,
    2e-6 relative on the std): the yardstick's own error leaves them room."""
    from oracle import ppo_np as P
    r, te, tr, v, nv = G.stats_inputs(T, Nl, regime)
    adv = P.gae(r, te, tr, v, nv)
    s = q = 0.0
    for k in range(2):
        shard = adv[:, k * Nl:(k + 1) * Nl]
        rs, rq = G.restated_sums(shard)
        es, eq = G.exact_sums(shard)
        print(T, Nl, regime, "shard", k, "|restated - exact| sum", abs(rs - es), "of", abs(es),
              "sumsq", abs(rq - eq), "of", eq)
        s, q = s + rs, q + rq
    n = float(adv.size)
    mu = s / n
    mean, std = np.float32(mu), np.float32(np.sqrt(max((q - s * mu) / (n - 1.0), 0.0)))
    ref_mean, ref_std = P.adv_stats(adv)
    assert abs(mean - ref_mean) <= 1e-6 * max(1.0, abs(ref_mean))
    assert abs(std - ref_std) <= 2e-6 * ref_std
