"""CPU half of tests/test_gpu_perm.py: the plan restatement against the C++ it restates, every
geometry class of the case tables asserted through it (so a case that drifts off its edge fails
here, without a GPU), what the real targets make of the LDS capacity and the heap-sort threshold,
and the list reference against a sample-by-sample loop."""
import numpy as np
import pytest

from diamond import _native as N

import perm_cases as C

ALL_RESOLVE = C.RESOLVE + C.RESOLVE_BIG


def pub(n, c):
    return C.plan(n, c, C.public_ints(n, c))


def pk(n, c):
    return C.plan(n, c, C.INF)


def test_plan_restates_the_native_scratch_size():
    """max(plan(n, count, inf).end, 3 * count * n) == dppo_perm_resolve_scratch(n, count) over the
    case tables and a dense sweep of small n (where the 256-B alignment of the regions decides)."""
    cases = [(n, c) for n, c, _ in ALL_RESOLVE]
    cases += [(n, C.ADVERSARIAL_COUNT) for n in C.ADVERSARIAL_N]
    cases += [(C.list_dims(case)["Bg"], case[4]) for case in C.LISTS]
    cases += [(n, c) for n in range(2, 3001) for c in range(1, 6)]
    for n, c in cases:
        assert C.packed_ints(n, c) == N.perm_resolve_scratch(n, c), (n, c)
    assert C.packed_ints(1, 1) == N.perm_resolve_scratch(1, 1) == 3
    # every packed plan is the fused form: from packed - 1 down it is another layout
    for n, c in cases[:len(ALL_RESOLVE)]:
        p = pk(n, c)
        if p:
            assert p["pack"] and p["end"] > 3 * c * n
            q = C.plan(n, c, p["end"] - 1)
            assert q is None or not q["pack"]


def test_plan_table():
    """The plan of the documented (n, count, scratch) rows, recomputed."""
    assert pub(17, 2) is None
    p = pub(1000, 4)
    assert p and not p["pack"] and p["nparts"] == 1 and p["end"] == 10240
    assert pub(363, 1) and not pub(363, 1)["pack"]
    assert pub(533, 1) is None
    p = pub(8388608, 1)
    assert p and not p["pack"] and (p["logp"], p["nparts"]) == (11, 4096)
    p = pub(8388609, 1)
    assert p and not p["pack"] and (p["logp"], p["nparts"], p["bpe"]) == (12, 2049, 257)
    p = pub(16777216, 1)
    assert p and not p["pack"] and (p["logp"], p["nparts"]) == (12, 4096)
    assert pub(16777217, 1) is None and pk(16777217, 1) is None
    assert pk(8388608, 1)["cap"] == 12272 and pk(8388609, 1)["cap"] == 8176


def test_public_scratch_fit_edges_are_cases():
    """Within the public 3 * n the two-array layout first fits at n = 363 and, the regions being
    256-B aligned, last fails at n = 533: both sides of both edges are resolution cases."""
    fits = {n: pub(n, 1) is not None for n in range(2, 3001)}
    first = min(n for n, f in fits.items() if f)
    last_miss = max(n for n, f in fits.items() if not f)
    assert (first, last_miss) == (363, 533)
    assert any(not fits[n] for n in range(first, last_miss))      # non-monotonic in between
    assert any(fits[n] for n in range(first, last_miss))
    have = {(n, c) for n, c, tag in C.RESOLVE if tag == "fit-edge"}
    assert have == {(first - 1, 1), (first, 1), (last_miss, 1), (last_miss + 1, 1)}


def test_every_geometry_class_has_a_case():
    cases = [(n, c) for n, c, _ in ALL_RESOLVE]
    P = {nc: pk(*nc) for nc in cases}
    U = {nc: pub(*nc) for nc in cases}
    ok = [nc for nc in cases if P[nc]]

    def some(pred, plans=P):
        return [nc for nc in cases if plans[nc] and pred(plans[nc], *nc)]

    # the linked lists: tiny n on the public scratch, n beyond 4096 partitions of 4096 on any
    assert [nc for nc in cases if nc[0] >= 2 and nc[0] < 363 and U[nc] is None]
    big = [nc for nc in cases if nc[0] > (C.MAX_PARTS << C.MAX_LOGP)]
    assert big and all(P[nc] is None and U[nc] is None for nc in big)
    # ... whose passes go grid-stride (a second round per thread)
    assert any(n * c > C.FY_GRID for n, c in big)
    # n = 1: nothing to resolve, no plan
    assert (1, 1) in cases and P[(1, 1)] is None
    # packed layout with one partition of 2,048 positions at tiny n
    tiny = some(lambda p, n, c: n <= 17 and p["pack"] and p["nparts"] == 1 and p["logp"] == 11)
    assert {n for n, _ in tiny} >= {2, 3, 17}
    # packed - 1: the two-array layout wherever it fits at all
    for n, c in ok:
        q = C.plan(n, c, C.packed_ints(n, c) - 1)
        assert (q is not None and not q["pack"]) or n < 363, (n, c)
    # one partition -> two, at count 1 and above
    assert P[(2047, 1)]["nparts"] == P[(2048, 1)]["nparts"] == 1 and P[(2049, 3)]["nparts"] == 2
    assert P[(2049, 3)]["np"] == 6
    # one chunk per epoch -> two
    assert P[(32768, 1)]["bpe"] == 1 and P[(32769, 2)]["bpe"] == 2
    # csr_colscan_kernel: more than one round of 8 chunks, the last one partial
    assert some(lambda p, n, c: p["bpe"] > 8 and p["bpe"] % 8)
    # csr_count / csr_scatter: more partitions than threads
    assert some(lambda p, n, c: p["nparts"] > 256)
    # csr_basescan_kernel: exactly one entry per thread, and more than one (ragged: np no multiple
    # of the per-thread count times 1024)
    assert some(lambda p, n, c: p["np"] == 1024 and c > 1)
    assert some(lambda p, n, c: p["np"] > 1024 and p["np"] % 1024)
    # partitions of 2,048 up to exactly 4,096 of them; of 4,096 from the next n on, up to 4,096
    assert some(lambda p, n, c: p["logp"] == 11 and p["nparts"] == C.MAX_PARTS)
    assert some(lambda p, n, c: p["logp"] == 12 and p["nparts"] == C.MAX_PARTS // 2 + 1)
    assert some(lambda p, n, c: p["logp"] == 12 and p["nparts"] == C.MAX_PARTS)
    # a last partition / chunk of one position, and full ones
    assert some(lambda p, n, c: n % (1 << p["logp"]) == 1) and some(lambda p, n, c: n % C.CHUNK == 1)
    assert some(lambda p, n, c: n % (1 << p["logp"]) == 0 and n % C.CHUNK == 0)
    # both layouts at both partition sizes: the public scratch gives the two arrays
    for logp in (11, 12):
        assert some(lambda p, n, c: p["logp"] == logp and not p["pack"], U)
        assert some(lambda p, n, c: p["logp"] == logp and p["pack"])
    # the big cases run on the public and the packed scratch only, the others on all three
    assert {k for n, c, k in C.resolve_params(C.RESOLVE) if n > 1} == set(C.SCRATCH_KINDS)
    assert [k for n, c, k in C.resolve_params(C.RESOLVE) if n == 1] == ["public"]
    assert all(n > 8388608 for n, _, _ in C.RESOLVE_BIG)
    assert all(n <= 8388608 for n, _, _ in C.RESOLVE)


def test_random_targets_at_4096_position_partitions_split_at_the_lds_capacity():
    """(8388609, 1): partitions of 4,096 positions, cap 8,176 -- the low partitions (large buckets)
    sort in memory, the others in LDS, and in numbers that make both branches count."""
    n, c = 8388609, 1
    p = pk(n, c)
    sz = C.partition_sizes(C.random_targets(n, c), p["logp"])
    assert len(sz) == p["nparts"] and sz.sum() == n - 1
    over = int((sz > p["cap"]).sum())
    assert 200 < over < 400 and len(sz) - over > 1000, over
    # at 2,048-position partitions hardly any does (why the smaller cases do not cover it)
    q = pk(524288, 4)
    tg = C.random_targets(524288, 4)
    for e in range(4):
        assert (C.partition_sizes(tg[e * 524288:(e + 1) * 524288], q["logp"]) > q["cap"]).sum() <= 2


def test_random_targets_never_reach_the_heap_sort():
    for n, c, _ in ALL_RESOLVE:
        tg = C.random_targets(n, c)
        for e in range(c):
            assert C.bucket_sizes(tg[e * n:(e + 1) * n]).max(initial=0) <= C.HEAP_ABOVE, (n, c)


def test_mod64_targets_heap_sort_in_lds_and_in_memory():
    """mod64 at n = 12,001: one partition holds all 12,000 steps, within cap 12,272, in buckets of
    ~187 > 32: csr_bucket_links heap-sorts in LDS.  At n = 20,011 the partition exceeds cap."""
    small, large = C.ADVERSARIAL_N
    for n, in_lds in ((small, True), (large, False)):
        p = pk(n, C.ADVERSARIAL_COUNT)
        assert p["pack"] and p["logp"] == 11
        j = C.adversarial_targets("mod64", n)
        sz, bk = C.partition_sizes(j, p["logp"]), C.bucket_sizes(j)
        assert sz[0] == n - 1 and (sz[1:] == 0).all()
        assert (sz[0] <= p["cap"]) == in_lds
        assert bk[:64].min() > C.HEAP_ABOVE and bk.max() >= (n - 1) // 64
    # zeros (one bucket of n - 1 steps) splits the same way
    assert small - 1 <= pk(small, 2)["cap"] < large - 1


@pytest.mark.parametrize("kind", C.ADVERSARIAL_KINDS)
def test_adversarial_targets_are_valid_and_give_permutations(kind):
    for n in (1, 2, 65, 1000):
        j = C.adversarial_targets(kind, n)
        assert j[0] == 0 and (j <= np.arange(n)).all() and (j >= 0).all()
        assert np.array_equal(np.sort(C.fisher_yates(j)), np.arange(n))
    # the loop is numpy's: replaying real targets gives RandomState.permutation
    assert np.array_equal(C.fisher_yates(C.random_targets(1000, 4)[:1000]),
                          C.random_reference(1000, 4)[:1000])


def test_list_case_geometry():
    d = [C.list_dims(case) for case in C.LISTS]
    assert [x["Bg"] for x in d] == [64, 6, 105, 16384, 16400, 4198400, 4915712]
    assert [x["chunks"] for x in d] == [1, 1, 1, 1, 2, 257, 301]
    # shard_write_kernel adds the counts of the chunks before its own, 256 per round: the last
    # workgroup of 257 chunks still adds one per thread; a second round needs a chunk index above
    # 256, and only counts that are not zero there can show a wrong sum
    assert d[5]["chunks"] - 1 == 256 and d[6]["chunks"] - 1 > 256
    rank, Nl = C.LISTS[6][5][0], d[6]["Nl"]
    late = C.list_inputs(6)[1][0, 256 * C.SEL_CHUNK:(d[6]["chunks"] - 1) * C.SEL_CHUNK]
    env = late.astype(np.int64) % d[6]["Ng"]
    assert ((env >= rank * Nl) & (env < (rank + 1) * Nl)).sum() > 1000
    assert d[6]["Bg"] % C.SEL_CHUNK == 512 and d[6]["mbg"] % 256
    assert all(x["Bg"] % x["M"] == 0 and x["B"] % x["M"] == 0 for x in d)
    assert d[1]["M"] == 1
    assert d[2]["Ng"] == 21 and d[2]["mbg"] == 15
    assert d[3]["Bg"] == C.SEL_CHUNK and d[3]["Nl"] == 1
    assert d[4]["Bg"] - C.SEL_CHUNK == 16 and d[4]["mbg"] == 2050 and d[4]["mbg"] % 256
    assert d[5]["chunks"] > 256 and d[5]["Bg"] % C.SEL_CHUNK         # ragged last chunk too
    assert d[5]["mbg"] % 256 == 0 and d[5]["mbg"] % C.SEL_CHUNK      # seg inside a chunk
    assert any(x["Ng"] & (x["Ng"] - 1) for x in d) and any(not x["Ng"] & (x["Ng"] - 1) for x in d)
    for case, x in zip(C.LISTS, d):
        assert all(0 <= r < x["world"] for r in case[5])
        # every handle's scratch holds the packed layout (the production path of the walk)
        p = C.plan(x["Bg"], x["E"], C.packed_ints(x["Bg"], x["E"]))
        assert p and p["pack"]
    # Bg = 64 over 8 ranks and 8 minibatches of 8: some rank misses some minibatch
    _, seg = C.list_reference(0, 0)
    _, seg7 = C.list_reference(0, 7)
    assert (np.diff(seg, axis=1) == 0).any() or (np.diff(seg7, axis=1) == 0).any()


@pytest.mark.parametrize("k", [0, 1, 2])
def test_global_lists_matches_the_sample_loop(k):
    T, Nl, world, M, E, _ = C.LISTS[k]
    perms = C.list_inputs(k)[1]
    for rank in range(world):
        a = C.global_lists(perms, T, Nl, world, rank, M)
        b = C.global_lists_loop(perms, T, Nl, world, rank, M)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("k,rank", C.list_params())
def test_global_lists_shape_properties(k, rank):
    d = C.list_dims(C.LISTS[k])
    tg, perms = C.list_inputs(k)
    assert perms.shape == (d["E"], d["Bg"]) and tg.shape == (d["E"] * d["Bg"],)
    local, seg = C.list_reference(k, rank)
    assert local.shape == (d["E"], d["B"]) and seg.shape == (d["E"], d["M"] + 1)
    for e in range(d["E"]):
        assert np.array_equal(np.sort(local[e]), np.arange(d["B"]))
    assert (seg[:, 0] == 0).all() and (seg[:, -1] == d["B"]).all()
    assert (np.diff(seg, axis=1) >= 0).all()


def test_all_ranks_lists_partition_the_permutation():
    """Over all ranks the members of each global minibatch are exactly that minibatch."""
    k = 2
    T, Nl, world, M, E, _ = C.LISTS[k]
    d = C.list_dims(C.LISTS[k])
    perms = C.list_inputs(k)[1]
    for e in range(E):
        for j in range(M):
            got = []
            for rank in range(world):
                local, seg = C.global_lists(perms, T, Nl, world, rank, M)
                l = local[e, seg[e, j]:seg[e, j + 1]].astype(np.int64)
                got += list((l // Nl) * d["Ng"] + l % Nl + rank * Nl)
            assert sorted(got) == sorted(perms[e, j * d["mbg"]:(j + 1) * d["mbg"]])
