"""Device shuffle (csrc/shuffle.hip) against NumPy, bit for bit: the Fisher-Yates resolution over
every scratch layout, partition size and solve path the host plan can choose, and the
global-minibatch member lists called directly.

Every comparison is np.array_equal.  Outputs and scratch sit between sentinel guards that must
come back untouched.  Cases, references and what each case is there for: tests/perm_cases.py
(asserted without a GPU by tests/test_perm_cpu.py).

DPPO_PERM_WALK is read at every call; DPPO_PERM_CSR and DPPO_PERM_EPOCHWISE once per process, so
those two run in a fresh child each (one at a time, each under its own time limit)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from diamond import _native as N

import perm_cases as C

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "diamond-ppo_amd")

GUARD = 1024            # int32 elements on either side
SENTINEL = -1515870811  # 0xA5A5A5A5: no valid sample index, bucket link or offset


def dev():
    return torch.device("cuda", 0)


def stream():
    return torch.cuda.current_stream().cuda_stream


def to_dev(a):
    return torch.from_numpy(np.array(a, np.int32)).to(dev())


def guarded(ints):
    """(whole allocation, its middle `ints` elements), all holding the sentinel."""
    buf = torch.full((GUARD + ints + GUARD,), SENTINEL, dtype=torch.int32, device=dev())
    return buf, buf[GUARD:GUARD + ints]


def guards_intact(buf, ints):
    edge = torch.cat([buf[:GUARD], buf[GUARD + ints:]])
    return edge.numel() == 2 * GUARD and bool((edge == SENTINEL).all())


def walk_is(walk):
    assert os.environ.get("DPPO_PERM_WALK") == walk


def run_resolve(tg, ref, n, count, ints, what):
    """dppo_perm_resolve_ex(tg) in `ints` of scratch == ref, touching nothing outside
    out[count * n] and scratch[ints]."""
    assert tg.shape == ref.shape == (count * n,) and ints >= 3 * count * n
    td = to_dev(tg)
    obuf, out = guarded(count * n)
    sbuf, scratch = guarded(ints)
    N.perm_resolve_ex(td.data_ptr(), out.data_ptr(), n, count, scratch.data_ptr(), ints, stream())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    print(f"PERM-CHECK {what}: n {n} count {count} scratch {ints} "
          f"mismatches {int((got != ref).sum())}")
    assert guards_intact(obuf, count * n), "wrote outside perms[count * n]"
    assert guards_intact(sbuf, ints), "wrote outside scratch[scratch_ints]"
    for c in range(count):
        row = got[c * n:(c + 1) * n]
        assert row.min() >= 0 and row.max() < n
        assert (np.bincount(row, minlength=n) == 1).all(), f"row {c} is no permutation"
    assert np.array_equal(got, ref)


def check_resolution(n, count, walk, kind):
    walk_is(walk)
    ints = C.scratch_ints(n, count, kind)
    run_resolve(C.random_targets(n, count), C.random_reference(n, count), n, count, ints,
                f"random walk={walk} {kind}")


def check_adversarial(name, n, walk, kind):
    walk_is(walk)
    count = C.ADVERSARIAL_COUNT
    tg = np.concatenate([C.adversarial_targets(name, n)] * count)
    ref = np.concatenate([C.adversarial_reference(name, n)] * count)
    run_resolve(tg, ref, n, count, C.scratch_ints(n, count, kind), f"{name} walk={walk} {kind}")


def check_lists(k, rank, walk):
    """dppo_global_minibatch_lists on a handle of its own (no communicator), twice."""
    walk_is(walk)
    d = C.list_dims(C.LISTS[k])
    E, B, M = d["E"], d["B"], d["M"]
    ref_local, ref_seg = C.list_reference(k, rank)
    h = N.Handle(0, N.Dims(d["T"], d["Nl"], 4, 2, 0, 64, E, M, d["world"], rank, 1))
    try:
        td = to_dev(C.list_inputs(k)[0])
        got = []
        for _ in range(2):
            lbuf, local = guarded(E * B)
            sbuf, seg = guarded(E * (M + 1))
            N.check(h.lib.dppo_global_minibatch_lists(h.h, td.data_ptr(), local.data_ptr(),
                                                      seg.data_ptr(), stream()),
                    "dppo_global_minibatch_lists")
            torch.cuda.synchronize()
            assert guards_intact(lbuf, E * B), "wrote outside local[E][B]"
            assert guards_intact(sbuf, E * (M + 1)), "wrote outside seg[E][M + 1]"
            got.append((local.cpu().numpy().reshape(E, B), seg.cpu().numpy().reshape(E, M + 1)))
    finally:
        h.close()
    print(f"PERM-CHECK lists walk={walk}: Bg {d['Bg']} Ng {d['Ng']} M {M} E {E} rank {rank} "
          f"seg[0] {got[0][1][0][:6]} reference {ref_seg[0][:6]} "
          f"mismatches {int((got[0][0] != ref_local).sum())}")
    for local, seg in got:
        assert np.array_equal(seg, ref_seg)
        assert np.array_equal(local, ref_local)


# ---------------------------------------------------------------------------------------------
# 1. resolution: geometry x walk mode x scratch size
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["0", "1"])
@pytest.mark.parametrize("n,count,kind", C.resolve_params(C.RESOLVE))
def test_resolution_geometry_sweep(monkeypatch, n, count, kind, walk):
    """Random targets over the plan's edges (tiny n, the public-scratch fit, 1 -> 2 partitions and
    chunks, the scans' unrolled and multi-entry forms, 4,096 partitions) on the public scratch,
    the packed one and one int less (the two-array layout again, or the lists)."""
    monkeypatch.setenv("DPPO_PERM_WALK", walk)
    if kind != "public":
        assert C.packed_ints(n, count) == N.perm_resolve_scratch(n, count)
    check_resolution(n, count, walk, kind)


@pytest.mark.parametrize("walk", ["0", "1"])
@pytest.mark.parametrize("n,count,kind", C.resolve_params(C.RESOLVE_BIG, ("public", "packed")))
def test_resolution_above_8m(monkeypatch, n, count, kind, walk):
    """n > 8,388,608: partitions of 4,096 positions (about 280 of 2,049 beyond the LDS capacity
    of the fused fill at n = 8,388,609; exactly 4,096 partitions at 16,777,216), and one more
    sample: the linked lists, whose passes go grid-stride."""
    monkeypatch.setenv("DPPO_PERM_WALK", walk)
    if kind != "public":
        assert C.packed_ints(n, count) == N.perm_resolve_scratch(n, count)
    check_resolution(n, count, walk, kind)


# ---------------------------------------------------------------------------------------------
# 2. adversarial but valid targets
# ---------------------------------------------------------------------------------------------
@pytest.mark.timeout(120)
@pytest.mark.parametrize("walk", ["0", "1"])
@pytest.mark.parametrize("kind", ["public", "packed"])
@pytest.mark.parametrize("n", C.ADVERSARIAL_N)
@pytest.mark.parametrize("name", C.ADVERSARIAL_KINDS)
def test_resolution_on_adversarial_targets(monkeypatch, name, n, kind, walk):
    """The sequential loop's permutation for all-zero, identity, shifted, halved and mod-64
    targets: buckets of up to n - 1 steps, heap-sorted in LDS (n = 12,001 packed) or in memory,
    chains of n links, and the walk over them."""
    monkeypatch.setenv("DPPO_PERM_WALK", walk)
    check_adversarial(name, n, walk, kind)


# ---------------------------------------------------------------------------------------------
# 3. global-minibatch member lists, direct
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", ["1", "0"])
@pytest.mark.parametrize("k,rank", C.list_params())
def test_global_minibatch_lists_match_numpy(monkeypatch, k, rank, walk):
    """One rank's members of every global minibatch, from device swap targets: by the walk of the
    rank's own values and the marks selection (DPPO_PERM_WALK=1, the default) and by the whole
    resolution and the shard selection (=0), against the lists cut from NumPy's permutations."""
    monkeypatch.setenv("DPPO_PERM_WALK", walk)
    check_lists(k, rank, walk)


# ---------------------------------------------------------------------------------------------
# 4. the switches read once per process
# ---------------------------------------------------------------------------------------------
_CHILD = r"""
import os
import sys
sys.path[:0] = {paths!r}
import perm_cases as C
import test_gpu_perm as G
from diamond import _native as N
mode = {mode!r}
if mode == "csr0":    # no partitioned sort: no packed size either
    assert N.perm_resolve_scratch(1000, 4) == 3 * 4 * 1000
    sizes = [(1000, 4), (65539, 2), (2100001, 1)]
else:
    assert N.perm_resolve_scratch(1000, 4) == C.packed_ints(1000, 4)
    sizes = [(1000, 4), (65539, 2), (524288, 4)]
for walk in ("0", "1"):
    os.environ["DPPO_PERM_WALK"] = walk
    for n, count in sizes:
        G.check_resolution(n, count, walk, "public")
    if mode == "csr0":
        for name in ("zeros", "mod64"):
            G.check_adversarial(name, C.ADVERSARIAL_N[0], walk, "public")
if mode == "csr0":
    os.environ["DPPO_PERM_WALK"] = "1"
    for k in (2, 4, 5, 6):
        for rank in C.LISTS[k][5]:
            G.check_lists(k, rank, "1")
print("PERM-CHILD-OK", mode, flush=True)
"""


def run_child(mode, env, checks):
    paths = [ROOT, PKG, os.path.join(ROOT, "tests")]
    r = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths, mode=mode)],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=240)
    print(r.stdout)
    assert r.returncode == 0 and f"PERM-CHILD-OK {mode}" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("PERM-CHECK") == checks


@pytest.mark.timeout(300)
def test_linked_lists_only_process():
    """DPPO_PERM_CSR=0: every resolution and list build through the linked lists -- sizes the
    partitioned sort otherwise takes (2,100,001: grid-stride), heavy buckets, and the marks walk
    over lists at Bg = 105, 16,400, 4,198,400 and 4,915,712."""
    ks = (2, 4, 5, 6)
    assert [C.list_dims(C.LISTS[k])["Bg"] for k in ks] == [105, 16400, 4198400, 4915712]
    lists = sum(len(C.LISTS[k][5]) for k in ks)
    run_child("csr0", {"DPPO_PERM_CSR": "0"}, 2 * (3 + 2) + lists)


@pytest.mark.timeout(300)
def test_epochwise_process():
    """DPPO_PERM_EPOCHWISE=1: one epoch at a time through launch_perm_resolve_one, both solve
    paths (count 1 would take the ordinary path: every size here has more epochs)."""
    run_child("epochwise", {"DPPO_PERM_EPOCHWISE": "1"}, 2 * 3)
