"""CPU side of the wide kernel family on several ranks (tests/test_gpu_wide_dp.py is the GPU
side): the opt-in through the predicate, the configs and the ABI struct; the conditions the GPU
module's case table rests on, asserted from NumPy alone so that its tests cannot pass vacuously;
and the ranks' agreement on the transport when a layout is past the peer exchange's capacity
(the pattern of tests/test_comm_agreement_cpu.py: a world-2 gloo group and a stand-in handle whose
peer_export raises as _native does)."""
import dataclasses
import os
import socket
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import diamond
from diamond import _native as N
from diamond.engine import fused_shape_class

import wide_dp_cases as C


# ---- 1: the predicate, the configs, the struct
def test_predicate_is_opt_in(monkeypatch):
    monkeypatch.delenv("DPPO_WIDE", raising=False)
    for Hd, D in ((128, 8), (64, 33)):
        assert fused_shape_class(Hd, D, 4, 2, wide_ranks=True) == "wide"
        assert fused_shape_class(Hd, D, 4, 8, True) == "wide"
        assert fused_shape_class(Hd, D, 4, 2) is None
        assert fused_shape_class(Hd, D, 4, 2, wide_ranks=False) is None
        assert fused_shape_class(Hd, D, 4, 1) == "wide"
        assert fused_shape_class(Hd, D, 4, 1, wide_ranks=True) == "wide"
    # the tuned class does not depend on it
    for wr in (False, True):
        assert fused_shape_class(64, 4, 2, 2, wide_ranks=wr) == "tuned"
        assert fused_shape_class(64, 32, 16, 8, wide_ranks=wr) == "tuned"
    # what no class serves stays unserved
    assert fused_shape_class(128, 129, 4, 2, wide_ranks=True) is None
    assert fused_shape_class(64, 129, 4, 2, wide_ranks=True) is None
    assert fused_shape_class(256, 8, 4, 2, wide_ranks=True) is None
    assert fused_shape_class(128, 8, 17, 2, wide_ranks=True) is None
    assert fused_shape_class(64, 40, 17, 2, wide_ranks=True) is None


def test_kill_switch_wins_over_the_flag(monkeypatch):
    monkeypatch.setenv("DPPO_WIDE", "0")
    for wr in (False, True):
        assert fused_shape_class(128, 8, 4, 2, wide_ranks=wr) is None
        assert fused_shape_class(64, 33, 4, 2, wide_ranks=wr) is None
        assert fused_shape_class(128, 8, 4, 1, wide_ranks=wr) is None
        assert fused_shape_class(64, 4, 2, 2, wide_ranks=wr) == "tuned"


def test_config_field_is_additive_and_off():
    n_ref = 21  # the reference's fields, pinned by test_native_cpu.test_configs_are_field_compatible
    for cls in (diamond.PPOConfig, diamond.ContinuousPPOConfig):
        names = [f.name for f in dataclasses.fields(cls)]
        assert names[n_ref - 1] == "verbose"
        assert names.index("wide_data_parallel") >= n_ref
        assert names.index("wide_data_parallel") > names.index("gae_bitexact")
        assert cls().wide_data_parallel is False
        assert cls(wide_data_parallel=True).wide_data_parallel is True


def test_dims_field_is_trailing_and_defaults_to_off():
    assert N.Dims._fields_[-1][0] == "wide_ranks"
    assert N.Dims._fields_[-2][0] == "global_minibatches"
    d = N.Dims(4, 32, 8, 4, 0, 128, 1, 1, 2, 0)       # the 10- and 11-argument forms of the tests
    assert (d.world_size, d.global_minibatches, d.wide_ranks) == (2, 0, 0)
    d = N.Dims(4, 32, 8, 4, 0, 128, 1, 1, 2, 0, 1)
    assert (d.global_minibatches, d.wide_ranks) == (1, 0)
    d = N.Dims(4, 32, 8, 4, 0, 128, 1, 1, 2, 0, 1, 1)
    assert (d.global_minibatches, d.wide_ranks) == (1, 1)
    assert C.dims(128, 8, 4, False, 4, 32, 1, 2, 0, 1, 1).wide_ranks == 1


def test_layout_query_validates_the_flag():
    N.param_layout(C.dims(128, 8, 4, False, 4, 32, 1, 2, 0, 0, 1))
    with pytest.raises(ValueError, match="wide_ranks"):
        N.param_layout(C.dims(128, 8, 4, False, 4, 32, 1, 2, 0, 0, 2))
    with pytest.raises(ValueError, match="wide_ranks"):
        N.param_layout(C.dims(128, 8, 4, False, 4, 32, 1, 2, 0, 0, -1))


# ---- 2: what the GPU module's cases rest on
def test_uneven_case_has_empty_and_multi_sample_shares():
    g = C.UNEVEN
    Bg = g["T"] * g["Nl"] * C.WORLD
    for perms_g in C.global_perms(C.UNEVEN_PERM_SEED, Bg, 2):
        counts = C.share_counts(perms_g, g["Nl"], g["M"])
        assert counts.shape == (C.E, g["M"], C.WORLD)
        assert (counts.sum(axis=2) == Bg // g["M"]).all()
        assert (counts == 0).any() and counts.max() >= 3
    # one workgroup: an empty share is a launch whose only workgroup runs no tile
    assert C.handle_grid(g["T"], g["Nl"], g["M"], C.WORLD, True) == 1


def test_straddling_case_has_two_and_three_tile_shares_on_a_grid_of_eight():
    g = C.STRADDLE
    Bg = g["T"] * g["Nl"] * C.WORLD
    perms_g, = C.global_perms(C.STRADDLE_PERM_SEED, Bg)
    counts = C.share_counts(perms_g, g["Nl"], g["M"])
    assert Bg // g["M"] == 512
    assert (counts <= 2 * C.S).any() and (counts > 2 * C.S).any()
    tiles = (counts + C.S - 1) // C.S
    assert set(np.unique(tiles)) == {2, 3}
    G = C.handle_grid(g["T"], g["Nl"], g["M"], C.WORLD, True)
    assert G == 8                       # wide_grid of a whole global minibatch: 16 tiles / 2
    assert tiles.max() < G              # so every launch has workgroups that run no tile


def test_local_cases_tile_geometry():
    g = C.RAGGED
    m = g["T"] * g["Nl"] // g["M"]
    assert m == 35 and g["T"] * g["Nl"] % g["M"] == 0
    assert C.wide_grid(m, C.MI355X_CUS) == 1 and C.tiles_per_group(m, C.S, 1) == (2, 2)
    assert m % C.S == 3
    g = C.MULTI
    m = g["T"] * g["Nl"] // g["M"]
    G = C.wide_grid(m, C.MI355X_CUS)
    assert (m, G) == (268, 4) and g["T"] * g["Nl"] % g["M"] == 0
    assert C.tiles_per_group(m, C.S, G) == (2, 3)
    assert 0 < m % C.S < C.S            # a partial last tile
    assert C.handle_grid(g["T"], g["Nl"], g["M"], C.WORLD, False) == G


def test_shapes_cover_both_widths_heads_and_every_nb1():
    from wide_mb_cases import nb1
    assert {(Hd, nb1(D)) for Hd, D, _, _ in C.SHAPES} == {(128, 2), (64, 8), (64, 4)}
    assert {cont for *_, cont in C.SHAPES} == {False, True}
    assert {nb1(D) for _, D, _, _ in C.SHAPES + [C.OVER_CAPACITY]} == {2, 4, 8}


def test_exchange_capacity_of_the_shapes():
    for Hd, D, A, cont in C.SHAPES + [(Hd, D, A, False) for Hd, D, A in C.AGENT_SHAPES]:
        L = N.param_layout(C.dims(Hd, D, A, cont, 4, 32, 1))
        assert L.total + 8 <= C.PEER_CAPACITY, (Hd, D, A, L.total)
    Hd, D, A, cont = C.OVER_CAPACITY
    L = N.param_layout(C.dims(Hd, D, A, cont, 4, 32, 1))
    assert L.total + 8 > C.PEER_CAPACITY, L.total
    assert fused_shape_class(Hd, D, A, 2, wide_ranks=True) == "wide"


# ---- 3: transport agreement on an over-capacity layout
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class _OverCapacityHandle:
    """peer_export as _native.Handle's on a layout past the exchange: check() maps
    DPPO_EUNSUPPORTED onto NotImplementedError."""

    def __init__(self, refuses):
        self.refuses = refuses
        self.calls = []

    def comm_init(self, nranks, rank, uid):
        self.calls.append("comm_init")

    def peer_export(self):
        self.calls.append("peer_export")
        if self.refuses:
            raise NotImplementedError("dppo_peer_export: peer exchange: 68392 parameters exceed "
                                      "the exchange's 65536 elements")
        return bytes(64)

    def peer_open(self, nranks, rank, handles, shared_device=False):
        self.calls.append("peer_open")
        return ""

    def peer_selftest(self, stream):
        self.calls.append("peer_selftest")
        return ""

    def peer_close(self):
        self.calls.append("peer_close")


class _FakeFlat:
    def __init__(self):
        self.flat = torch.zeros(8)


class _CurrentStream:
    cuda_stream = 0


def _worker(rank, world, port, mode, refusing, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), DPPO_COMM=mode)
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "diamond-ppo_amd"))
    from diamond import engine
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        engine.N.comm_unique_id = lambda: bytes(128)
        torch.cuda.current_stream = lambda device=None: _CurrentStream()
        L = object.__new__(engine.NativeLearner)
        L.world, L.rank, L.device = world, rank, torch.device("cpu")
        L.handle = _OverCapacityHandle(rank in refusing)
        L.flat = _FakeFlat()
        L._gpu_identity = lambda: ("host", 0, rank, 0)
        err = ""
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            try:
                L._init_comm()
            except RuntimeError as e:
                err = str(e)
        q.put((rank, getattr(L, "peer", None), L.handle.calls, err,
               [str(x.message) for x in w]))
        # a collective after _init_comm: a rank that left it early or late hangs here (the parent
        # process sees it as a rank that does not exit)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def _run(mode, check, refusing=(0, 1)):
    """Both ranks' results, each passed through `check` as it arrives: a rank that already shows
    the failure ends the run there (the other may be waiting in a collective that this one
    skipped; nobody waits for that to time out)."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, mode, tuple(refusing), q))
             for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            r, peer, calls, err, warns = q.get(timeout=120)
            res[r] = {"peer": peer, "calls": calls, "err": err, "warns": warns}
            check(res[r])
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0, p.exitcode
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
                p.join()
    return res


@pytest.mark.timeout(300)
@pytest.mark.parametrize("refusing", [(0, 1), (1,)], ids=["both", "rank1-only"])
def test_auto_over_capacity_every_rank_keeps_rccl(refusing):
    def check(x):
        assert x["peer"] is False and not x["err"], x
        assert x["calls"] == ["comm_init", "peer_export"], x["calls"]
        assert any("peer exchange unavailable" in m and "RCCL carries the exchange" in m
                   for m in x["warns"]), x["warns"]

    res = _run("auto", check, refusing)
    assert res[0]["warns"] == res[1]["warns"]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("refusing", [(0, 1), (0,)], ids=["both", "rank0-only"])
def test_peer_required_over_capacity_raises_the_same_on_every_rank(refusing):
    def check(x):
        assert "peer exchange unavailable" in x["err"], x
        assert "exceed the exchange's 65536 elements" in x["err"]
        assert x["calls"] == ["peer_export"], x["calls"]

    res = _run("peer", check, refusing)
    assert res[0]["err"] == res[1]["err"]
