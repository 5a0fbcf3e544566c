"""GPU tests of the wide kernel family (csrc/mbwide.hip) on several ranks: the opt-in
dppo_dims.wide_ranks / PPOConfig.wide_data_parallel.  World 8 runs as a
single-device loopback group (tests/test_gpu_dataparallel.py explains why), two ranks through the
drop-in agents as two processes on the one GPU under DPPO_COMM=peer.  Shapes, geometries and seeds
are tests/wide_dp_cases.py's; tests/test_wide_dp_cpu.py asserts what they rest on.

The float32 oracle's learns are computed once per case and shared (never modified)."""
import functools
import multiprocessing as mp
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from diamond import _native as N
from oracle import ppo_np as P

import wide_dp_cases as C

WORLD = C.WORLD


# ---- 4: the class through the ABI.  First in the file: a rank of a loopback group that refused
# its launches would leave the others in the group barrier for its bound.
@pytest.mark.parametrize("shape", C.SHAPES + [C.OVER_CAPACITY], ids=C.shape_id)
def test_class_through_the_abi(shape):
    Hd, D, A, cont = shape
    T, Nl, M = 16, 32, 8
    for gmb in (0, 1):
        for rank in (0, 1):
            h = N.Handle(0, C.dims(Hd, D, A, cont, T, Nl, M, 2, rank, gmb, 1))
            plan = h.fused_plan(T * Nl // M)
            assert plan["shape_class"] == "wide" and plan["tile"] == C.S, (gmb, rank, plan)
            h.close()
        h = N.Handle(0, C.dims(Hd, D, A, cont, T, Nl, M, 2, 0, gmb, 0))
        assert h.fused_plan(T * Nl // M)["shape_class"] is None
        h.close()
    h = N.Handle(0, C.dims(Hd, D, A, cont, T, Nl, M, 1, 0, 0, 1))   # no effect on one rank
    assert h.fused_plan(T * Nl // M)["shape_class"] == "wide"
    h.close()


def test_flag_does_not_touch_the_other_classes():
    for Hd, D, A, want in ((64, 4, 2, "tuned"), (128, 129, 4, None), (256, 8, 4, None),
                           (128, 8, 17, None)):
        for wr in (0, 1):
            h = N.Handle(0, C.dims(Hd, D, A, False, 4, 32, 1, 2, 0, 0, wr))
            assert h.fused_plan(128)["shape_class"] == want, (Hd, D, A, wr)
            h.close()
    with pytest.raises(ValueError, match="wide_ranks"):
        N.Handle(0, C.dims(128, 8, 4, False, 4, 32, 1, 2, 0, 0, 2))


# ---- 5: local minibatches against the oracle
@functools.lru_cache(maxsize=None)
def _local_case(shape, geom):
    Hd, D, A, cont = shape
    g = getattr(C, geom)
    T, Nl, M = g["T"], g["Nl"], g["M"]
    L, names, params, flat0, host = C.setup(Hd, T, Nl, D, A, cont, seed=40 + Hd + D)
    perms = C.local_perms(T * Nl)
    ref, ref_params = C.oracle_learns(params, names, host, [C.union_perms(perms, T, Nl, M)],
                                      cont, M)[0]
    return L, names, flat0, host, perms, ref, ref_params


@pytest.mark.parametrize("shape,geom", [(s, "RAGGED") for s in C.SHAPES] +
                         [(s, "MULTI") for s in C.MULTI_SHAPES],
                         ids=lambda v: v if isinstance(v, str) else C.shape_id(v))
def test_world8_local_minibatches_vs_oracle(shape, geom):
    """RAGGED: every rank one workgroup on a full and a 3-sample tile; MULTI: nine tiles on four
    workgroups.  The oracle learns the global batch whose minibatch j is the union of the ranks'
    local minibatches j."""
    Hd, D, A, cont = shape
    g = getattr(C, geom)
    L, names, flat0, host, perms, ref, ref_params = _local_case(shape, geom)
    out, = C.run_loopback(Hd, g["T"], g["Nl"], D, A, cont, g["M"], flat0, host, [perms],
                          global_mb=False)
    C.check_vs_oracle(out, ref, ref_params, names, L, f"{C.shape_id(shape)} {geom}")


# ---- 6, 9: global minibatches reproduce world 1; determinism
@functools.lru_cache(maxsize=None)
def _straddle_case(shape):
    Hd, D, A, cont = shape
    g = C.STRADDLE
    T, Nl, M = g["T"], g["Nl"], g["M"]
    L, names, params, flat0, host = C.setup(Hd, T, Nl, D, A, cont, seed=31 + Hd + D)
    perms_g, = C.global_perms(C.STRADDLE_PERM_SEED, T * Nl * WORLD)
    ref, ref_params = C.oracle_learns(params, names, host, [perms_g], cont, M)[0]
    return L, names, params, flat0, host, perms_g, ref, ref_params


@pytest.mark.parametrize("shape", C.STRADDLE_SHAPES, ids=C.shape_id)
def test_world8_global_minibatches_reproduce_world1(shape):
    """512 samples per global minibatch, per-rank shares around 64: two- and three-tile shares on
    the handle's grid of 8, so every launch has workgroups that run no tile.  Against the oracle's
    learn with the same global permutations, and against the world-1 wide learn of the 256-env
    buffer at the bounds of test_world8_global_minibatches_reproduce_world1_oracle (parameters
    5e-6, losses rtol 2e-5 / atol 2e-6; set on the tuned class).  Run twice from the same state:
    identical parameters and traces.

    Measured on an MI355X, world 8 against world 1 (max over the parameters; max relative loss
    difference): 6.0e-8 and 1.7e-7 at H128 D8 A4 categorical, 1.2e-7 and 2.4e-7 at H128 D17 A6
    Gaussian -- the wide class meets the tuned class's bounds, which stand unwidened.  Against the
    oracle: parameters 6.0e-8 / 1.8e-7, losses 2.8e-6 / 4.3e-6."""
    Hd, D, A, cont = shape
    g = C.STRADDLE
    T, Nl, M = g["T"], g["Nl"], g["M"]
    L, names, params, flat0, host, perms_g, ref, ref_params = _straddle_case(shape)
    out, = C.run_loopback(Hd, T, Nl, D, A, cont, M, flat0, host, [perms_g], global_mb=True)
    single = C.run_single(Hd, T, Nl * WORLD, D, A, cont, M, flat0, host, perms_g)
    dp = float(np.abs(out[0][0] - single[0]).max())
    dl = float((np.abs(out[0][1][:, 0] - single[1][:, 0]) /
                np.maximum(np.abs(single[1][:, 0]), 1e-12)).max())
    print(f"{C.shape_id(shape)}: world 8 vs world 1: max |dparam| {dp:.3g}, max rel dloss {dl:.3g}")
    C.check_vs_oracle(out, ref, ref_params, names, L, f"{C.shape_id(shape)} STRADDLE")
    np.testing.assert_allclose(out[0][1][:, 0], single[1][:, 0], rtol=2e-5, atol=2e-6)
    np.testing.assert_allclose(out[0][0], single[0], rtol=0, atol=5e-6)
    again, = C.run_loopback(Hd, T, Nl, D, A, cont, M, flat0, host, [perms_g], global_mb=True)
    for r in range(WORLD):
        assert np.array_equal(again[r][0], out[r][0]) and np.array_equal(again[r][1], out[r][1]), r


# ---- 7: uneven and empty shares, twice on the same handles
@pytest.mark.parametrize("shape", C.UNEVEN_SHAPES, ids=C.shape_id)
def test_uneven_and_empty_shares_two_learns(shape):
    """Shares of 0 to >= 3 samples on a grid of one workgroup: the zero-sample share and the
    workgroup that runs no tile.  The second learn on the same handles follows launches with
    larger shares: a slab left over from them would show."""
    Hd, D, A, cont = shape
    g = C.UNEVEN
    T, Nl, M = g["T"], g["Nl"], g["M"]
    L, names, params, flat0, host = C.setup(Hd, T, Nl, D, A, cont, seed=5)
    learns = C.global_perms(C.UNEVEN_PERM_SEED, T * Nl * WORLD, 2)
    refs = C.oracle_learns(params, names, host, learns, cont, M)
    outs = C.run_loopback(Hd, T, Nl, D, A, cont, M, flat0, host, learns, global_mb=True)
    for k, (out, (ref, ref_params)) in enumerate(zip(outs, refs)):
        assert np.isfinite(out[0][0]).all()
        C.check_vs_oracle(out, ref, ref_params, names, L, f"{C.shape_id(shape)} UNEVEN learn {k}")


# ---- 8: swap targets
def _perms_and_targets(n, seed):
    key, pos, _ = N.mt_state(np.random.RandomState(seed))
    perms = np.empty(C.E * n, np.int32)
    N.perm_numpy(key.copy(), pos, n, C.E, perms)
    tg = np.empty(C.E * n, np.int32)
    N.perm_targets_numpy(key.copy(), pos, n, C.E, tg)
    return perms.reshape(C.E, n), tg.reshape(C.E, n)


@functools.lru_cache(maxsize=None)
def _swap_reference():
    Hd, D, A, cont = C.SHAPES[0]
    g = C.STRADDLE
    T, Nl, M = g["T"], g["Nl"], g["M"]
    L, names, params, flat0, host = C.setup(Hd, T, Nl, D, A, cont, seed=9 + T)
    perms, tg = _perms_and_targets(T * Nl * WORLD, seed=77 + T)
    ref, = C.run_loopback(Hd, T, Nl, D, A, cont, M, flat0, host, [perms], global_mb=True)
    return flat0, host, tg, ref


@pytest.mark.parametrize("walk", ["1", "0"])
def test_world8_global_minibatches_from_swap_targets(monkeypatch, walk):
    """Global minibatches from device-resolved swap targets, with the value walk and with the
    whole-permutation resolution: bit for bit the learn from host permutations on every rank."""
    monkeypatch.setenv("DPPO_PERM_WALK", walk)
    Hd, D, A, cont = C.SHAPES[0]
    g = C.STRADDLE
    flat0, host, tg, ref = _swap_reference()
    got, = C.run_loopback(Hd, g["T"], g["Nl"], D, A, cont, g["M"], flat0, host, [tg],
                          global_mb=True, targets=True)
    for r in range(WORLD):
        assert np.array_equal(got[r][0], ref[r][0]) and np.array_equal(got[r][1], ref[r][1]), r


# ---- 10: two processes on one GPU through the drop-in agents
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(kind, tmp_path, args=(), world=2):
    from dist_scripts import wide_peer_dp
    ctx = mp.get_context("spawn")
    port = _free_port()
    outs = [str(tmp_path / f"{kind}_r{r}.npz") for r in range(world)]
    procs = [ctx.Process(target=wide_peer_dp.run, args=(r, world, port, kind, outs[r], args))
             for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(200)
    for p in procs:
        if p.is_alive():
            p.kill()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return [np.load(o) for o in outs]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("Hd,D,A", C.AGENT_SHAPES)
def test_two_processes_drop_in_agents(tmp_path, Hd, D, A):
    g = C.AGENT
    T, Nl, M = g["T"], g["Nl"], g["M"]
    r0, r1 = _spawn("agent", tmp_path, (Hd, D, A, True))
    names = P.DISCRETE_NAMES
    for r in (r0, r1):
        assert str(r["shape_class"]) == "wide" and int(r["fused"]) == 1 and int(r["wide_ranks"]) == 1
    for n in names:
        assert np.array_equal(r0["init/" + n], r1["init/" + n]), n
        assert np.array_equal(r0["final/" + n], r1["final/" + n]), n
    assert np.array_equal(r0["trace"], r1["trace"])
    # the oracle's learn of the two-rank global batch
    from gpu_helpers import synth_host
    host = synth_host(T, Nl * 2, D, A, False, C.AGENT_DATA_SEED + Hd + D)
    host = tuple(x if x.dtype != np.uint8 else x.astype(bool) for x in host)
    # what each rank's learn drew: E consecutive permutations from its own seeded stream
    perms = [C.global_perms(C.AGENT_PERM_SEED + r, T * Nl)[0] for r in range(2)]
    params = {n: r0["init/" + n].copy() for n in names}
    ref, ref_params = C.oracle_learns(params, names, host,
                                      [C.union_perms(perms, T, Nl, M, world=2)], False, M)[0]
    tr = r0["trace"]
    perr = max(float(np.abs(r0["final/" + n] - ref_params[n]).max()) for n in names)
    print(f"H{Hd} D{D} A{A}: two ranks vs oracle: max |dparam| {perr:.3g}")
    np.testing.assert_allclose(tr[:, 0], ref["loss"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(tr[:, 4], ref["norm"], rtol=1e-4, atol=1e-5)
    for n in names:
        np.testing.assert_allclose(r0["final/" + n], ref_params[n], rtol=0, atol=2e-5, err_msg=n)
        assert np.abs(r0["final/" + n] - r0["init/" + n]).max() > 0


@pytest.mark.timeout(300)
def test_two_processes_flag_off_keeps_the_generic_path(tmp_path):
    Hd, D, A = C.AGENT_SHAPES[0]
    for r in _spawn("agent", tmp_path, (Hd, D, A, False)):
        assert str(r["shape_class"]) == "None" and int(r["fused"]) == 0
        assert int(r["wide_ranks"]) == 0


@pytest.mark.timeout(300)
def test_two_processes_over_capacity_raise_on_every_rank(tmp_path):
    errs = [str(r["err"]) for r in _spawn("capacity", tmp_path)]
    for e in errs:
        assert "peer exchange unavailable" in e and "exceed the exchange's 65536 elements" in e, e
    assert errs[0] == errs[1]
