"""The generic learn under data parallelism (NativeLearner._learn_generic and the torch loop of
RecurrentPPO.learn at world > 1) against the oracle.  Cases, seeds and the NumPy restatements are
tests/generic_dp_cases.py's; tests/test_generic_dp_cpu.py asserts what they rest on.

A.  dppo_adv_sums + dppo_adv_stats_from_sums, the statistics entry points of a caller that does
    its own exchange: dppo_gae_f32 on each of two env shards on its own handle, the shards' sums
    added on the host in float64 and finalised with n_total = T * N_global, against P.adv_stats of
    the oracle's GAE of the whole batch (1e-6 on the mean, 2e-6 relative on the std: the bounds
    of test_gae_vs_oracle_sizes / test_gae_stats_large_mean).  Each shard's own sums against the
    correctly rounded float64 sum and sum of squares of the oracle's advantages, within 4x the
    distance of the float32-shifted / float64-folded scheme itself, measured in a NumPy
    restatement of stats4 / stats_fold and the kernels' fixed summation order on the same inputs
    (generic_dp_cases.restated_sums).  That distance, measured on the CPU, relative to the exact
    value: sum 8.6e-10 / 2.3e-10 (plain: 16 x 48, 129 x 64) and 0 (7 x 33 and every large-mean
    case: the float64 additions are exact there); sum of squares 1.5e-9 / 8.7e-10 (plain),
    9.5e-15 / 6.2e-15 (large mean), 0 (7 x 33: the serial kernel, float64 throughout).  Where the
    distance is 0 the device must return the correctly rounded value itself.

B.  Two processes on one GPU through the drop-in agents with a subclass of the default network:
    local and global minibatches, both heads, empty / single-sample / full shares, the torch loss
    and the loss-head kernel in consecutive learns on one Adam state.  Against the float32
    oracle's two learns of the two-rank global batch: both ranks bit-equal, parameters within
    atol 2e-5, loss_head_calls = the non-empty minibatches of the fused-loss learn.

C.  RecurrentPPO's torch loop (fused_gru = False) on one and on two ranks, two learns, fused_loss
    off then on.

Measured on an MI355X.  A: every device sum equalled the restatement bit for bit, so its distance
from the exact value was the scheme's own (1.0x of the 4x allowed), and mean and std equalled
P.adv_stats' float32 values in all six cases.  B, largest |param - oracle| after learn 0 / learn 1:
B1 3.0e-8 / 3.0e-8, B2 8.9e-8 / 1.2e-7, B3 6.3e-8 / 6.3e-8, B4 1.2e-7 / 1.2e-7 -- under 1 % of the
2e-5 bound, and what the CPU restatement of the decomposition predicts (3.0e-8 to 1.4e-7); the
mistakes the CPU module applies land at 3.2e-4 to 6.3e-3.  C: world 2 against world 1 3.0e-8 after
either learn.  No test exposed a disagreement: the package and csrc/ are unchanged.  Wall time
of the module: 38 s, of which 36 s are the six spawns (5.2 to 6.6 s per two-process case, 13 s
for the recurrent test's world 1 + world 2); the seven single-process tests take 0.3 s."""
import functools
import multiprocessing as mp
import socket
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from diamond import _native as N
from oracle import ppo_np as P

import generic_dp_cases as G


# ---- A: the statistics entry points ------------------------------------------------------------
def dev():
    import torch
    return torch.device("cuda", 0)


def stream():
    import torch
    return torch.cuda.current_stream(dev()).cuda_stream


def t(x, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).to(dev()).contiguous()


def gae_handle(T, Nn):
    return N.Handle(0, N.Dims(T, Nn, 1, 1, 0, 64, 1, 1, 1, 0))


def _shard_sums(T, Nl, arrays):
    """dppo_gae_f32 + dppo_adv_sums of one shard on a handle of its own: (adv, sums[2])."""
    import torch
    h = gae_handle(T, Nl)
    r, te, tr, v, nv = arrays
    args = [t(r, torch.float32), t(te, torch.uint8), t(tr, torch.uint8), t(v, torch.float32),
            t(nv, torch.float32)]
    adv = torch.empty(T, Nl, device=dev())
    ret = torch.empty(T, Nl, device=dev())
    sums = torch.full((2,), float("nan"), dtype=torch.float64, device=dev())
    N.check(h.lib.dppo_gae_f32(h.h, *[a.data_ptr() for a in args], adv.data_ptr(), ret.data_ptr(),
                               0.99, 0.95, stream()))
    N.check(h.lib.dppo_adv_sums(h.h, sums.data_ptr(), stream()))
    torch.cuda.synchronize()
    out = adv.cpu().numpy(), sums.cpu().numpy()
    h.close()
    return out


@pytest.mark.parametrize("regime", G.STATS_REGIMES)
@pytest.mark.parametrize("T,Nl", G.STATS_SHAPES)
def test_adv_sums_of_two_shards_finalise_to_the_global_statistics(T, Nl, regime):
    import torch
    arrays = G.stats_inputs(T, Nl, regime)
    ref = P.gae(*arrays)
    total = np.zeros(2, np.float64)
    for k in range(2):
        sl = slice(k * Nl, (k + 1) * Nl)
        adv, sums = _shard_sums(T, Nl, [np.ascontiguousarray(a[:, sl]) for a in arrays])
        assert np.array_equal(adv, ref[:, sl])
        exact = G.exact_sums(ref[:, sl])
        restated = G.restated_sums(ref[:, sl])
        for i, what in enumerate(("sum", "sumsq")):
            d_scheme = abs(restated[i] - exact[i])
            d = abs(float(sums[i]) - exact[i])
            print(f"T{T} N{Nl} {regime} shard {k} {what}: |device - exact| {d:.3g}, scheme "
                  f"{d_scheme:.3g}, |exact| {abs(exact[i]):.6g}")
        for i in range(2):
            assert abs(float(sums[i]) - exact[i]) <= 4.0 * abs(restated[i] - exact[i]), (k, i)
        total += sums                                   # the host's float64 addition
    dsum = torch.from_numpy(total).to(dev())
    ms = torch.full((4,), float("nan"), device=dev())
    N.check(N.load().dppo_adv_stats_from_sums(dsum.data_ptr(), float(T * 2 * Nl), ms.data_ptr(),
                                              stream()))
    torch.cuda.synchronize()
    ms = ms.cpu().numpy()
    mean, std = P.adv_stats(ref)
    print(f"T{T} N{Nl} {regime}: mean {ms[0]} vs {mean}, std {ms[1]} vs {std}")
    assert abs(ms[0] - mean) <= 1e-6 * max(1.0, abs(mean)), (ms[0], mean)
    assert abs(ms[1] - std) <= 2e-6 * std, (ms[1], std)


def test_statistics_entry_points_refuse_bad_arguments_without_a_launch():
    import torch
    lib = N.load()
    p = 0x1000                      # never dereferenced: refused before any HIP call
    h = gae_handle(4, 16)
    assert lib.dppo_adv_sums(None, p, None) == N.DPPO_EINVAL
    assert lib.dppo_adv_sums(h.h, None, None) == N.DPPO_EINVAL
    assert b"dppo_adv_sums" in lib.dppo_last_error()
    assert lib.dppo_adv_stats_from_sums(None, 8.0, p, None) == N.DPPO_EINVAL
    assert lib.dppo_adv_stats_from_sums(p, 8.0, None, None) == N.DPPO_EINVAL
    for n_total in (0.0, 0.5, -3.0, float("nan")):
        assert lib.dppo_adv_stats_from_sums(p, n_total, p, None) == N.DPPO_EINVAL, n_total
        assert b"dppo_adv_stats_from_sums" in lib.dppo_last_error()
    torch.cuda.synchronize(dev())   # nothing was enqueued, nothing faulted
    h.close()


# ---- B: two processes through the drop-in agents -----------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_ranks(target, argsets, limit=200.0):
    """One spawned process per argument tuple.  Ends at the first rank that shows a failure (its
    peer would wait for it in a collective), or when all have exited, or at the limit; kills what
    is still alive and asserts every exit code is 0."""
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=target, args=a) for a in argsets]
    for p in procs:
        p.start()
    end = time.monotonic() + limit
    while time.monotonic() < end:
        for p in procs:
            p.join(0.05)            # returns at once for a rank that has exited
        codes = [p.exitcode for p in procs]
        if all(c is not None for c in codes) or any(c not in (None, 0) for c in codes):
            break
    codes = [p.exitcode for p in procs]
    for p in procs:
        if p.is_alive():
            p.kill()
            p.join(10)
    assert all(c == 0 for c in codes), codes


def _spawn(case, tmp_path):
    from dist_scripts import generic_dp
    port = _free_port()
    outs = [str(tmp_path / f"{case}_r{r}.npz") for r in range(G.WORLD)]
    _run_ranks(generic_dp.run, [(r, G.WORLD, port, case, outs[r]) for r in range(G.WORLD)])
    return [np.load(o) for o in outs]


@functools.lru_cache(maxsize=None)
def _oracle(case):
    return G.oracle(case)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", list(G.CASES))
def test_two_processes_generic_learn_vs_oracle(tmp_path, case):
    c = G.CASES[case]
    names = G.case_setup(case)[0]
    r0, r1 = _spawn(case, tmp_path)
    _, params, _ = G.case_setup(case)
    for n in names:
        assert np.array_equal(r0["init/" + n], params[n]), n
        assert np.array_equal(r1["init/" + n], params[n]), n
    refs = _oracle(case)
    calls_before = [0, 0]
    for k in range(G.LEARNS):
        _, ref_params = refs[k]
        d = max(float(np.abs(r0[f"final{k}/" + n].astype(np.float64) - ref_params[n]).max())
                for n in names)
        print(f"{case} learn {k} (fused_loss {c['fused_loss'][k]}): max |param - oracle| {d:.3g}")
    for k in range(G.LEARNS):
        _, ref_params = refs[k]
        # two addends commute: the ranks' clip + Adam saw the same bits
        for n in names:
            assert np.array_equal(r0[f"final{k}/" + n], r1[f"final{k}/" + n]), (k, n)
        assert np.array_equal(r0[f"m{k}"], r1[f"m{k}"]) and np.array_equal(r0[f"v{k}"], r1[f"v{k}"])
        assert np.isfinite(r0[f"m{k}"]).all() and np.isfinite(r0[f"v{k}"]).all()
        before = "init/" if k == 0 else f"final{k - 1}/"
        for n in names:
            np.testing.assert_allclose(r0[f"final{k}/" + n], ref_params[n], rtol=0, atol=G.BOUND,
                                       err_msg=f"{case} learn {k} {n}")
            assert np.abs(r0[f"final{k}/" + n] - r0[before + n]).max() > 0, (k, n)
        for r, res in enumerate((r0, r1)):
            want = G.nonempty_minibatches(case, k, r) if c["fused_loss"][k] else 0
            got = int(res[f"calls{k}"]) - calls_before[r]
            assert got == want, (case, k, r, got, want)
            calls_before[r] = int(res[f"calls{k}"])


# ---- C: RecurrentPPO's torch loop ----------------------------------------------------------------
@pytest.mark.timeout(300)
def test_recurrent_torch_loop_two_ranks_match_one(tmp_path):
    """T 16, 16 global envs, gru_hidden_dim 16, M 1, fused_gru = False: two consecutive learns,
    fused_loss off then on.  Ranks bit-equal, world 2 within atol 2e-5 of world 1 after each
    learn (the bound of test_recurrent_ppo_two_ranks_match_one), loss_head_calls = the second
    learn's 3 epochs x 1 minibatch."""
    from dist_scripts import recurrent_dp
    T, Ng, D, A, Gh = 16, 16, 5, 3, 16
    outs = {}
    for world in (1, 2):
        port = _free_port()
        argsets = []
        for r in range(world):
            outs[(world, r)] = str(tmp_path / f"w{world}_r{r}.npz")
            argsets.append((r, world, port, T, Ng, D, A, outs[(world, r)], Gh, True))
        _run_ranks(recurrent_dp.run, argsets, limit=240.0)
    one = np.load(outs[(1, 0)])
    r0, r1 = np.load(outs[(2, 0)]), np.load(outs[(2, 1)])
    assert np.array_equal(r0["init"], one["init"]) and np.array_equal(r1["init"], one["init"])
    prev = one["init"]
    for k in range(2):
        d = float(np.abs(r0[f"final{k}"] - one[f"final{k}"]).max())
        print(f"recurrent torch loop learn {k}: world 2 vs world 1 max |dparam| {d:.3g}")
    for k in range(2):
        assert np.array_equal(r0[f"final{k}"], r1[f"final{k}"]), k
        assert np.all(np.isfinite(r0[f"final{k}"]))
        assert np.abs(one[f"final{k}"] - prev).max() > 1e-4     # 3 Adam steps of lr 3e-4
        prev = one[f"final{k}"]
        np.testing.assert_allclose(r0[f"final{k}"], one[f"final{k}"], rtol=0, atol=2e-5)
        for res in (one, r0, r1):
            assert int(res[f"calls{k}"]) == (0, 3)[k], (k, int(res[f"calls{k}"]))
