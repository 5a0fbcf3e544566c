"""Shapes, geometries, seeds and helpers shared by tests/test_wide_dp_cpu.py and
tests/test_gpu_wide_dp.py: the wide kernel family (csrc/mbwide.hip) on several ranks
(dppo_dims.wide_ranks / PPOConfig.wide_data_parallel).  Test infrastructure only.  Nothing here
touches the GPU at import; the run_* helpers (copied from tests/test_gpu_dataparallel.py, taking a
hidden width and wide_ranks) do when called.

Geometries (the GPU module's sections):

RAGGED     T = 5, 21 envs per rank, M = 3: m = 35, one full and one 3-sample tile per rank;
MULTI      T = 8, 67 envs per rank, M = 2: m = 268, nine tiles on four workgroups, the last
           tile partial;
STRADDLE   global minibatches, T = 16, 32 envs per rank, M = 8: 512 samples per global minibatch,
           per-rank shares around 64 = two tiles -- two- and three-tile shares on a grid of 8;
UNEVEN     global minibatches, T = 4, 2 envs per rank, M = 8 (the geometry and seed of
           test_gpu_dataparallel.py::test_global_minibatch_shares_are_uneven_and_exact): shares
           of 0 to >= 3 samples on a grid of 1.
"""
import ctypes
import threading

import numpy as np

from diamond import _native as N
from oracle import ppo_np as P

from gpu_helpers import random_params, synth_host
from wide_mb_cases import MI355X_CUS, S, names_of, tiles_per_group, wide_grid  # noqa: F401

WORLD = 8
E = 4
PEER_CAPACITY = 65536   # kPeerChunk * kPeerMaxSlices (csrc/common.h), elements of one exchange

# (hidden, D, A, Gaussian): both widths, both heads, NB1 = 2, 4, 8
SHAPES = [(128, 8, 4, False), (128, 17, 6, True), (64, 105, 8, True), (64, 40, 5, False)]
OVER_CAPACITY = (128, 128, 16, True)

RAGGED = dict(T=5, Nl=21, M=3)
MULTI = dict(T=8, Nl=67, M=2)
MULTI_SHAPES = [SHAPES[0], SHAPES[2]]
STRADDLE = dict(T=16, Nl=32, M=8)
STRADDLE_SHAPES = [SHAPES[0], SHAPES[1]]
STRADDLE_PERM_SEED = 42
UNEVEN = dict(T=4, Nl=2, M=8)
UNEVEN_SHAPES = [(128, 8, 3, False), (64, 40, 5, False)]
UNEVEN_PERM_SEED = 3
# two processes on one GPU through the drop-in agents
AGENT = dict(T=8, Nl=16, M=2)
AGENT_SHAPES = [(128, 8, 4), (64, 40, 5)]
AGENT_PERM_SEED = 4321
AGENT_DATA_SEED = 900


def shape_id(s):
    Hd, D, A, cont = s
    return f"H{Hd}-D{D}-A{A}-{'gauss' if cont else 'cat'}"


def dims(Hd, D, A, cont, T, Nn, M, world=1, rank=0, gmb=0, wide_ranks=0):
    return N.Dims(T, Nn, D, A, int(cont), Hd, E, M, world, rank, int(gmb), int(wide_ranks))


def handle_grid(T, Nl, M, world, gmb, cus=MI355X_CUS):
    """dppo_create's h->G for the wide class: wide_grid of a local minibatch, or, with global
    minibatches, of a whole global one (capped at the rank's batch)."""
    B = T * Nl
    return wide_grid(min(B * world // M, B) if gmb else B // M, cus)


def global_perms(seed, Bg, n=1):
    """n learns' worth of [E][Bg] global permutations, drawn one after the other from one
    RandomState as np.random.permutation draws them."""
    rs = np.random.RandomState(seed)
    out = [np.stack([rs.permutation(Bg) for _ in range(E)]).astype(np.int32) for _ in range(n)]
    return out


def local_perms(B, world=WORLD, base=100):
    return [np.stack([np.random.RandomState(base + r).permutation(B) for _ in range(E)])
            .astype(np.int32) for r in range(world)]


def share_counts(perms_g, Nl, M, world=WORLD):
    """[E][M][world]: how many samples of global minibatch j fall in rank r's env shard (global
    flat index t * Ng + n, shard [r * Nl, (r + 1) * Nl))."""
    Ng = Nl * world
    mbg = perms_g.shape[1] // M
    rank_of = (perms_g % Ng) // Nl
    return np.array([[[int((rank_of[e, j * mbg:(j + 1) * mbg] == r).sum()) for r in range(world)]
                      for j in range(M)] for e in range(perms_g.shape[0])])


def union_perms(perms, T, Nl, M, world=WORLD):
    """Global permutations whose minibatch j is the union of the ranks' local minibatches j."""
    Ng, B = Nl * world, T * Nl
    mb = B // M
    to_global = lambda r, i: (i // Nl) * Ng + r * Nl + i % Nl
    return np.stack([np.concatenate([to_global(r, perms[r][e, j * mb:(j + 1) * mb])
                                     for j in range(M) for r in range(world)])
                     for e in range(E)])


def setup(Hd, T, Nl, D, A, cont, seed, world=WORLD):
    """(layout, names, params dict, flat parameters, host rollout of the global batch)."""
    L = N.param_layout(dims(Hd, D, A, cont, T, Nl, 1))
    names = names_of(cont)
    params, flat0 = random_params(L, names, D, A, cont, np.random.default_rng(seed))
    host = synth_host(T, Nl * world, D, A, cont, seed)
    host = tuple(x if x.dtype != np.uint8 else x.astype(bool) for x in host)
    return L, names, params, flat0, host


def shard(host, r, Nl):
    sl = slice(r * Nl, (r + 1) * Nl)
    obs, nobs, act, rew, te, tr = host
    return [[obs[k, sl], nobs[k, sl], act[k, sl], rew[k, sl], te[k, sl].astype(bool),
             tr[k, sl].astype(bool)] for k in range(obs.shape[0])]


def run_loopback(Hd, T, Nl, D, A, cont, M, flat0, host, learns, global_mb, targets=False,
                 wide_ranks=1):
    """WORLD ranks in one loopback group.  `learns`: one entry per consecutive learn on the same
    handles, parameters and Adam state -- the global permutations (or swap targets) when
    global_mb, else the list of the ranks' local ones.  Returns, per learn, the per-rank
    (params, trace)."""
    import torch
    import diamond
    from gpu_helpers import dev, hparams
    handles = [N.Handle(0, dims(Hd, D, A, cont, T, Nl, M, WORLD, r, global_mb, wide_ranks))
               for r in range(WORLD)]
    # a rank that refused a launch would leave the others in the group barrier for its bound
    classes = [h.fused_plan(T * Nl // M)["shape_class"] for h in handles]
    assert classes == ["wide"] * WORLD, classes
    N.loopback_group(handles)
    state = []
    for r in range(WORLD):
        ro = diamond.engine.stage_experience(shard(host, r, Nl), dev(), cont)
        state.append({"ro": ro, "st": ro.as_struct(), "p": torch.from_numpy(flat0).to(dev()),
                      "m": torch.zeros(len(flat0), device=dev()),
                      "v": torch.zeros(len(flat0), device=dev()), "rc": 0, "err": b"",
                      "out": []})
    torch.cuda.synchronize()

    def run(r):
        torch.cuda.set_device(0)
        s = torch.cuda.Stream(device=dev())
        x = state[r]
        fn = handles[r].lib.dppo_learn_targets_f32 if targets else handles[r].lib.dppo_learn_f32
        for k, perms in enumerate(learns):
            pr = perms if global_mb else perms[r]
            hp = hparams(adam_step=k * E * M)
            x["rc"] = fn(handles[r].h, ctypes.byref(x["st"]), x["p"].data_ptr(),
                         x["m"].data_ptr(), x["v"].data_ptr(), ctypes.byref(hp), pr.ctypes.data,
                         None, s.cuda_stream)
            if x["rc"] != 0:
                x["err"] = handles[r].lib.dppo_last_error()   # thread-local: read on this thread
                return
            s.synchronize()
            x["out"].append((x["p"].cpu().numpy(), handles[r].trace(E * M)))

    th = [threading.Thread(target=run, args=(r,)) for r in range(WORLD)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=240)
    assert all(not x.is_alive() for x in th)
    bad = [(r, x["rc"], x["err"]) for r, x in enumerate(state) if x["rc"] != 0]
    assert not bad, bad
    torch.cuda.synchronize()
    out = [[state[r]["out"][k] for r in range(WORLD)] for k in range(len(learns))]
    for h in handles:
        h.close()
    return out


def run_single(Hd, T, Ng, D, A, cont, M, flat0, host, perms_g):
    """World-1 libdppo learn of the whole global buffer with the given global permutations."""
    import torch
    import diamond
    from gpu_helpers import dev, hparams, stream
    h = N.Handle(0, dims(Hd, D, A, cont, T, Ng, M))
    assert h.fused_plan(T * Ng // M)["shape_class"] == "wide"
    obs, nobs, act, rew, te, tr = host
    exp = [[obs[k], nobs[k], act[k], rew[k], te[k].astype(bool), tr[k].astype(bool)]
           for k in range(T)]
    ro = diamond.engine.stage_experience(exp, dev(), cont)
    p = torch.from_numpy(flat0).to(dev())
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    hp = hparams()
    pg = np.ascontiguousarray(perms_g, dtype=np.int32)
    N.check(h.lib.dppo_learn_f32(h.h, ctypes.byref(ro.as_struct()), p.data_ptr(), m.data_ptr(),
                                 v.data_ptr(), ctypes.byref(hp), pg.ctypes.data, None, stream()))
    torch.cuda.synchronize()
    res = (p.cpu().numpy(), h.trace(E * M))
    h.close()
    return res


def oracle_learns(params, names, host, perms_list, cont, M):
    """The float32 oracle's consecutive learns of the global batch (params and Adam state carried
    on); per learn (trace, copy of the parameters after it).  `params` is not modified.  `host`
    is one rollout for every learn, or a list with one rollout per learn."""
    params = {n: params[n].copy() for n in names}
    adam = P.new_adam_state(params, names)
    hosts = host if isinstance(host, list) else [host] * len(perms_list)
    assert len(hosts) == len(perms_list)
    out = []
    for host, perms_g in zip(hosts, perms_list):
        ref = P.learn(params, adam, list(host), P.Hyper(num_minibatches=M), 3e-4, cont,
                      perms=perms_g)
        out.append((ref, {n: params[n].copy() for n in names}))
    return out


def check_vs_oracle(out, ref, ref_params, names, L, what=""):
    """The bounds of test_gpu_dataparallel.py's check_vs_oracle and test_ragged_learn_vs_oracle:
    every rank's parameters bit-equal to rank 0's, losses and norms rtol 1e-4 / atol 1e-5,
    parameters atol 2e-5.  Prints the figures before it asserts."""
    flats = [p for p, _ in out]
    tr0 = out[0][1]
    perr = max(float(np.abs(flats[0][L.offset[i]:L.offset[i] + L.numel[i]] -
                            ref_params[n].ravel()).max()) for i, n in enumerate(names))
    lerr = float(np.abs(tr0[:, 0] - np.asarray(ref["loss"])).max())
    print(f"{what}: max |param - oracle| {perr:.3g}, max |loss - oracle| {lerr:.3g}")
    for r in range(1, len(out)):
        assert np.array_equal(flats[0], flats[r]), (what, r)
    for r in range(len(out)):
        tr = out[r][1]
        np.testing.assert_allclose(tr[:, 0], ref["loss"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(tr[:, 4], ref["norm"], rtol=1e-4, atol=1e-5)
    for i, n in enumerate(names):
        np.testing.assert_allclose(flats[0][L.offset[i]:L.offset[i] + L.numel[i]],
                                   ref_params[n].ravel(), rtol=0, atol=2e-5, err_msg=n)
