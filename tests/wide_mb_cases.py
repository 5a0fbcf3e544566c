"""Shapes, sizes, seeds, inputs and bounds shared by tests/test_gpu_wide_mb.py and
tests/test_wide_mb_cpu.py: the launch configurations of the wide family (csrc/mbwide.hip
wide_mb_kernel, wide_eval_kernel, wide_pack_kernel) that tests/test_gpu_wide.py does not reach.
Test infrastructure only; NumPy, the oracle and the layout query, no GPU.

Groups (the GPU module's sections):

A  one shape per reachable wide_mb_kernel<H, CONT, NB1>, on-policy here and off-policy through
   gpu_helpers.OFFPOLICY_SHAPES;
B  every first-layer width at which D8, D16 and the `k < D` slab guard part ways;
C  every action count 1..16, both heads;
D  minibatches of 3, 5 and 7 tiles: workgroups with unequal tile counts;
E  the smallest minibatch at which wide_grid's cap at the compute-unit count binds;
F  the smallest batch at which wide_pack_kernel's grid-stride loop takes a second pass;
G  a whole learn() whose batch and minibatch are no multiple of the tile.
"""
import functools

import numpy as np

from diamond import _native as N
from oracle import ppo_np as P

import gpu_helpers as G
import wide_act_cases as W

S = 32                       # samples per tile (mbwide.hip S; dppo_fused_plan reports it as `tile`)
MI355X_CUS = W.MI355X_CUS    # the CPU module's stand-in for the device's compute-unit count
# launch_wide_pack's grid cap and block size (csrc/mbwide.hip), not visible through the ABI
PACK_BLOCKS, PACK_THREADS = 4096, 256


def d16(D):
    return (D + 15) // 16 * 16


def nb1(D):
    """16-column blocks of dW1 the instantiation holds in registers (launch_wide_mb's choice of
    wide_mb_kernel<H, CONT, NB1>).  Not visible through the ABI."""
    return 2 if d16(D) <= 32 else 4 if d16(D) <= 64 else 8


def ncb1(D):
    """16-column blocks of dW1 the kernel accumulates (the rest of the NB1 stay zero)."""
    return d16(D) // 16


def record_floats(D, A, cont):
    """Floats per sample record, as dppo_create computes it: D8 + 4 + roundup4(A) (Gaussian)."""
    return (D + 7) // 8 * 8 + 4 + ((A + 3) // 4 * 4 if cont else 0)


def wide_grid(m, cus):
    """Python restatement of mbwide.hip wide_grid: a workgroup per two tiles, capped at the
    compute-unit count, at least one.  The GPU tests take the grid from dppo_fused_plan."""
    return max(1, min(((m + S - 1) // S) // 2, cus))


def tiles_per_group(m, tile, grid):
    """(fewest, most) tiles any workgroup runs: workgroup b takes tiles b, b + grid, ..."""
    tiles = (m + tile - 1) // tile
    return tiles // grid, (tiles + grid - 1) // grid


# the small recipe of tests/test_gpu_wide.py: 12 tiles on 6 workgroups, the last tile partial
SMALL_T, SMALL_N, SMALL_M, SMALL_RAGGED = 16, 96, 4, 5
SMALL_MB = SMALL_T * SMALL_N // SMALL_M - SMALL_RAGGED  # 379

# ---- A: (hidden, D, A, Gaussian), one per reachable (H, CONT, NB1); <64, *, 2> is the tuned class
INSTANTIATIONS = [
    (128, 8, 4, False), (128, 50, 7, False), (128, 128, 16, False),
    (128, 17, 6, True), (128, 33, 3, True), (128, 105, 8, True),
    (64, 40, 5, False), (64, 128, 16, False),
    (64, 57, 11, True), (64, 105, 8, True),
]
REACHABLE = {(Hd, cont, nb) for Hd in (128, 64) for cont in (False, True) for nb in (2, 4, 8)
             if not (Hd == 64 and nb == 2)}


def instantiation_of(shape):
    Hd, D, _A, cont = shape
    return Hd, cont, nb1(D)


assert {instantiation_of(s) for s in INSTANTIATIONS} == REACHABLE and len(INSTANTIATIONS) == 10

# ---- B: first-layer widths, 4 categorical actions, three tiles on one workgroup
WIDTH_D = [15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113,
           127, 128]
WIDTH_A, WIDTH_MB = 4, 71
# ---- C: action counts
ACTION_BASES = [(128, 8), (64, 40)]
ACTION_MB = 71
# ---- D: unequal tile counts
UNEQUAL_SHAPES = [(128, 8, 4, False), (64, 105, 8, True)]
UNEQUAL_MB = [71, 135, 199]
# ---- E: the capped grid.  T = 8 and N = m // 8 + 1: B = m + 1, and B % 32 == 8
CAPPED_SHAPES = [(128, 8, 4, False), (128, 17, 6, True), (64, 105, 8, True)]
CAPPED_T = 8
CAPPED_AFTER = [7, SMALL_MB]   # the sizes taken on the same handle after the capped one
# ---- F: the pack kernel's second pass
PACK_SHAPE = (128, 128, 16, True)
PACK_T, PACK_N = 16, 1800
# ---- G: a ragged learn(): B = 105, m = 35
LEARN_SHAPES = [(128, 8, 4, False), (64, 40, 5, False)]
LEARN_T, LEARN_N, LEARN_M = 5, 21, 3


def capped_mb(cus):
    """The smallest minibatch whose tile count, halved, exceeds the compute-unit count, plus a
    partial tile: 32 (2 CUs + 1) + 7."""
    return S * (2 * cus + 1) + 7


def capped_envs(cus):
    return capped_mb(cus) // CAPPED_T + 1


def pack_first_second_pass_sample(shape=PACK_SHAPE):
    """The first sample with a 16-byte record piece that wide_pack_kernel writes in its second
    grid-stride pass (one thread per piece, PACK_BLOCKS * PACK_THREADS threads)."""
    _Hd, D, A, cont = shape
    return PACK_BLOCKS * PACK_THREADS // (record_floats(D, A, cont) // 4)


def small_cases():
    """(group, seed, hidden, D, A, Gaussian, T, N, M, m) of every on-policy gradient case of the
    groups A to D.  The seed is the case's own."""
    out = []
    t = (SMALL_T, SMALL_N, SMALL_M)
    for j, s in enumerate(INSTANTIATIONS):
        out.append(("A", 100 + j, *s, *t, SMALL_MB))
    k = 0
    for D in WIDTH_D:
        for Hd in (128, 64):
            if Hd == 128 or D >= 33:
                out.append(("B", 200 + k, Hd, D, WIDTH_A, False, *t, WIDTH_MB))
                k += 1
    k = 0
    for Hd, D in ACTION_BASES:
        for cont in (False, True):
            for A in range(1, 17):
                out.append(("C", 300 + k, Hd, D, A, cont, *t, ACTION_MB))
                k += 1
    k = 0
    for s in UNEQUAL_SHAPES:
        for mb in UNEQUAL_MB:
            out.append(("D", 400 + k, *s, *t, mb))
            k += 1
    return out


def cases_of(group):
    return [c for c in small_cases() if c[0] == group]


def capped_case(j, cus):
    shape = CAPPED_SHAPES[j]
    return ("E", 500 + j, *shape, CAPPED_T, capped_envs(cus), 1, capped_mb(cus))


def learn_first_minibatch_cases():
    """G's shapes as one on-policy gradient of learn()'s minibatch size (the CPU guard)."""
    return [("G", 700 + j, *s, LEARN_T, LEARN_N, LEARN_M, LEARN_T * LEARN_N // LEARN_M)
            for j, s in enumerate(LEARN_SHAPES)]


def case_id(c):
    grp, _seed, Hd, D, A, cont, _T, _Nn, _M, mb = c
    return f"{grp}-H{Hd}-D{D}-A{A}-{'gauss' if cont else 'cat'}-m{mb}"


def shape_id(s):
    Hd, D, A, cont = s
    return f"H{Hd}-D{D}-A{A}-{'gauss' if cont else 'cat'}"


def dims(Hd, D, A, cont, T, Nn, M):
    return N.Dims(T, Nn, D, A, int(cont), Hd, 4, M, 1, 0)


def names_of(cont):
    return P.CONTINUOUS_NAMES if cont else P.DISCRETE_NAMES


@functools.lru_cache(maxsize=4)
def inputs(seed, Hd, D, A, cont, T, Nn, M):
    """(layout, names, params dict, flat parameters, host rollout) of one case: the draws of
    tests/test_gpu_wide.py's _prepare.  Shared between tests; never modified."""
    L = N.param_layout(dims(Hd, D, A, cont, T, Nn, M))
    names = names_of(cont)
    params, flat = G.random_params(L, names, D, A, cont, np.random.default_rng(1000 + seed))
    host = G.synth_host(T, Nn, D, A, cont, 2000 + seed)
    return L, names, params, flat, host


def minibatch_idx(seed, B, mb):
    return np.random.RandomState(3000 + seed).permutation(B)[:mb].astype(np.int32)


def pack_idx(seed, B, first):
    """F's minibatch: every sample from `first` on, and as many drawn from the samples before."""
    tail = np.arange(first, B)
    head = np.random.RandomState(3000 + seed).permutation(first)[:tail.size]
    return np.random.RandomState(3001 + seed).permutation(np.concatenate([tail, head])).astype(
        np.int32)


def oracle_records(params, host, cont):
    """{log_probs, values, next_values, advantages, returns}, flat, as the float32 oracle's learn()
    computes them (the CPU module's stand-in for dppo_prepare_f32's outputs)."""
    obs, nobs, act, rew, te, tr = host
    logp, v, nv, _ = P.old_policy(params, obs, act, nobs, cont)
    adv = P.gae(rew, te, tr, v, nv)
    return {"log_probs": logp.ravel(), "values": v.ravel(), "next_values": nv.ravel(),
            "advantages": P.normalize_adv(adv).ravel(), "returns": (v + adv).ravel()}


def oracle_gradient(params, host, cont, records, idx, dt):
    """(loss, components, gradient dict) of the minibatch `idx` in precision `dt`"""
    obs, _, act, *_ = host
    B = obs.shape[0] * obs.shape[1]
    obs_f = obs.reshape(B, -1)
    act_f = act.reshape(B, -1) if cont else act.reshape(B)
    args = (obs_f[idx], act_f[idx], records["log_probs"][idx], records["advantages"][idx],
            records["returns"][idx])
    return P.minibatch_loss_grads(params, *args, P.Hyper(), cont, dt=dt)


def loss_terms(ref):
    loss, comps, _ = ref
    return loss, comps["loss_policy"], comps["loss_value"], comps["entropy"]


def check_gradient(L, names, got_flat, got_loss4, ref64, what, ref32=None):
    """The assertions of tests/test_gpu_wide.py's _check on a flat-layout gradient and the four
    loss terms {loss, policy, value, entropy}: within 2e-5 max|g| of float64 overall, each tensor
    within 1e-4 of its own scale (floored at 1e-3 max|g|), loss and entropy within
    2e-5 max(1, |x|).  With ref32 (the float32 oracle on the same inputs) the bounds of
    test_gpu_production's test_full_minibatch_gradient_vs_oracle: also no further from float64
    than 4 x the float32 oracle's own distance + 1e-6 max|g|, and all four loss terms.
    Returns (overall error / max|g|, worst per-tensor error, float32 oracle's overall error)."""
    overall, per = G.gradient_errors(L, names, got_flat, ref64[2])
    worst = max(per, key=per.get)
    o32 = None
    if ref32 is not None:
        o32, _ = G.gradient_errors(L, names, G.flat_of(L, names, ref32[2]), ref64[2])
    print(f"{what}: overall {overall:.3g} worst tensor {per[worst]:.3g} ({worst})" +
          (f" float32 oracle {o32:.3g}" if o32 is not None else ""))
    assert np.isfinite(np.asarray(got_flat)).all(), what
    assert overall <= 2e-5, (what, overall)
    if o32 is not None:
        assert overall <= 4 * o32 + 1e-6, (what, overall, o32)
    for n in names:
        assert per[n] <= 1e-4, (what, n, per[n])
    want = loss_terms(ref64)
    for k in ((0, 1, 2, 3) if ref32 is not None else (0, 3)):
        assert abs(got_loss4[k] - want[k]) <= 2e-5 * max(1.0, abs(want[k])), \
            (what, k, tuple(got_loss4), want)
    return overall, per[worst], o32
