"""Shapes, sizes, seeds and inputs shared by tests/test_gpu_wide_large.py and
tests/test_wide_large_cpu.py: the wide family's large heads (csrc/mbwide.hip at hidden 64 with
obs_dim up to 384 and up to 32 actions, csrc/dispatch.cpp wide_large_shape).  Test infrastructure
only; NumPy, the oracle and the layout query, no GPU.  Inputs, oracles and bounds are
tests/wide_mb_cases.py's (inputs / oracle_gradient / check_gradient) and tests/wide_act_cases.py's.

Groups (a case is wide_mb_cases' tuple (group, seed, hidden, D, A, Gaussian, T, N, M, m)):

I  one shape per new wide_mb_kernel<64, CONT, NB1, false, AB>, m = 379 (12 tiles, 6 workgroups);
W  first-layer widths: a 16-column block boundary on each side of every new NB1 (12, 16, 24:
   D16 144 .. 384) and the two Humanoid widths, all with 17 actions (two action blocks),
   m = 71 (one workgroup, three tiles);
C  action counts 15, 16, 17, 20, 31, 32 at D = 136 and 17, 32 at D = 8, both heads, m = 135 (two
   workgroups with three and two tiles);
and the same W and C shapes at m = 7 (one partial tile) and through the old-policy evaluation.
"""
import numpy as np

from diamond import _native as N
from oracle import ppo_np as P

import gpu_helpers as G
import wide_act_cases as W
import wide_mb_cases as C

HID = 64
MAX_D, MAX_A = 384, 32
S = C.S

# the gradient recipe: B = 384 records, one minibatch of B - 5 = 379 (the last tile partial)
T, NN, M, RAGGED = 8, 48, 1, 5
MB = T * NN // M - RAGGED
assert MB == C.SMALL_MB == 379


def ab(A):
    """Blocks of 16 actions the instantiation holds (wide_*_kernel's AB).  Not visible through the
    ABI."""
    return 2 if A > 16 else 1


def nb1(D):
    """launch_wide_mb's choice of NB1 for a large-head shape (wide_mb_cases.nb1 up to D16 = 128)."""
    d = C.d16(D)
    return C.nb1(D) if d <= 128 else 12 if d <= 192 else 16 if d <= 256 else 24


def is_large(Hd, D, A):
    """csrc/dispatch.cpp wide_large_shape"""
    return Hd == HID and 1 <= D <= MAX_D and 1 <= A <= MAX_A and (D > 128 or A > 16)


# ---- I: (D, A, Gaussian), one per new (CONT, NB1, AB)
INSTANTIATIONS = [
    (8, 17, False), (40, 20, False), (100, 32, False), (136, 24, False), (200, 17, False),
    (300, 32, False), (150, 5, False), (250, 16, False), (384, 3, False),
    (20, 32, True), (50, 17, True), (128, 18, True), (190, 32, True), (256, 17, True),
    (376, 17, True), (129, 1, True), (193, 16, True), (348, 9, True),
]
NEW = {(cont, nb, a) for cont in (False, True) for nb in (2, 4, 8, 12, 16, 24) for a in (1, 2)
       if nb > 8 or a == 2}


def instantiation_of(shape):
    D, A, cont = shape
    return cont, nb1(D), ab(A)


assert {instantiation_of(s) for s in INSTANTIATIONS} == NEW and len(INSTANTIATIONS) == 18
assert all(is_large(HID, D, A) for D, A, _ in INSTANTIATIONS)

# ---- W: first-layer widths
WIDTH_D = [129, 143, 144, 145, 191, 192, 193, 255, 256, 257, 348, 376, 383, 384]
HUMANOID = [(348, 17, True), (376, 17, True)]
WIDTH_A, WIDTH_MB = 17, 71
# ---- C: action counts
ACTION_A = {136: [15, 16, 17, 20, 31, 32], 8: [17, 32]}
ACTION_MB = 135
TINY_MB = 7
# ---- old-policy evaluation: a whole number of tiles, then a partial one
EVAL_TN = [(4, 32), (5, 21)]
assert [t * n for t, n in EVAL_TN] == [128, 105]
# ---- learn() through the public classes
LEARN_SHAPES = [(348, 17, True), (136, 20, False)]
LEARN_T, LEARN_N, LEARN_E, LEARN_M = 8, 32, 2, 4
# ---- off-policy: the noise on the parameters after prepare (gpu_helpers.perturbed_params), by
# head: the scales of gpu_helpers.OFFPOLICY_SHAPES' categorical and many-action Gaussian rows,
# halved for up to 32 Gaussian dims
OFFPOLICY_S = {False: 0.2, True: 0.01}


def width_shapes():
    """(D, A, Gaussian) of group W: the Humanoid widths Gaussian, the edges categorical"""
    return [(D, WIDTH_A, (D, WIDTH_A, True) in HUMANOID) for D in WIDTH_D]


def action_shapes():
    return [(D, A, cont) for D, As in ACTION_A.items() for A in As for cont in (False, True)]


def _case(grp, seed, shape, mb):
    D, A, cont = shape
    return (grp, seed, HID, D, A, cont, T, NN, M, mb)


def cases_of(group):
    if group == "I":
        return [_case("I", 1100 + j, s, MB) for j, s in enumerate(INSTANTIATIONS)]
    if group == "W":
        return [_case("W", 1200 + j, s, WIDTH_MB) for j, s in enumerate(width_shapes())]
    if group == "C":
        return [_case("C", 1300 + j, s, ACTION_MB) for j, s in enumerate(action_shapes())]
    raise KeyError(group)


def small_cases():
    return cases_of("I") + cases_of("W") + cases_of("C")


def sweep_cases():
    """Every width and action case: what the evaluation, the tiny minibatch, the actor heads and
    the oracle mutations run over."""
    return cases_of("W") + cases_of("C")


case_id = C.case_id


def shape_id(s):
    return C.shape_id((HID, *s))


def eval_dims(D, A, cont, t, n):
    return N.Dims(t, n, D, A, int(cont), HID, 1, 1, 1, 0)


def eval_inputs(case, t, n):
    """(params, flat, host rollout [t][n]) of a case's evaluation: its own parameters (the layout
    does not depend on T and N), a rollout of the size"""
    _grp, seed, Hd, D, A, cont, *_ = case
    _L, _names, params, flat, _host = C.inputs(seed, Hd, D, A, cont, T, NN, M)
    return params, flat, G.synth_host(t, n, D, A, cont, 2500 + seed + t)


def offpolicy_params(case):
    """(new params dict, flat) of a case: its parameters moved by OFFPOLICY_S of their own scale"""
    _grp, seed, Hd, D, A, cont, *_ = case
    L, names, params, _flat, _host = C.inputs(seed, Hd, D, A, cont, T, NN, M)
    return G.perturbed_params(L, names, params, OFFPOLICY_S[cont],
                              np.random.default_rng(4000 + seed))


def offpolicy_idx(case, new, records):
    """The case's minibatch among the samples whose ratio exp(logp_new - logp_old) is neither
    within gpu_helpers.NEAR_BOUND of a clip bound nor outside RATIO_RANGE (float64 new log-probs on
    `records`): (idx, the regime of every chosen sample)."""
    _grp, seed, Hd, D, A, cont, _T, _N, _M, mb = case
    _L, _names, _params, _flat, host = C.inputs(seed, Hd, D, A, cont, T, NN, M)
    obs, _, act, *_ = host
    B = T * NN
    obs_f = obs.reshape(B, D)
    act_f = act.reshape(B, A) if cont else act.reshape(B)
    ratio = np.exp(G.new_policy_logp64(new, obs_f, act_f, cont) - records["log_probs"])
    reg, _near, _far = G.surrogate_regimes(ratio, records["advantages"], P.Hyper().ppo_clip)
    ok = np.flatnonzero(reg >= 0)
    idx = np.random.RandomState(3000 + seed).permutation(ok)[:mb].astype(np.int32)
    return idx, reg[idx]


# ---- the rollout sampler (wide_act_kernel<64, CONT, AB>)
ACT_N = 33
ACT_SHAPES = sorted({(D, A, cont) for D, A, cont in width_shapes() + action_shapes()})
GAUSS_DRAW_SHAPES = [(136, 17, True), (136, 32, True), (8, 17, True), (8, 32, True),
                     (376, 17, True)]
CAT_DRAW_SHAPE = (136, 32, False)
GRID_STRIDE_SHAPES = [(376, 17, True), (136, 32, False)]
# 31 CDF boundaries with a margin of 1e-4 on each side leave a sample in 160 undecided, more than
# MIN_CLEAR allows among 33: a call counter at which every discrete case below is clear
SEED, COUNTER = W.SEED, 55


def act_inputs(D, A, cont, n=ACT_N):
    return W.inputs(HID, D, A, cont, n)


def peaked_last_inputs(n=4 * ACT_N):
    """CAT_DRAW_SHAPE's inputs with the output bias of the last action raised by log(A): the last
    action holds about half the mass, so the inverse CDF runs through every action before it on
    half the samples (the remainder branch) and stops at one of them, 16 and above included, on
    the other half."""
    D, A, cont = CAT_DRAW_SHAPE
    params, flat, obs = act_inputs(D, A, cont, n)
    params = {k: np.array(v) for k, v in params.items()}
    params["actor_head.2.bias"][-1] += np.float32(np.log(A))
    L = N.param_layout(W.dims(HID, D, A, cont))
    return params, G.flat32(L, P.DISCRETE_NAMES, params), obs


# ---- regimes (tests/regime_cases.py's transforms at large-head shapes; n = 33 sampler inputs)
PEAKED_SHAPE, PEAKED_GAP = (136, 32, False), 230.0
SIGMA_SHAPE = (136, 17, True)
SIGMA_LOG_STD = {"sigma.05": -3.0, "sigma4.5": 1.5}


def regime_sampler_inputs(name):
    """(params, flat, obs, Gaussian) of a regime's sampler case.  peaked: the output weights and
    bias scaled so that the largest logit gap of a sample is PEAKED_GAP in float64."""
    D, A, cont = PEAKED_SHAPE if name == "peaked" else SIGMA_SHAPE
    params, _flat, obs = act_inputs(D, A, cont)
    params = {k: np.array(v) for k, v in params.items()}
    if name == "peaked":
        p64 = {k: v.astype(np.float64) for k, v in params.items()}
        out = P.forward(p64, obs, False, np.float64)["out"]
        k = np.float32(PEAKED_GAP / (out.max(1) - out.min(1)).max())
        params["actor_head.2.weight"] *= k
        params["actor_head.2.bias"] *= k
    else:
        params["actor_log_std"][:] = SIGMA_LOG_STD[name]
    L = N.param_layout(W.dims(HID, D, A, cont))
    names = P.CONTINUOUS_NAMES if cont else P.DISCRETE_NAMES
    return params, G.flat32(L, names, params), obs, cont
