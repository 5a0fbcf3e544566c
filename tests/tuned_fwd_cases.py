"""Shapes, sizes, seeds and inputs shared by tests/test_gpu_tuned_fwd.py and
tests/test_tuned_fwd_cpu.py: the two forward kernels of the tuned class (csrc/mlp.hip eval_kernel
and act_kernel, hidden 64, obs <= 32, actions <= 16) behind dppo_old_policy_f32,
dppo_actor_forward_f32, dppo_act_f32, dppo_act_squash_f32 and dppo_prepare_f32, plus three wide
shapes through dppo_old_policy_f32.  Test infrastructure only; NumPy, the oracle and the layout
query, no GPU."""
import math

import numpy as np

from diamond import _native as N
from oracle import ppo_np as P

import wide_act_cases as W
from gpu_helpers import random_params, synth_host

H = 64

# (obs_dim, act_dim, Gaussian head), all at hidden 64
SHAPES = [
    (1, 2, False),    # D = 1, one k-group, per-feature loads, 2-head build
    (2, 3, False),    # D = 2, 4-head build with 3 heads
    (4, 2, False),    # 16-byte loads; lane half 1 is past D in the only k-group
    (5, 3, False),    # D % 4 != 0
    (8, 4, False),    # the headline shape
    (12, 5, False),   # D % 8 == 4: the `D - 4` address in the second k-group; 8-head build with
                      # 5 heads
    (16, 8, False),   # 8-head build, full
    (24, 7, False),   # three k-groups, 16-byte loads
    (28, 9, False),   # D % 8 == 4 in the fourth k-group; 16-head build with 9 heads
    (31, 12, False),  # four k-groups, per-feature loads
    (32, 16, False),  # the ABI limit
    (3, 1, True),     # one action: half a Philox block, 2-head Gaussian build
    (7, 4, True),     # one full Philox block
    (17, 6, True),    # HalfCheetah's shape
    (20, 9, True),    # 16-head Gaussian build; the third Philox block holds one dim
    (32, 16, True),   # the ABI limit
]
# the shapes that also run n = 1, 31 (less than a tile), 32 (one full tile), 71 (a partial third
# tile) and BIG
SIZED = [(8, 4, False), (31, 12, False), (17, 6, True)]
# BIG = 32 * K_WAVES * 2 * CUs + 7.  Both kernels walk 32-sample tiles, one per wave, with a grid
# capped at 2 * CUs workgroups of K_WAVES waves (csrc/mlp.hip: kWaves = kThreads / kWave = 512 / 64,
# launch_eval / launch_act: g > 2 * cus), so this is the smallest size at which a wave loops to a
# second tile; its last tile is partial.  K_WAVES is not visible through the ABI.
K_WAVES = 8
BIG = -1          # stands for the above until real_n() has the device's CU count
MI355X_CUS = W.MI355X_CUS  # the CPU module's stand-in for the device's compute-unit count

# the heads check also runs every first-layer width, at (D, 4, categorical)
SWEEP_A, SWEEP_N = 4, 71
# the alignment checks: the shapes whose rows are a multiple of 4 floats (16-byte loads from a
# 16-byte aligned buffer, per-feature loads from any other) and one shape that never takes them
ALIGN_SHAPES = [s for s in SHAPES if s[0] % 4 == 0] + [(5, 3, False)]
ALIGN_SIZES = (33, 71)
# the wide class sits behind the same dppo_old_policy_f32: (hidden, D, A, Gaussian)
WIDE_SHAPES = [(128, 8, 4, False), (64, 33, 2, False), (128, 105, 8, True)]
WIDE_SIZES = (1, 31, 33, 71)

# (T, N, D, A, Gaussian) of the chained rollouts through dppo_prepare_f32's reuse path: T * N off
# a multiple of 32 and N off a multiple of 4 (but for the HalfCheetah row)
REUSE_CASES = [
    (3, 37, 8, 4, False),
    (5, 13, 12, 5, False),
    (2, 1, 5, 3, False),
    (7, 32, 17, 6, True),
    (9, 33, 32, 16, True),
    (40, 70, 4, 2, False),  # 2,800 samples: the waves' rings fill and drain over several tiles
]

SEED, COUNTER = 0x7E57_F0D5_1CED_C0DE, 23
CLEAR_MARGIN = W.CLEAR_MARGIN


def max_unclear(n):
    """The most samples of a categorical case that may lie within CLEAR_MARGIN of a CDF boundary
    (and so are left out of the draw comparison).  A condition on the inputs."""
    return max(1, math.ceil(n / 100))


def sizes(shape):
    return [33] + ([1, 31, 32, 71, BIG] if shape in SIZED else [])


def real_n(n, cus):
    return 32 * K_WAVES * 2 * cus + 7 if n == BIG else n


def cases(cont=None):
    """(H, D, A, cont, n) of every tuned shape (Gaussian / categorical only when cont is set)"""
    return [(H, *s, n) for s in SHAPES if cont is None or s[2] == cont for n in sizes(s)]


def sweep_cases():
    return [(H, D, SWEEP_A, False, SWEEP_N) for D in range(1, 33)]


def align_cases():
    return [(H, *s, n) for s in ALIGN_SHAPES for n in ALIGN_SIZES]


def wide_cases():
    return [(*s, n) for s in WIDE_SHAPES for n in WIDE_SIZES]


def draw_cases(cont=None):
    """Every tuned (shape, size) whose draws are compared: cases() and align_cases()."""
    out = cases(cont)
    return out + [c for c in align_cases() if c not in out and (cont is None or c[3] == cont)]


case_id = W.case_id
dims = W.dims


def reuse_id(c):
    T, Nn, D, A, cont = c
    return f"T{T}-N{Nn}-D{D}-A{A}-{'gauss' if cont else 'cat'}"


def names_of(cont):
    return P.CONTINUOUS_NAMES if cont else P.DISCRETE_NAMES


def inputs(Hd, D, A, cont, n):
    """(params dict, flat parameters in the library's layout, obs [n][D], next_obs [n][D], actions
    [n] int32 or [n][A]) of one case: the parameters by the shape, the data by the shape and the
    size."""
    L = N.param_layout(dims(Hd, D, A, cont))
    rng = np.random.default_rng(17000 + 1000 * Hd + 10 * D + A)
    params, flat = random_params(L, names_of(cont), D, A, cont, rng)
    rng = np.random.default_rng(19000 + 100 * D + A + 7 * (n % 1000))
    obs = rng.standard_normal((n, D), dtype=np.float32)
    nobs = rng.standard_normal((n, D), dtype=np.float32)
    act = (rng.standard_normal((n, A), dtype=np.float32) if cont
           else rng.integers(0, A, n).astype(np.int32))
    return params, flat, obs, nobs, act


def oracle_eval(params, obs, act, nobs, cont):
    """{output: (float64 oracle, float32 oracle)} of the old-policy evaluation and the heads: the
    float64 restatement is P.forward in float64 plus categorical_logp_entropy /
    normal_logp_entropy in float64, the float32 one P.old_policy."""
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    f = P.forward(p64, obs, cont, np.float64)
    if cont:
        lp64 = P.normal_logp_entropy(f["out"], p64["actor_log_std"], act, np.float64)[0]
    else:
        lp64 = P.categorical_logp_entropy(f["out"], act, np.float64)[0]
    nv64 = P.forward(p64, nobs, cont, np.float64)["v"]
    lp32, v32, nv32, out32 = P.old_policy(params, obs, act, nobs, cont)
    return {"heads": (f["out"], out32), "log_probs": (lp64, lp32), "values": (f["v"], v32),
            "next_values": (nv64, nv32)}


def chained_rollout(T, Nn, D, A, cont):
    """(params, flat, host arrays (obs, next_obs, actions, rewards, term, trunc), keep) of one
    REUSE_CASES row.  The rollout is chained as a vector env chains it: next_obs[t] is obs[t + 1]
    except on the rows of ``keep`` ([T - 1][N], about 3 %: an episode ended there) and in the last
    step."""
    L = N.param_layout(N.Dims(T, Nn, D, A, int(cont), H, 1, 1, 1, 0))
    seed = 1000 * T + 10 * D + A + Nn
    params, flat = random_params(L, names_of(cont), D, A, cont, np.random.default_rng(21000 + seed))
    obs, nobs, act, rew, te, tr = synth_host(T, Nn, D, A, cont, 23000 + seed)
    keep = np.random.default_rng(23001 + seed).random((T - 1, Nn)) < 0.03
    nobs = nobs.copy()
    nobs[:-1] = np.where(keep[..., None], nobs[:-1], obs[1:])
    return params, flat, (obs, nobs, act, rew, te, tr), keep
