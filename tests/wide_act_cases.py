"""Shapes, sizes, seeds and inputs shared by tests/test_gpu_wide_act.py and
tests/test_wide_act_cpu.py (the wide class's fused rollout sampler, csrc/mbwide.hip
wide_act_kernel).  Test infrastructure only; NumPy, the oracle and the layout query, no GPU."""
import numpy as np

from diamond import _native as N
from oracle import ppo_np as P

from gpu_helpers import random_params

M32 = np.uint64(0xFFFFFFFF)

# (hidden, obs_dim, act_dim, Gaussian head)
SHAPES = [
    (128, 8, 4, False),
    (128, 17, 6, True),
    (128, 1, 2, False),     # D = 1: the unaligned first layer
    (128, 30, 1, True),     # one action: a half-used Philox block
    (128, 128, 16, False),  # the largest: five Philox blocks' worth of dims
    (128, 128, 16, True),
    (64, 33, 2, False),
    (64, 105, 8, True),
]
# the shapes that also run n = 1, 31 (less than a tile) and 32 * CUs + 7 (the only size at which a
# workgroup loops to a second tile; its last tile is partial)
SIZED = [(128, 8, 4, False), (64, 105, 8, True)]
BIG = -1          # stands for 32 * CUs + 7 until real_n() has the device's CU count
MI355X_CUS = 256  # the CPU module's stand-in for the device's compute-unit count

SEED, COUNTER = 0x51DE_C0DE_0BAD_CAFE, 41
CLEAR_MARGIN = 1e-4   # |u - CDF boundary| beyond which the discrete draw is decided
MIN_CLEAR = 0.99


def sizes(shape):
    return [33] + ([1, 31, BIG] if shape in SIZED else [])


def real_n(n, cus):
    return 32 * cus + 7 if n == BIG else n


def cases(cont=None):
    """(hidden, D, A, cont, n) of every shape (Gaussian / categorical only when cont is set)"""
    return [(*s, n) for s in SHAPES if cont is None or s[3] == cont for n in sizes(s)]


def case_id(c):
    Hd, D, A, cont, n = c
    return f"H{Hd}-D{D}-A{A}-{'gauss' if cont else 'cat'}-n{'big' if n == BIG else n}"


def dims(Hd, D, A, cont, T=4, Nn=32):
    return N.Dims(T, Nn, D, A, int(cont), Hd, 1, 1, 1, 0)


def inputs(Hd, D, A, cont, n):
    """(params dict, flat parameters in the library's layout, obs [n][D]) of one case"""
    L = N.param_layout(dims(Hd, D, A, cont))
    names = P.CONTINUOUS_NAMES if cont else P.DISCRETE_NAMES
    rng = np.random.default_rng(7000 + 1000 * Hd + 10 * D + A)
    params, flat = random_params(L, names, D, A, cont, rng)
    obs = np.random.default_rng(9000 + D + n % 1000).standard_normal((n, D), dtype=np.float32)
    return params, flat, obs


def categorical_oracle(logits, seed, counter, philox, u01):
    """The documented discrete draw on the oracle's logits: inverse CDF of the float64 softmax at
    u01(c0), the last action taking the remainder.  Returns (actions, clear) with clear = u farther
    than CLEAR_MARGIN from every CDF boundary."""
    out = np.asarray(logits, np.float64)
    n, A = out.shape
    key = (seed & 0xFFFFFFFF, seed >> 32)
    i = np.arange(n, dtype=np.uint64)
    c = philox((i & M32, i >> np.uint64(32), np.full(n, counter & 0xFFFFFFFF),
                np.full(n, counter >> 32)), key)
    u = u01(c[0])
    p = np.exp(out - out.max(1, keepdims=True))
    cdf = np.cumsum(p / p.sum(1, keepdims=True), axis=1)
    want = np.minimum((u[:, None] >= cdf).sum(1), A - 1)
    margin = np.abs(u[:, None] - cdf[:, :-1]).min(1)
    return want, margin > CLEAR_MARGIN
