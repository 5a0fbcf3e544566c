"""Shapes, sizes, seeds and inputs shared by tests/test_gpu_depth.py and tests/test_depth_cpu.py:
one off-policy minibatch per template instantiation of the tuned class's two minibatch kernels,
at the smallest sizes at which their software pipelines run three (and, for one shape, four)
groups deep.

* sample-split kernel (csrc/mbwave.hip, mbw_kernel<AMAX, CONT, NIB[, X1]>): min(ceil(m/64), 256)
  workgroups of 4 waves, wave `first = 4 * block + wave` runs the 16-sample groups
  first + k * 1024.  SPLIT_M = 2 * 16384 + 16 * 37 + 5 is 2,086 groups: waves 0..37 run three,
  the others two, workgroup 9 holds waves of both counts, and the last group (5 samples) is wave
  37's third.
* two-team kernel (csrc/mbstep.hip, mb_kernel<AMAX, CONT>): min(ceil(m/32), 256) workgroups,
  workgroup g runs the 32-sample steps g + it * 256.  TEAM_M = 2 * 8192 + 32 * 37 + 5 is 550
  steps: workgroups 0..37 run three (hand-off parity 0, 1, 0), the others two and an empty one,
  and the last step holds 5 samples.  TEAM_M4 = 3 * 8192 + 32 * 37 + 5 is 806 steps, four deep.

Test infrastructure only; NumPy, the oracle and the layout query, no GPU."""
import functools

from diamond import _native as N
from oracle import ppo_np as P

import gpu_helpers as G

H, T, E, M = 64, 16, 1, 2

SPLIT_M, SPLIT_N = 2 * 16384 + 16 * 37 + 5, 4172    # B = 66,752 >= 2 m
TEAM_M, TEAM_N = 2 * 8192 + 32 * 37 + 5, 2200       # B = 35,200 >= 2 m
TEAM_M4, TEAM_N4 = 3 * 8192 + 32 * 37 + 5, 3221     # B = 51,536 >= 2 m

# (kernel, D, A, Gaussian head, instantiation, hyper set, noise scale s); seed 500 + row
SHAPES = [
    ("split", 4, 2, False, "<2,F,1>", "clip.1", 0.2),
    ("split", 3, 1, True, "<2,T,1>", "clip.1", 0.05),
    ("split", 8, 4, False, "<4,F,1>", "clip.3", 0.2),
    ("split", 11, 4, True, "<4,T,1>", "clip.1", 0.03),
    ("split", 20, 2, False, "<2,F,2>", "clip.1", 0.2),
    ("split", 24, 2, True, "<2,T,2>", "clip.3", 0.03),
    ("split", 20, 3, False, "<4,F,2>", "clip.3", 0.2),
    ("split", 32, 4, True, "<4,T,2>", "clip.1", 0.03),
    ("split", 16, 8, False, "<8,F,1>", "clip.1", 0.2),
    ("split", 17, 6, True, "<6,T,2,X1>", "clip.3", 0.03),
    ("team", 20, 7, False, "<8,F>", "clip.3", 0.2),     # D16 = 32
    ("team", 5, 8, True, "<8,T>", "clip.1", 0.03),      # D16 = 16
    ("team", 32, 16, False, "<16,F>", "clip.1", 0.2),
    ("team", 5, 10, True, "<16,T>", "clip.3", 0.03),
]
DEEPER = ("team", 20, 7, False)                    # the shape that also runs TEAM_M4
MTOTAL = [("split", 8, 4, False), ("team", 5, 10, True)]   # ... and m_total = 2 m + 3
# the shapes of the two-team kernel's <2,*> and <4,*> instantiations (DPPO_MB_LEGACY=1 sends them
# there); inputs of the sample-split rows of the same shape, at the two-team size
LEGACY = [(4, 2, False), (3, 1, True), (8, 4, False), (11, 4, True)]
# learn() under DPPO_FUSED_ADAM=1: (D, A, Gaussian head), T = 2, N = TEAM_M, E = 1, M = 2
FUSED_TAIL = [(8, 4, False), (3, 1, True)]
FUSED_T, FUSED_E, FUSED_M = 2, 1, 2

SPLIT_INSTANTIATIONS = {"<2,F,1>", "<2,T,1>", "<4,F,1>", "<4,T,1>", "<2,F,2>", "<2,T,2>",
                        "<4,F,2>", "<4,T,2>", "<8,F,1>", "<6,T,2,X1>"}
TEAM_INSTANTIATIONS = {"<8,F>", "<8,T>", "<16,F>", "<16,T>"}


def instantiation(kernel, D, A, cont):
    """The template arguments launch_mbw (csrc/mbwave.hip) / launch_mb (csrc/mbstep.hip) pick."""
    c = "T" if cont else "F"
    if kernel == "team":
        return f"<{2 if A <= 2 else 4 if A <= 4 else 8 if A <= 8 else 16},{c}>"
    if A > 4 and cont:
        return "<6,T,2,X1>" if D == 17 else "<6,T,2>"
    return f"<{2 if A <= 2 else 4 if A <= 4 else 8},{c},{2 if D > 16 else 1}>"


def cases():
    """(id, seed, kernel, D, A, cont, Nn, m, hyper key, s, m_total is 2m + 3, depth)"""
    out = []
    for row, (kern, D, A, cont, _, key, s) in enumerate(SHAPES):
        Nn, m = (SPLIT_N, SPLIT_M) if kern == "split" else (TEAM_N, TEAM_M)
        name = f"{kern}-D{D}-A{A}-{'gauss' if cont else 'cat'}-{key}"
        out.append((name, 500 + row, kern, D, A, cont, Nn, m, key, s, False, 3))
        if (kern, D, A, cont) in MTOTAL:
            out.append((name + "-mtotal", 500 + row, kern, D, A, cont, Nn, m, key, s, True, 3))
    row = [s[:4] for s in SHAPES].index(DEEPER)
    kern, D, A, cont, _, key, s = SHAPES[row]
    out.append((f"{kern}-D{D}-A{A}-{'gauss' if cont else 'cat'}-{key}-nit4", 500 + len(SHAPES),
                kern, D, A, cont, TEAM_N4, TEAM_M4, key, s, False, 4))
    return out


def legacy_cases():
    """The LEGACY shapes as two-team cases: seed, hyper set and noise of their sample-split row."""
    out = []
    for D, A, cont in LEGACY:
        row = [s[:4] for s in SHAPES].index(("split", D, A, cont))
        key, s = SHAPES[row][5:]
        name = f"legacy-team-D{D}-A{A}-{'gauss' if cont else 'cat'}-{key}"
        out.append((name, 500 + row, "team", D, A, cont, TEAM_N, TEAM_M, key, s, False, 3))
    return out


def dims(D, A, cont, Nn):
    return N.Dims(T, Nn, D, A, int(cont), H, E, M, 1, 0)


def names_of(cont):
    return P.CONTINUOUS_NAMES if cont else P.DISCRETE_NAMES


@functools.lru_cache(maxsize=2)
def inputs(D, A, cont, Nn, m, key, s, seed):
    """(hyper, gpu_helpers.offpolicy_inputs(...)) of one case: shared by a shape's m_total == m
    and m_total != m cases, never modified.  (Two entries: a case's inputs are ~10 MB.)"""
    hy = G.offpolicy_hyper(key)
    L = N.param_layout(dims(D, A, cont, Nn))
    return hy, G.offpolicy_inputs(L, names_of(cont), D, A, cont, T, Nn, m, hy, s, seed)


def wave_groups(m):
    """Groups each of the sample-split kernel's waves runs (mbwave.hip: first, stride, nk), and
    the (wave, k, samples) of the last group."""
    ngroups = (m + 15) // 16
    stride = 4 * min((m + 63) // 64, 256)
    nk = [(ngroups - w + stride - 1) // stride if w < ngroups else 0 for w in range(stride)]
    last = ngroups - 1
    return nk, (last % stride, last // stride, m - 16 * last)


def workgroup_steps(m):
    """Live steps of each of the two-team kernel's workgroups (mbstep.hip: step = it * G + g,
    live where step * 32 < m), steps per workgroup (nit), and the (workgroup, it, samples) of the
    last step."""
    nsteps = (m + 31) // 32
    Gd = min(nsteps, 256)
    nit = (nsteps + Gd - 1) // Gd
    live = [sum(1 for it in range(nit) if (it * Gd + g) * 32 < m) for g in range(Gd)]
    last = nsteps - 1
    return live, nit, (last % Gd, last // Gd, m - 32 * last)
