"""Inputs of the GRU minibatch kernel's per-width cases (tests/test_gpu_gru_wide.py;
csrc/grugrad.hip): tests/gru_cases.py's recipe with the weights, the data and hx0 built for a given
G.  gru_hidden_dim 32 and 64 get every case class; 16, whose edge cases are gru_cases.CASES
(tests/test_gpu_gru.py), gets the env-count edges and the long cases only.  Built on the CPU so the clip-regime guards of every case (gru_cases.guards) can be
evaluated with the float64 oracle alone (tests/test_gru_wide_cpu.py) before the kernel runs them.
Test infrastructure only.

A case's ``seed_shift`` moves the seed of its weights and data; it is 0 unless the guards failed
there (a selected sample within 1e-4 of a clip edge, or fewer than 20 % of the samples on one side
of the clip), and tests/test_gru_wide_cpu.py is the proof that the chosen ones hold."""
from dataclasses import dataclass, replace

import gru_cases
from gru_cases import KTAIL_SHAPES, MID, guards  # noqa: F401  (re-exported)

WIDTHS = (32, 64)
# envs per workgroup of the gradient kernel (256 threads, G lanes per env); dppo_gru_plan reports
# the same figures (test_gru_wide_cpu.py::test_envs_per_workgroup)
ENVS_PER_WG = {16: 16, 32: 8, 64: 4}


@dataclass(frozen=True)
class Case(gru_cases.Case):
    G: int = 32

    def __str__(self):
        return f"g{self.G}-{self.name}"


def _edge_shapes(G):
    E = ENVS_PER_WG[G]
    return [(7, n, 5, 3) for n in (E - 1, E, E + 1, 2 * E + 1) if (7, n, 5, 3) not in KTAIL_SHAPES]


def _cases(G):
    x = lambda s: "x".join(map(str, s))
    return (
        [Case(f"ktail-{x(s)}-{f}", s, frac=f, G=G) for s in KTAIL_SHAPES for f in (1.0, 0.4)]
        # a last workgroup of E - 1, 0, 1 envs, and of 1 env behind two full ones
        + [Case(f"envs-{x(s)}", s, G=G) for s in _edge_shapes(G)]
        + [Case(f"hyper-c{c}-v{v}-e{e}-x{k}", MID, clip=c, vf=v, ent=e, m_total_mul=k, G=G)
           for c, v, e in ((0.3, 0.5, 0.0), (0.05, 2.0, 0.05)) for k in (1, 3)]
        + [Case(f"dones-{d}", MID, dones=d, G=G) for d in ("none", "first", "env_always", "last")]
        + [Case("pick-last-step", MID, pick=(MID[0] - 1, 2), dones="none", G=G),
           Case("pick-first-step", MID, pick=(0, 2), dones="none", G=G)]
        + [Case(f"onpolicy-{x(s)}", s, on_policy=True, G=G) for s in (MID, (9, 18, 32, 16))])


# (G, case name) -> seed_shift, where the guards fail at 0
SEED_SHIFT = {(64, "ktail-5x3x4x2-1.0"): 1}   # at 0: 2 of its 15 samples clipped (13 %)

CASES = [replace(c, seed_shift=SEED_SHIFT.get((c.G, c.name), 0)) for G in WIDTHS for c in _cases(G)]

# G = 16: a last workgroup of E - 1, 0 and 1 envs (E + 1 = 17 is in KTAIL_SHAPES, which
# tests/gru_cases.py runs), each off-policy at frac 1.0 and 0.4 and on-policy at 1.0
ENV_EDGE_SHAPES_16 = [(7, 15, 5, 3), (7, 16, 5, 3), (7, 33, 5, 3)]
CASES += ([Case(f"envs-{'x'.join(map(str, s))}-{f}", s, frac=f, G=16)
           for s in ENV_EDGE_SHAPES_16 for f in (1.0, 0.4)]
          + [Case(f"onpolicy-envs-{'x'.join(map(str, s))}", s, on_policy=True, G=16)
             for s in ENV_EDGE_SHAPES_16])


# Sequences of more than one pass and many slabs.  A workgroup holds S = T * ne samples of its
# ne <= ENVS_PER_WG envs and walks them 256 at a time; the gradient slabs are one per workgroup.
# Per G: a full workgroup just past one pass; a full and a partial workgroup past one pass; the
# same at D = 32, A = 16 with a 1-env tail; three passes; the class default (S = 256 exactly at
# G = 32, no thread idle and no second pass); and 1030 envs (129 / 258 slabs, a partial last
# workgroup); at G = 16 S = 256 exactly is (16, 16), and 1030 envs are 65 slabs with a last
# workgroup of 6 envs.  Each runs off-policy at frac 1.0 and 0.4 and on-policy at 1.0; the (40, 15) /
# (72, 7) / (20, 29) shape also with the dones patterns that reset the BPTT carry at every step of one env
# and at the last step of all.
LONG_SHAPES = {
    16: [(17, 16, 5, 3), (20, 29, 5, 3), (20, 17, 32, 16), (35, 16, 4, 2), (16, 16, 4, 2),
         (2, 1030, 5, 3)],
    32: [(33, 8, 5, 3), (40, 15, 5, 3), (40, 17, 32, 16), (70, 9, 4, 2), (32, 32, 4, 2),
         (2, 1030, 5, 3)],
    # (90, 7): at 4 envs per workgroup a partial one needs T >= 86 to pass 256 samples
    64: [(65, 4, 5, 3), (72, 7, 5, 3), (90, 7, 5, 3), (72, 9, 32, 16), (130, 5, 4, 2),
         (32, 32, 4, 2), (2, 1030, 5, 3)],
}
LONG_DONES_SHAPE = {16: (20, 29, 5, 3), 32: (40, 15, 5, 3), 64: (72, 7, 5, 3)}
MANY_ENVS = (2, 1030, 5, 3)     # compared with its first 1024 envs alone (test_gpu_gru_wide.py)
MANY_ENVS_HEAD = 1024


def _long_cases(G):
    x = lambda s: "x".join(map(str, s))
    return (
        [Case(f"long-{x(s)}-{f}", s, frac=f, G=G) for s in LONG_SHAPES[G] for f in (1.0, 0.4)]
        + [Case(f"long-onpolicy-{x(s)}", s, on_policy=True, G=G) for s in LONG_SHAPES[G]]
        + [Case(f"long-dones-{d}-{x(LONG_DONES_SHAPE[G])}", LONG_DONES_SHAPE[G], dones=d, G=G)
           for d in ("env_always", "last")])


# at 0: a ratio 7e-5 / 3e-5 from a clip edge
SEED_SHIFT.update({(32, "long-70x9x4x2-1.0"): 1, (64, "long-90x7x5x3-1.0"): 1})

LONG_CASES = [replace(c, seed_shift=SEED_SHIFT.get((c.G, c.name), 0))
              for G in WIDTHS + (16,) for c in _long_cases(G)]


def workgroups(case):
    """[(envs, samples S)] of the gradient kernel's workgroups on one case."""
    T, Nn = case.shape[:2]
    E = ENVS_PER_WG[case.G]
    return [(min(E, Nn - lo), T * min(E, Nn - lo)) for lo in range(0, Nn, E)]


def config(G, **kw):
    from diamond.recurrent_ppo import RecurrentPPOConfig
    return RecurrentPPOConfig(gru_hidden_dim=G, **kw)


def initial_params(D, A, G, seed=42):
    """RecurrentPPO's initial weights for RecurrentPPOConfig(gru_hidden_dim=G, seed=seed), built
    on the CPU."""
    return gru_cases.initial_params(D, A, seed, G=G)


def data(T, Nn, D, A, G, seed):
    return gru_cases.data(T, Nn, D, A, seed, G=G)


def build(case):
    """(params, data dict, mb_idx int32, m_total) of one case: gru_cases.build at case.G, regime
    fields (tests/regime_cases.py) included."""
    assert case.G in ENVS_PER_WG
    return gru_cases.build(case)
