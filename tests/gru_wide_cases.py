"""Inputs of the wide GRU minibatch kernel's cases (tests/test_gpu_gru_wide.py; csrc/gruwide.hip,
gru_hidden_dim 32 and 64): tests/gru_cases.py's recipe with the weights, the data and hx0 built for
a given G.  Built on the CPU so the clip-regime guards of every case (gru_cases.guards) can be
evaluated with the float64 oracle alone (tests/test_gru_wide_cpu.py) before the kernel runs them.
Test infrastructure only.

A case's ``seed_shift`` moves the seed of its weights and data; it is 0 unless the guards failed
there (a selected sample within 1e-4 of a clip edge, or fewer than 20 % of the samples on one side
of the clip), and tests/test_gru_wide_cpu.py is the proof that the chosen ones hold."""
from dataclasses import dataclass, replace
from math import sqrt

import numpy as np
import torch

import gru_cases
from gru_cases import KTAIL_SHAPES, MID, guards  # noqa: F401  (re-exported)
from oracle import gru_torch as GT

WIDTHS = (32, 64)
# envs per workgroup of the gradient kernel (256 threads, G lanes per env); dppo_gru_plan reports
# the same figures (test_gru_wide_cpu.py::test_envs_per_workgroup)
ENVS_PER_WG = {32: 8, 64: 4}


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


def config(G, **kw):
    from diamond.recurrent_ppo import RecurrentPPOConfig
    return RecurrentPPOConfig(gru_hidden_dim=G, **kw)


def initial_params(D, A, G, seed=42):
    """RecurrentPPO's initial weights for RecurrentPPOConfig(gru_hidden_dim=G, seed=seed), built
    on the CPU."""
    import gym_stub
    from diamond.recurrent_ppo import RecurrentActorCriticNetwork, network_parameter_init_
    torch.manual_seed(seed)
    net = RecurrentActorCriticNetwork(gym_stub.Box(shape=(D,)), gym_stub.Discrete(A),
                                      cfg=config(G))
    network_parameter_init_(net, gain=sqrt(2.0))
    p = {n: t.detach().numpy().copy() for n, t in net.named_parameters()}
    assert list(p) == GT.GRU_NAMES
    return p


def data(T, Nn, D, A, G, seed):
    rng = np.random.default_rng(seed)
    return dict(obs=rng.standard_normal((T, Nn, D)).astype(np.float32),
                actions=rng.integers(0, A, (T, Nn)).astype(np.int32),
                old_log_probs=(-rng.uniform(0.2, 1.5, (T, Nn))).astype(np.float32),
                advantages=rng.standard_normal((T, Nn)).astype(np.float32),
                returns=rng.standard_normal((T, Nn)).astype(np.float32),
                prev_dones=(rng.random((T, Nn)) < 0.08),
                hx0=(rng.standard_normal((Nn, G)) * 0.5).astype(np.float32))


def build(case):
    """(params, data dict, mb_idx int32, m_total) of one case: gru_cases.build at case.G."""
    T, Nn, D, A = case.shape
    seed = T * 100 + Nn + case.seed_shift
    rng = np.random.default_rng(seed + 1)
    params = {n: (p + 0.3 * rng.standard_normal(p.shape)).astype(np.float32)
              for n, p in initial_params(D, A, case.G).items()}
    x = data(T, Nn, D, A, case.G, seed)
    pd = x["prev_dones"]
    if case.dones == "none":
        pd[:] = False
    elif case.dones == "first":
        pd[0] = True
    elif case.dones == "env_always":
        pd[:, gru_cases.DONE_ENV] = True
    elif case.dones == "last":
        pd[:] = False
        pd[T - 1] = True
    else:
        assert case.dones == "random"
    if case.on_policy:
        lp = GT.log_probs(params, x["obs"], x["actions"], pd, x["hx0"])
        x["old_log_probs"] = lp.astype(np.float32)
    B = T * Nn
    if case.pick is not None:
        mb_idx = np.array([case.pick[0] * Nn + case.pick[1]], np.int32)
    else:
        m = max(1, int(B * case.frac))
        mb_idx = np.random.default_rng(7).permutation(B)[:m].astype(np.int32)
    return params, x, mb_idx, case.m_total_mul * len(mb_idx)
