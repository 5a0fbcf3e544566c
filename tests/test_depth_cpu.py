"""The cases of tests/test_gpu_depth.py (tests/depth_cases.py), checked without a GPU.

For every case -- one shape per template instantiation of the tuned class's two minibatch
kernels, at sizes at which each wave / workgroup runs three or four groups -- this asserts

* the conditions of tests/test_offpolicy_inputs_cpu.py: a full stratified minibatch without
  excluded samples, every surrogate regime with at least 5 % of it;
* the depth the case is about, from gpu_helpers.production_depth and from a plain restatement of
  the kernels' group-to-wave / step-to-workgroup maps: how many waves run three groups and how
  many two, how many workgroups have three live steps, and where the 5-sample group sits;
* the seed condition: on exactly these inputs the float32 oracle is within a QUARTER of each of
  the GPU module's bounds against the float64 oracle (overall 5e-6 of max|g|, each tensor 2.5e-5
  of its own scale, the loss terms 5e-6 * max(1, |x|)), so that the GPU bounds measure the kernel
  and not the draw.  A seed that misses is replaced; the bound is not.
* that every default instantiation (10 sample-split, 4 two-team) has a row.

Largest float32-oracle errors over the cases: overall 4.8e-6 * max|g|, per tensor 7.5e-6 of the
tensor's scale.
"""
import numpy as np
import pytest

from diamond import _native as N
from oracle import ppo_np as P

import depth_cases as C
import gpu_helpers as G

_ALL = C.cases() + C.legacy_cases()


@pytest.mark.parametrize("name,seed,kern,D,A,cont,Nn,m,key,s,scaled,depth", _ALL,
                         ids=[c[0] for c in _ALL])
def test_depth_case_inputs_and_float32_oracle(name, seed, kern, D, A, cont, Nn, m, key, s, scaled,
                                              depth):
    hy, c = C.inputs(D, A, cont, Nn, m, key, s, seed)
    L = N.param_layout(C.dims(D, A, cont, Nn))
    names = C.names_of(cont)
    idx = c["idx"]
    assert C.T * Nn >= 2 * m and m <= C.T * Nn // C.M
    # the last 16-sample group holds 5 samples; so does the two-team kernel's last 32-sample step
    # (SPLIT_M % 32 is 21: 37 groups past a multiple of 32 samples)
    assert len(np.unique(idx)) == m and m % 16 == 5 and m % 32 == (21 if kern == "split" else 5)
    share = G.check_offpolicy_conditions(c["regime"][idx], m, c["near"], c["far"])
    # the labels mean what they say: the surrogate's own branches, from the oracle's formulas
    r, a, eps = c["ratio"][idx], c["adv"][idx].astype(np.float64), hy.ppo_clip
    u, w = -a * r, -a * np.clip(r, 1 - eps, 1 + eps)
    reg = c["regime"][idx]
    assert (u[reg == 0] == w[reg == 0]).all()
    assert (w[(reg == 1) | (reg == 4)] >= u[(reg == 1) | (reg == 4)]).all()   # clipped term wins
    assert (u[(reg == 2) | (reg == 3)] >= w[(reg == 2) | (reg == 3)]).all()   # unclipped wins

    # the depth: by the library's own rule for a default process, and by the kernels' maps
    legacy = name.startswith("legacy")
    assert G.sample_split(D, A, cont) == (kern == "split" or legacy)
    if not legacy:
        assert G.production_depth(m, D, A, cont) == depth
    if kern == "split":
        assert G.groups_per_wave(m) == depth == 3
        nk, (wave, k, left) = C.wave_groups(m)
        assert len(nk) == 1024 and sum(nk) == 2086
        assert nk[:38] == [3] * 38 and nk[38:] == [2] * 986
        assert sorted(set(nk[4 * 9:4 * 10])) == [2, 3]     # workgroup 9: waves 36..39
        assert (wave, k, left) == (37, 2, 5)
    else:
        assert G.nit_of(m) == depth
        live, nit, (wg, it, left) = C.workgroup_steps(m)
        assert len(live) == 256 and nit == depth
        assert sum(live) == (550 if depth == 3 else 806)
        assert live[:38] == [depth] * 38 and live[38:] == [depth - 1] * 218
        assert (wg, it, left) == (37, depth - 1, 5)
        # parity of the hand-off images over a workgroup's steps: 0, 1, 0 (and 1: both reused)
        assert [i & 1 for i in range(nit)] == ([0, 1, 0] if depth == 3 else [0, 1, 0, 1])

    m_total = 2 * m + 3 if scaled else m
    args = (c["new"], c["obs"][idx], c["act"][idx], c["logp_old"][idx], c["adv"][idx],
            c["ret"][idx], hy, cont)
    l32, c32, g32 = P.minibatch_loss_grads(*args, m_total=m_total)
    l64, c64, g64 = P.minibatch_loss_grads(*args, m_total=m_total, dt=np.float64)
    overall, per = G.gradient_errors(L, names, G.flat_of(L, names, g32), g64)
    print(f"{name}: shares {np.round(share, 3)} near {c['near']:.4f} far {c['far']:.4f} "
          f"f32 oracle overall {overall:.3g} worst tensor {max(per.values()):.3g}")
    assert overall <= 2e-5 / 4, overall
    assert max(per.values()) <= 1e-4 / 4, per
    for x32, x64 in [(l32, l64)] + [(c32[k], c64[k]) for k in c64]:
        assert abs(x32 - x64) <= 2e-5 / 4 * max(1.0, abs(x64)), (x32, x64)


def test_every_instantiation_is_listed():
    """One row per default instantiation of both kernels, each labelled with what the launchers
    pick for its shape; both heads and both hyper-parameter sets per kernel; the four-deep size;
    one categorical and one Gaussian m_total != m case; the <2,*> / <4,*> two-team shapes."""
    rows = {k: [s for s in C.SHAPES if s[0] == k] for k in ("split", "team")}
    for kern, D, A, cont, inst, key, _ in C.SHAPES:
        assert C.instantiation(kern, D, A, cont) == inst, (kern, D, A, cont)
        assert G.sample_split(D, A, cont) == (kern == "split")
        assert 1 <= D <= 32 and 1 <= A <= 16 and key in G.OFFPOLICY_HYPER
    assert sorted(s[4] for s in rows["split"]) == sorted(C.SPLIT_INSTANTIATIONS)
    assert sorted(s[4] for s in rows["team"]) == sorted(C.TEAM_INSTANTIATIONS)
    assert len(C.SPLIT_INSTANTIATIONS) == 10 and len(C.TEAM_INSTANTIATIONS) == 4
    # the two-team kernel's layer 1 has a 16- and a 32-input build
    assert {(s[1] + 15) // 16 for s in rows["team"] if s[4].startswith("<8")} == {1, 2}
    for kern in rows:
        assert {s[3] for s in rows[kern]} == {False, True}
        assert {s[5] for s in rows[kern]} == set(G.OFFPOLICY_HYPER)
    cases = C.cases()
    assert len(cases) == 17 and len({c[0] for c in cases}) == 17
    assert [c[2:6] for c in cases if c[11] == 4] == [C.DEEPER]
    assert sorted(c[5] for c in cases if c[10]) == [False, True]
    assert (C.SPLIT_M, C.TEAM_M, C.TEAM_M4) == (33365, 17573, 25765)
    assert {C.instantiation("team", *s) for s in C.LEGACY} == {"<2,F>", "<2,T>", "<4,F>", "<4,T>"}
    assert all(G.sample_split(*s) for s in C.LEGACY + C.FUSED_TAIL)
    assert {C.instantiation("team", *s) for s in C.FUSED_TAIL} == {"<4,F>", "<2,T>"}
    assert G.nit_of(C.FUSED_T * C.TEAM_M // C.FUSED_M) == 3
