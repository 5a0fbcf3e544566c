"""The inputs of tests/test_gpu_offpolicy.py, checked without a GPU.

gpu_helpers.offpolicy_inputs draws old parameters, perturbs them into new ones and picks a
stratified minibatch so that every branch of the clipped surrogate (reference ppo.py:266-270)
carries samples.  For every shape and hyper-parameter set of the GPU module this asserts

* the conditions that keep the GPU check from being vacuous: the samples excluded (ratio within
  1e-3 of a clip bound, or outside [1/16, 16]) are at most 5 % of the batch, the minibatch is
  full, holds no excluded sample, and every one of the five regimes holds at least 5 % of it;
* that the float32 oracle, on exactly those inputs, stays inside the GPU module's bounds against
  the float64 oracle (overall 2e-5 * max|g|, each tensor 1e-4 of its own scale floored at
  1e-3 * max|g|, the four loss terms 2e-5 * max(1, |x|)): the bounds are met by a correct
  float32 implementation, so a kernel that misses them is wrong.

Largest float32-oracle errors over the cases: overall 2.0e-6 * max|g|, per tensor 6.6e-6 of the
tensor's scale.
"""
import numpy as np
import pytest

from diamond import _native as N
from oracle import ppo_np as P

import gpu_helpers as G


def build_case(Hd, D, A, cont, Nn, key, s, seed):
    T, M = G.OFFPOLICY_T, G.OFFPOLICY_M
    m = T * Nn // M - G.OFFPOLICY_RAGGED
    L = N.param_layout(N.Dims(T, Nn, D, A, int(cont), Hd, 4, M, 1, 0))
    names = P.CONTINUOUS_NAMES if cont else P.DISCRETE_NAMES
    hy = G.offpolicy_hyper(key)
    return L, names, hy, m, G.offpolicy_inputs(L, names, D, A, cont, T, Nn, m, hy, s, seed)


@pytest.mark.parametrize("name,seed,fam,Hd,D,A,cont,Nn,key,s,scaled", G.offpolicy_cases(),
                         ids=[c[0] for c in G.offpolicy_cases()])
def test_offpolicy_inputs_and_float32_oracle(name, seed, fam, Hd, D, A, cont, Nn, key, s, scaled):
    L, names, hy, m, c = build_case(Hd, D, A, cont, Nn, key, s, seed)
    idx = c["idx"]
    assert len(np.unique(idx)) == m and m % 16 != 0 and m % 32 != 0
    share = G.check_offpolicy_conditions(c["regime"][idx], m, c["near"], c["far"])
    # the labels mean what they say: the surrogate's own branches, from the oracle's formulas
    r, a, eps = c["ratio"][idx], c["adv"][idx].astype(np.float64), hy.ppo_clip
    u, w = -a * r, -a * np.clip(r, 1 - eps, 1 + eps)
    reg = c["regime"][idx]
    assert (u[reg == 0] == w[reg == 0]).all()
    assert (w[(reg == 1) | (reg == 4)] >= u[(reg == 1) | (reg == 4)]).all()   # clipped term wins
    assert (u[(reg == 2) | (reg == 3)] >= w[(reg == 2) | (reg == 3)]).all()   # unclipped wins
    m_total = 2 * m + 3 if scaled else m
    args = (c["new"], c["obs"][idx], c["act"][idx], c["logp_old"][idx], c["adv"][idx],
            c["ret"][idx], hy, cont)
    l32, c32, g32 = P.minibatch_loss_grads(*args, m_total=m_total)
    l64, c64, g64 = P.minibatch_loss_grads(*args, m_total=m_total, dt=np.float64)
    overall, per = G.gradient_errors(L, names, G.flat_of(L, names, g32), g64)
    print(f"{name}: shares {np.round(share, 3)} near {c['near']:.4f} far {c['far']:.4f} "
          f"f32 oracle overall {overall:.3g} worst tensor {max(per.values()):.3g}")
    assert overall <= 2e-5, overall
    assert max(per.values()) <= 1e-4, per
    for x32, x64 in [(l32, l64)] + [(c32[k], c64[k]) for k in c64]:
        assert abs(x32 - x64) <= 2e-5 * max(1.0, abs(x64)), (x32, x64)
    if scaled:
        # the divisor only scales: gradients and loss terms by m / m_total
        _, c1, g1 = P.minibatch_loss_grads(*args, dt=np.float64)
        k = m / m_total
        for n in names:
            if n == "actor_log_std":   # its entropy term is -beta whatever the divisor
                np.testing.assert_allclose(g64[n] + hy.entropy_beta,
                                           k * (g1[n] + hy.entropy_beta), rtol=1e-12, atol=1e-15)
            else:
                np.testing.assert_allclose(g64[n], k * g1[n], rtol=1e-12, atol=1e-15, err_msg=n)
        for key_ in c1:
            assert abs(c64[key_] - k * c1[key_]) <= 1e-12 * max(1.0, abs(c1[key_]))


def test_every_family_and_head_is_listed():
    """The table keeps one shape per kernel family and head path, both hyper-parameter sets, and
    an m_total != m case for one categorical and one Gaussian head per family."""
    shapes = {(s[1], s[2], s[3], s[4]) for s in G.OFFPOLICY_SHAPES}
    assert shapes >= {(64, 8, 4, False), (64, 3, 1, True), (64, 16, 8, False), (64, 17, 6, True),
                      (64, 32, 16, False), (64, 5, 10, True), (128, 8, 4, False),
                      (128, 105, 8, True), (128, 128, 16, False), (128, 30, 1, True),
                      (64, 40, 5, False), (64, 128, 16, True)}
    cases = G.offpolicy_cases()
    for s in G.OFFPOLICY_SHAPES:
        keys = {c[8] for c in cases if (c[3], c[4], c[5], c[6]) == (s[1], s[2], s[3], s[4])}
        assert keys == set(G.OFFPOLICY_HYPER)
    for fam in ("sample-split", "two-team", "wide"):
        assert {c[6] for c in cases if c[2] == fam and c[10]} == {False, True}, fam
    a, b = (G.OFFPOLICY_HYPER[k] for k in ("clip.1", "clip.3"))
    assert (a["ppo_clip"], a["value_loss_weight"], a["entropy_beta"], a["advantage_norm"]) == \
        (0.1, 0.5, 0.05, False)
    assert (b["ppo_clip"], b["value_loss_weight"], b["entropy_beta"], b["advantage_norm"]) == \
        (0.3, 2.0, 0.0, True)
