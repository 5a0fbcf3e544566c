"""GPU parity of every template instantiation of the tuned class's minibatch kernels with their
software pipelines three (and four) groups deep, off-policy.

The sample-split kernel (csrc/mbwave.hip, 10 default instantiations) prefetches indices two
groups ahead and records one group ahead, and carries or re-reads a different set of values per
instantiation; the two-team kernel (csrc/mbstep.hip, 8 instantiations) hands each step from its
forward to its backward team through images double-buffered by step parity.  With one group per
wave / one step per workgroup (m <= 16,384 / 8,192: every shape sweep and every off-policy and
regime test) none of that runs.  Here, for one shape per instantiation (tests/depth_cases.py):

1. dppo_prepare_f32 with the old parameters, dppo_minibatch_grad_f32 with perturbed ones, on a
   stratified minibatch in which each of the five surrogate regimes (gpu_helpers.REGIMES) holds
   at least 5 % of the samples, at m = 33,365 (sample-split: waves 0..37 run three groups, the
   others two, the last group holds 5 samples) or m = 17,573 (two-team: workgroups 0..37 run
   three steps, parity 0, 1, 0, the others two and an empty one); one two-team shape also at
   m = 25,765 (four steps: both parities reused), two cases also with m_total = 2m + 3.  The depth
   is asserted from the library's own plan.  Against the float64 oracle on the kernel's own
   records: overall 2e-5 * max|g| and 4x the float32 oracle's own distance + 1e-6
   (tests/test_gpu_production.py), each tensor 1e-4 of its own scale floored at 1e-3 * max|g|,
   the four loss terms 2e-5 * max(1, |x|) (tests/test_gpu_shapes.py).  The same launch a second
   time gives the same bits: the sums run in a fixed order, so a hand-off race would show.
   tests/test_depth_cpu.py asserts that the float32 oracle is within a quarter of these bounds on
   exactly these inputs.
2. the two-team kernel's <2,*> and <4,*> instantiations, which a default process reaches only
   through the fused Adam tail: the same check in a child process under DPPO_MB_LEGACY=1.
3. the fused Adam tail (DPPO_FUSED_ADAM=1) itself at three steps per workgroup: two learn() calls
   against the oracle's learn (bounds of test_two_learns_with_other_optimiser_settings).

Measured on an MI355X (item 1 and 2; largest overall error / max|g| and largest per-tensor error
/ own scale over the kernel's cases, every case printed by the test):

    kernel                          overall  worst tensor
    sample-split (11 cases)         9.9e-7   1.6e-6
    two-team (6 cases)              1.8e-6   1.8e-6
    two-team <2,*>, <4,*> (4 cases) 4.8e-7   3.5e-6

(the float32 oracle on the same records: 7e-7 .. 4.5e-6 overall).  No kernel change was needed:
every case met its bounds on the first run.

Hand mutations (not committed), each changing only which in-range data is read: with
`f_nxt = fetch(k + 1)` in place of `fetch(k + 2)` in mbwave.hip (a line that runs only in waves
with three or more groups) all 11 sample-split cases fail their overall bound (errors 1.2e-3 ..
3.0e-2 of max|g|) while the rest of this module and tests/test_gpu_shapes.py pass; with the
backward team of mbstep.hip always reading the parity-0 hand-off images all 6 two-team cases
(3.4e-2 .. 0.15), the child-process test and both fused-tail learns fail while the sample-split
cases and tests/test_gpu_shapes.py pass.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diamond
from diamond import _native as N
from oracle import ppo_np as P

import depth_cases as C
import gpu_helpers as G
from conftest import GOLDEN, PKG, ROOT
from gpu_helpers import SpecEnvs, dev, hparams, stream, synth, to_device

_KEYS = ("log_probs", "values", "next_values", "advantages", "returns")


# ---------------------------------------------------------------------------------------------
# 1. one off-policy minibatch gradient per instantiation
# ---------------------------------------------------------------------------------------------
def direct_gradient_check(name, seed, kern, D, A, cont, Nn, m, key, s, scaled, depth):
    """One case of depth_cases.cases() / legacy_cases(); returns (overall, worst tensor) error."""
    T, B = C.T, C.T * Nn
    hy, c = C.inputs(D, A, cont, Nn, m, key, s, seed)
    names = C.names_of(cont)
    idx = c["idx"]
    G.check_offpolicy_conditions(c["regime"][idx], m, c["near"], c["far"])
    h = N.Handle(0, C.dims(D, A, cont, Nn))
    L = h.layout
    # the kernel and the depth this case is about, from the library's own plan
    plan = h.fused_plan(m)
    assert plan["shape_class"] == "tuned" and plan["grid"] == 256, plan
    if kern == "split":
        assert G.sample_split(D, A, cont) and G.production_depth(m, D, A, cont) == depth
        assert (m + 15) // 16 > 2 * 4 * plan["grid"]
    else:
        assert G.nit_of(m) == depth and (m + 31) // 32 > (depth - 1) * plan["grid"]
    hp = hparams(ppo_clip=hy.ppo_clip, value_loss_weight=hy.value_loss_weight,
                 entropy_beta=hy.entropy_beta, advantage_norm=int(hy.advantage_norm))
    ro = to_device(c["host"])
    old_d = torch.from_numpy(c["old_flat"]).to(dev())
    new_d = torch.from_numpy(c["new_flat"]).to(dev())
    outs = {k: torch.empty(B, device=dev()) for k in _KEYS}
    lo = N.LearnOutputs(*[outs[k].data_ptr() for k in _KEYS])
    N.check(h.lib.dppo_prepare_f32(h.h, ctypes.byref(ro.as_struct()), old_d.data_ptr(),
                                   ctypes.byref(hp), ctypes.byref(lo), stream()))
    torch.cuda.synchronize()
    o = {k: v.cpu().numpy() for k, v in outs.items()}
    np.testing.assert_allclose(o["log_probs"], c["logp_old"], rtol=2e-5, atol=2e-5)

    # the regimes still hold on the kernel's own records (its float32 old log-probs move a ratio
    # by a few 1e-5 at most, so half the exclusion band remains)
    logp_new = G.new_policy_logp64(c["new"], c["obs"][idx], c["act"][idx], cont)
    reg, _, _ = G.surrogate_regimes(np.exp(logp_new - o["log_probs"][idx]), o["advantages"][idx],
                                    hy.ppo_clip, near_bound=G.NEAR_BOUND / 2)
    share = G.check_offpolicy_conditions(reg, m, c["near"], c["far"])

    m_total = 2 * m + 3 if scaled else m
    idx_d = torch.from_numpy(idx).to(dev())
    runs = []
    for _ in range(2):
        g = torch.zeros(L.total, device=dev())
        loss4 = (ctypes.c_float * 4)()
        N.check(h.lib.dppo_minibatch_grad_f32(h.h, new_d.data_ptr(), idx_d.data_ptr(), m, m_total,
                                              ctypes.byref(hp), g.data_ptr(), loss4, stream()))
        torch.cuda.synchronize()
        runs.append((g.cpu().numpy(), tuple(loss4)))
    (got, loss4), (again, loss4_again) = runs
    args = (c["obs"][idx], c["act"][idx], o["log_probs"][idx], o["advantages"][idx],
            o["returns"][idx])
    loss, comps, grads = P.minibatch_loss_grads(c["new"], *args, hy, cont, m_total=m_total,
                                                dt=np.float64)
    _, _, g32 = P.minibatch_loss_grads(c["new"], *args, hy, cont, m_total=m_total)
    overall, per = G.gradient_errors(L, names, got, grads)
    oracle32, _ = G.gradient_errors(L, names, G.flat_of(L, names, g32), grads)
    worst = max(per, key=per.get)
    print(f"DEPTH {name}: depth {depth} shares {np.round(share, 3)} overall {overall:.3g} "
          f"(float32 oracle {oracle32:.3g}) worst tensor {per[worst]:.3g} ({worst})")
    assert np.isfinite(got).all()
    assert overall <= 2e-5, overall
    assert overall <= 4 * oracle32 + 1e-6, (overall, oracle32)
    for n in names:
        assert per[n] <= 1e-4, (n, per[n])
    want = (loss, comps["loss_policy"], comps["loss_value"], comps["entropy"])
    for x, y in zip(loss4, want):
        assert abs(x - y) <= 2e-5 * max(1.0, abs(y)), (loss4, want)
    # the same launch again: the same bits
    assert np.array_equal(got, again) and loss4 == loss4_again, \
        (float(np.abs(got - again).max()), loss4, loss4_again)
    h.close()
    return overall, per[worst]


@pytest.mark.parametrize("name,seed,kern,D,A,cont,Nn,m,key,s,scaled,depth", C.cases(),
                         ids=[c[0] for c in C.cases()])
def test_depth_minibatch_gradient_vs_oracle(name, seed, kern, D, A, cont, Nn, m, key, s, scaled,
                                            depth):
    direct_gradient_check(name, seed, kern, D, A, cont, Nn, m, key, s, scaled, depth)


# ---------------------------------------------------------------------------------------------
# 2. the two-team kernel's <2,*> and <4,*> instantiations
# ---------------------------------------------------------------------------------------------
_CHILD = r"""
import sys
sys.path[:0] = {paths!r}
import depth_cases as C
import gpu_helpers as G
from test_gpu_depth import direct_gradient_check
for case in C.legacy_cases():
    assert G.nit_of(case[7]) == 3
    direct_gradient_check(*case)
print("LEGACY-DEPTH-OK", flush=True)
"""


def test_two_team_small_head_instantiations_at_depth():
    """DPPO_MB_LEGACY=1 (read once per process, so set before a fresh one starts) sends every
    tuned shape to the two-team kernel: mb_kernel<2,F>, <2,T>, <4,F> and <4,T> through the check
    of item 1 at three steps per workgroup."""
    env = dict(os.environ, DPPO_MB_LEGACY="1")
    paths = [ROOT, PKG, GOLDEN, os.path.join(ROOT, "tests")]
    r = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "LEGACY-DEPTH-OK" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("DEPTH legacy-team") == len(C.legacy_cases())


# ---------------------------------------------------------------------------------------------
# 3. the fused Adam tail at three steps per workgroup
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,A,cont,norm_clip", [(*s, c) for s, c in zip(C.FUSED_TAIL, (1e3, 0.05))])
def test_fused_tail_learns_at_depth(D, A, cont, norm_clip, monkeypatch):
    """Two consecutive learns under DPPO_FUSED_ADAM=1 (the two-team kernel with the slab
    reduction, clip and Adam as its tail: mb_kernel<4,F> and <2,T>) with minibatches of 17,573
    samples, against the oracle's learn; the handle's timing classes show that the tail ran."""
    monkeypatch.delenv("DPPO_SPLIT_ADAM", raising=False)
    monkeypatch.setenv("DPPO_FUSED_ADAM", "1")
    T, Nn, E, M = C.FUSED_T, C.TEAM_M, C.FUSED_E, C.FUSED_M
    assert T * Nn // M == C.TEAM_M and G.nit_of(T * Nn // M) == 3
    kw = dict(grad_norm_clip=norm_clip, adam_eps=1e-3, gamma=0.9, gae_lambda=0.8, ppo_clip=0.1,
              advantage_norm=False, num_epochs=E, num_minibatches=M)
    Cfg = diamond.ContinuousPPOConfig if cont else diamond.PPOConfig
    Agent = diamond.ContinuousPPO if cont else diamond.PPO
    cfg = Cfg(network_hidden_dim=64, rollout_steps=T, num_envs=Nn, verbose=False, **kw)
    agent = Agent(None, cfg, envs=SpecEnvs(D, A, cont))
    assert agent._learner.fused and agent._learner.shape_class == "tuned"
    names = [n for n, _ in agent.network.named_parameters()]
    params = {n: p.detach().cpu().numpy().copy() for n, p in agent.network.named_parameters()}
    seed = 64 + D + int(norm_clip)
    rollouts = [synth(T, Nn, D, A, cont, seed + k) for k in range(2)]
    np.random.seed(seed)
    st = np.random.get_state()
    agent._learner.handle.set_timing(True)
    traces = []
    for ro, _ in rollouts:
        agent.learn_device(ro)
        traces.append(agent.learn_trace().copy())
    torch.cuda.synchronize()
    tm = agent._learner.handle.timing()
    agent._learner.handle.set_timing(False)
    # one launch per minibatch step, and none of the kernels of the other two Adam paths
    assert tm["grad"][1] == 2 * E * M, tm
    assert tm["reduce_adam"][1] == tm["slab_reduce"][1] == tm["clip_adam"][1] == 0, tm
    np.random.set_state(st)
    adam = P.new_adam_state(params, names)
    hy = P.Hyper(**kw)
    for k, (_, host) in enumerate(rollouts):
        assert adam["step"] == k * E * M
        ref = P.learn(params, adam, list(host), hy, cfg.lr, cont, rng=np.random)
        norms = np.asarray(ref["norm"])
        if norm_clip > 1:   # never clips: coef = min(clip / (norm + 1e-6), 1) == 1
            assert (np.float32(norm_clip) / (norms.astype(np.float32) + np.float32(1e-6)) >= 1).all()
        else:               # always clips
            assert (norms > norm_clip).all(), norms
        print(f"FUSED-TAIL D{D} A{A} learn {k}: loss {traces[k][:, 0]} oracle {ref['loss']} "
              f"norm {traces[k][:, 4]} oracle {ref['norm']}")
        np.testing.assert_allclose(traces[k][:, 0], ref["loss"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(traces[k][:, 4], ref["norm"], rtol=1e-4, atol=1e-5)
    for n, p in agent.network.named_parameters():
        np.testing.assert_allclose(p.detach().cpu().numpy(), params[n], rtol=0, atol=2e-5,
                                   err_msg=n)
