"""GPU parity of the fused kernels off-policy and away from the default hyper-parameters.

Every other gradient test evaluates the minibatch gradient at the parameters that produced the old
log-probs (ratio 1 +- 1e-7: only the u == w tie of the clipped surrogate runs) and with one
hyper-parameter set (clip 0.2, value weight 1, entropy 0.01, advantage_norm, m_total == m).  Here:

1. off-policy minibatch gradients (dppo_prepare_f32 with old parameters, dppo_minibatch_grad_f32
   with perturbed ones) against the float64 oracle (reference ppo.py:261-283,
   continuous_ppo.py:273-295), on a stratified minibatch in which each of the five surrogate
   regimes (gpu_helpers.REGIMES) holds at least 5 % of the samples, for one shape per kernel
   family and head path, two hyper-parameter sets (gpu_helpers.OFFPOLICY_HYPER) and
   m_total = 2m + 3.  Bounds of tests/test_gpu_shapes.py: overall 2e-5 * max|g|, each tensor 1e-4
   of its own scale (floored at 1e-3 * max|g|), all four loss terms 2e-5 * max(1, |x|).
   tests/test_offpolicy_inputs_cpu.py asserts the same conditions on the inputs and that the
   float32 oracle meets these bounds.
2. dppo_gae_f32 at (gamma, lambda) other than (0.99, 0.95): bit-exact in exact mode, within
   test_gae_affine_mode_within_tolerance's bound in affine mode.
3. whole learn() calls with a gradient-norm clip that never / always clips, adam_eps 1e-3,
   gamma 0.9, lambda 0.8, clip 0.1 and no advantage normalisation, twice in a row, against the
   oracle's learn (bounds of test_wide_learn_vs_oracle).
4. dppo_clip_adam_f32 on its own against the oracle's clip_grad_norm + adam_step.

Measured on an MI355X (item 1; largest overall error / max|g| and largest per-tensor error / own
scale over the family's cases, every case printed by the test):

    family        noise scale s                                  overall  worst tensor
    sample-split  0.2 categorical; Gaussian 0.03, 0.05-0.08 (A=1)  2.1e-6   2.8e-6
    two-team      0.2 categorical; Gaussian 0.03                   1.6e-6   2.6e-6
    wide          0.2 categorical; Gaussian 0.02-0.05, 0.1 (A=1)   3.4e-6   5.3e-6

(the wide family's ten rows are one per reachable wide_mb_kernel<H, CONT, NB1>,
tests/wide_mb_cases.py)

Hand mutations of the three minibatch kernels (not committed): with `inr` replaced by 1.0f every
item-1 case fails its overall bound (errors 6e-3 .. 0.7 of max|g|) while every gradient test that
existed before still passes; with `u > w` turned into `u >= w` every item-1 case fails, and so do
the earlier gradient tests (in-range samples tie, u == w, and then count 1.5 times).

Found by item 2: dppo_gae_f32 multiplied the widened C floats gamma and lambda, which rounds to
another float32 than the reference's double product for about a third of the (gamma, lambda)
pairs (0.9 * 0.8 among them, not the default pair); see DESIGN.md.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diamond
from diamond import _native as N
from oracle import ppo_np as P

import gpu_helpers as G
from gpu_helpers import SpecEnvs, dev, hparams, sample_split, stream, synth, to_device

_KEYS = ("log_probs", "values", "next_values", "advantages", "returns")


# ---------------------------------------------------------------------------------------------
# 1. off-policy minibatch gradient
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(Hd, D, A, cont, Nn, key, s, seed):
    """The CPU half (shared by a shape's m_total == m and m_total != m cases; never modified)."""
    T, M = G.OFFPOLICY_T, G.OFFPOLICY_M
    m = T * Nn // M - G.OFFPOLICY_RAGGED
    L = N.param_layout(N.Dims(T, Nn, D, A, int(cont), Hd, 4, M, 1, 0))
    names = P.CONTINUOUS_NAMES if cont else P.DISCRETE_NAMES
    hy = G.offpolicy_hyper(key)
    return names, hy, m, G.offpolicy_inputs(L, names, D, A, cont, T, Nn, m, hy, s, seed)


@pytest.mark.parametrize("name,seed,fam,Hd,D,A,cont,Nn,key,s,scaled", G.offpolicy_cases(),
                         ids=[c[0] for c in G.offpolicy_cases()])
def test_offpolicy_minibatch_gradient_vs_oracle(name, seed, fam, Hd, D, A, cont, Nn, key, s,
                                                scaled):
    T, M = G.OFFPOLICY_T, G.OFFPOLICY_M
    B = T * Nn
    names, hy, m, c = _inputs(Hd, D, A, cont, Nn, key, s, seed)
    idx = c["idx"]
    G.check_offpolicy_conditions(c["regime"][idx], m, c["near"], c["far"])
    h = N.Handle(0, N.Dims(T, Nn, D, A, int(cont), Hd, 4, M, 1, 0))
    L = h.layout
    # the kernel family this case is about
    plan = h.fused_plan(m)
    if fam == "wide":
        assert plan["shape_class"] == "wide"
        assert m % plan["tile"] != 0 and m > plan["tile"]
    else:
        assert plan["shape_class"] == "tuned" and Hd == 64
        assert sample_split(D, A, cont) == (fam == "sample-split")
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

    # records: old log-probs of the OLD parameters, raw GAE under advantage_norm = 0
    obs, nobs, act, rew, te, tr = c["host"]
    np.testing.assert_allclose(o["log_probs"], c["logp_old"], rtol=2e-5, atol=2e-5)
    vals, nvals = o["values"].reshape(T, Nn), o["next_values"].reshape(T, Nn)
    raw = P.gae(rew, te, tr, vals, nvals, hy.gamma, hy.gae_lambda)
    assert np.array_equal(o["returns"].reshape(T, Nn), vals + raw)
    if hy.advantage_norm:
        np.testing.assert_allclose(o["advantages"], P.normalize_adv(raw).ravel(), rtol=0,
                                   atol=2e-6)
    else:
        assert np.array_equal(o["advantages"], raw.ravel())

    # the regimes still hold on the kernel's own records (its float32 old log-probs move a ratio
    # by a few 1e-5 at most, so half the exclusion band remains)
    logp_new = G.new_policy_logp64(c["new"], c["obs"][idx], c["act"][idx], cont)
    reg, _, _ = G.surrogate_regimes(np.exp(logp_new - o["log_probs"][idx]), o["advantages"][idx],
                                    hy.ppo_clip, near_bound=G.NEAR_BOUND / 2)
    share = G.check_offpolicy_conditions(reg, m, c["near"], c["far"])

    m_total = 2 * m + 3 if scaled else m
    idx_d = torch.from_numpy(idx).to(dev())
    g = torch.zeros(L.total, device=dev())
    loss4 = (ctypes.c_float * 4)()
    N.check(h.lib.dppo_minibatch_grad_f32(h.h, new_d.data_ptr(), idx_d.data_ptr(), m, m_total,
                                          ctypes.byref(hp), g.data_ptr(), loss4, stream()))
    torch.cuda.synchronize()
    args = (c["obs"][idx], c["act"][idx], o["log_probs"][idx], o["advantages"][idx],
            o["returns"][idx])
    loss, comps, grads = P.minibatch_loss_grads(c["new"], *args, hy, cont, m_total=m_total,
                                                dt=np.float64)
    overall, per = G.gradient_errors(L, names, g.cpu().numpy(), grads)
    worst = max(per, key=per.get)
    print(f"OFFPOLICY {name}: shares {np.round(share, 3)} overall {overall:.3g} "
          f"worst tensor {per[worst]:.3g} ({worst})")
    assert overall <= 2e-5, overall
    for n in names:
        assert per[n] <= 1e-4, (n, per[n])
    want = (loss, comps["loss_policy"], comps["loss_value"], comps["entropy"])
    for got, x in zip(loss4, want):
        assert abs(got - x) <= 2e-5 * max(1.0, abs(x)), (tuple(loss4), want)


# ---------------------------------------------------------------------------------------------
# 2. GAE away from gamma = 0.99, lambda = 0.95
# ---------------------------------------------------------------------------------------------
def _run_gae(r, te, tr, v, nv, gamma, lam, mode):
    T, Nn = r.shape
    h = N.Handle(0, N.Dims(T, Nn, 1, 1, 0, 64, 1, 1, 1, 0))
    h.set_gae_mode(mode)
    adv = torch.empty(T, Nn, device=dev())
    ret = torch.empty(T, Nn, device=dev())
    ms = torch.zeros(4, device=dev())
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev())
    args = [t(r), t(te), t(tr), t(v), t(nv)]
    N.check(h.lib.dppo_gae_f32(h.h, *[a.data_ptr() for a in args], adv.data_ptr(), ret.data_ptr(),
                               gamma, lam, stream()))
    N.check(h.lib.dppo_adv_stats(h.h, ms.data_ptr(), stream()))
    torch.cuda.synchronize()
    return adv.cpu().numpy(), ret.cpu().numpy(), ms.cpu().numpy()


def _check_gae(r, te, tr, v, nv, gamma, lam, mode):
    T, Nn = r.shape
    adv, ret, ms = _run_gae(r, te, tr, v, nv, gamma, lam, mode)
    ref = P.gae(r, te, tr, v, nv, gamma, lam)
    if mode == N.GAE_EXACT:
        assert np.array_equal(adv, ref)
        assert np.array_equal(ret, v + ref)
    else:  # the bound of test_gae_affine_mode_within_tolerance
        scale = float(np.abs(ref).max())
        err = np.abs(adv.astype(np.float64) - ref).max()
        assert err <= 1e-6 * scale, (err, scale)
        assert np.abs(ret.astype(np.float64) - (v + ref)).max() <= 1e-6 * scale + 1e-6
    if adv.size > 1:
        mean, std = P.adv_stats(ref)
        assert abs(ms[0] - mean) <= 1e-6 * max(1.0, abs(mean)), (ms[0], mean)
        assert abs(ms[1] - std) <= 2e-6 * std, (ms[1], std)


def _gae_inputs(T, Nn, seed):
    rng = np.random.default_rng(seed)
    r = rng.normal(1, 1, (T, Nn)).astype(np.float32)
    te = (rng.random((T, Nn)) < 0.02).astype(np.uint8)
    tr = (rng.random((T, Nn)) < 0.005).astype(np.uint8)
    v = rng.standard_normal((T, Nn)).astype(np.float32)
    nv = rng.standard_normal((T, Nn)).astype(np.float32)
    return r, te, tr, v, nv


_GAMMA_LAMBDA = [(0.9, 0.8), (1.0, 1.0), (0.995, 0.0), (0.0, 0.95)]


@pytest.mark.parametrize("mode", [N.GAE_EXACT, N.GAE_AFFINE], ids=["exact", "affine"])
@pytest.mark.parametrize("T,Nn", [(1, 1), (129, 33), (300, 16), (128, 512)])
@pytest.mark.parametrize("gamma,lam", _GAMMA_LAMBDA)
def test_gae_other_gamma_lambda(gamma, lam, T, Nn, mode):
    _check_gae(*_gae_inputs(T, Nn, T * 13 + Nn), gamma, lam, mode)


@pytest.mark.parametrize("mode", [N.GAE_EXACT, N.GAE_AFFINE], ids=["exact", "affine"])
@pytest.mark.parametrize("flags", ["column terminated", "no flags"])
def test_gae_other_gamma_lambda_flag_edges(flags, mode):
    """One env terminated at every step (its advantages are r - v whatever gamma and lambda), and
    a rollout in which no episode ends."""
    T, Nn = 129, 33
    r, te, tr, v, nv = _gae_inputs(T, Nn, 5)
    if flags == "no flags":
        te[:], tr[:] = 0, 0
    else:
        te[:, 7] = 1
    _check_gae(r, te, tr, v, nv, 0.9, 0.8, mode)
    if flags != "no flags" and mode == N.GAE_EXACT:
        adv, _, _ = _run_gae(r, te, tr, v, nv, 0.9, 0.8, mode)
        assert np.array_equal(adv[:, 7], r[:, 7] - v[:, 7])


# ---------------------------------------------------------------------------------------------
# 3. whole learn() with non-default optimiser settings
# ---------------------------------------------------------------------------------------------
_LEARN_SHAPES = [(64, 8, 4, False), (64, 17, 6, True), (128, 8, 4, False), (128, 17, 6, True)]
# the wide class has one Adam path; the tuned class also runs the two selected by environment
_LEARN_CASES = [(*s, c, a) for s in _LEARN_SHAPES for c in (1e3, 0.05)
                for a in ((None,) if s[0] == 128 else (None, "DPPO_FUSED_ADAM", "DPPO_SPLIT_ADAM"))]


@pytest.mark.parametrize("Hd,D,A,cont,norm_clip,adam_path", _LEARN_CASES)
def test_two_learns_with_other_optimiser_settings(Hd, D, A, cont, norm_clip, adam_path,
                                                  monkeypatch):
    """Two consecutive learns (adam_step > 0 on entry of the second: Adam's bias corrections) with
    a norm clip that never (1e3) or always (0.05) applies; the tuned class also with the fused
    tail (DPPO_FUSED_ADAM=1) and the multi-rank kernel sequence (DPPO_SPLIT_ADAM=1)."""
    wide = Hd == 128
    monkeypatch.delenv("DPPO_FUSED_ADAM", raising=False)
    monkeypatch.delenv("DPPO_SPLIT_ADAM", raising=False)
    if adam_path:
        monkeypatch.setenv(adam_path, "1")
    T, Nn, E, M = 16, 64, 2, 2
    kw = dict(grad_norm_clip=norm_clip, adam_eps=1e-3, gamma=0.9, gae_lambda=0.8, ppo_clip=0.1,
              advantage_norm=False, num_epochs=E, num_minibatches=M)
    Cfg = diamond.ContinuousPPOConfig if cont else diamond.PPOConfig
    Agent = diamond.ContinuousPPO if cont else diamond.PPO
    cfg = Cfg(network_hidden_dim=Hd, rollout_steps=T, num_envs=Nn, verbose=False, **kw)
    agent = Agent(None, cfg, envs=SpecEnvs(D, A, cont))
    assert agent._learner.fused
    assert agent._learner.shape_class == ("wide" if wide else "tuned")
    names = [n for n, _ in agent.network.named_parameters()]
    params = {n: p.detach().cpu().numpy().copy() for n, p in agent.network.named_parameters()}
    seed = Hd + D + int(norm_clip)
    rollouts = [synth(T, Nn, D, A, cont, seed + k) for k in range(2)]
    np.random.seed(seed)
    st = np.random.get_state()
    traces = []
    for ro, _ in rollouts:
        agent.learn_device(ro)
        traces.append(agent.learn_trace().copy())
    torch.cuda.synchronize()
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
        np.testing.assert_allclose(traces[k][:, 0], ref["loss"], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(traces[k][:, 4], ref["norm"], rtol=1e-4, atol=1e-5)
    for n, p in agent.network.named_parameters():
        np.testing.assert_allclose(p.detach().cpu().numpy(), params[n], rtol=0, atol=2e-5,
                                   err_msg=n)


# ---------------------------------------------------------------------------------------------
# 4. dppo_clip_adam_f32 on its own
# ---------------------------------------------------------------------------------------------
def _clip_adam64(p, g, m, v, max_norm, lr, b1, b2, eps, step):
    """clip_grad_norm_ + Adam (the formulas of P.clip_grad_norm / P.adam_step) in float64."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    norm = np.sqrt((g * g).sum())
    g = g * min(max_norm / (norm + 1e-6), 1.0)
    m = m + (1 - b1) * (g - m)
    v = v * b2 + (1 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - b2 ** step) + eps
    return p - lr / (1 - b1 ** step) * (m / denom), m, v, norm


def _allowance(ref32, ref64, rtol, atol=0.0):
    """The tolerance, plus 4x whatever the float32 oracle itself misses it by against the float64
    evaluation of the same formulas.  Measured over the cases below: parameters and v are inside
    (no allowance); the first moment misses rtol 1e-5 by up to 5.2e-9 absolute (|m| ~ 0.05), at
    the few elements where m + (1 - beta1) (g - m) cancels to nearly zero."""
    miss = np.abs(ref32 - ref64) - (atol + rtol * np.abs(ref64))
    return atol + rtol * np.abs(ref32) + 4 * max(0.0, float(np.max(miss)))


@pytest.mark.parametrize("b1,b2", [(0.9, 0.999), (0.8, 0.99)])
@pytest.mark.parametrize("step", [1, 7, 1000])
@pytest.mark.parametrize("clips", [True, False])
@pytest.mark.parametrize("n", [1, 63, 12995, 100003])
def test_clip_adam_vs_oracle(n, clips, step, b1, b2):
    """One flat tensor, non-zero moments on entry, max_norm below (clips) and above the norm."""
    rng = np.random.default_rng(n + step)
    p = rng.standard_normal(n).astype(np.float32)
    g = (0.1 * rng.standard_normal(n)).astype(np.float32)
    m = (0.05 * rng.standard_normal(n)).astype(np.float32)
    v = ((0.05 * rng.standard_normal(n)) ** 2).astype(np.float32)
    norm64 = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
    max_norm = norm64 * (0.37 if clips else 2.5)
    lr, eps = 3e-4, 1e-5
    d = [torch.from_numpy(x.copy()).to(dev()) for x in (p, g, m, v)]
    out_norm = torch.zeros(1, device=dev())
    N.check(N.load().dppo_clip_adam_f32(*[x.data_ptr() for x in d], n, max_norm, lr, b1, b2, eps,
                                        step, out_norm.data_ptr(), stream()))
    torch.cuda.synchronize()
    gp, gg, gm, gv = (x.cpu().numpy() for x in d)
    assert np.array_equal(gg, g)   # the gradient buffer is read, not scaled in place
    names = ["x"]
    params, grads = {"x": p.copy()}, {"x": g.copy()}
    state = {"step": step - 1, "m": {"x": m.copy()}, "v": {"x": v.copy()}}
    total, coef = P.clip_grad_norm(grads, names, max_norm)
    assert (coef < 1) == clips
    # the C ABI takes the betas as floats
    P.adam_step(params, grads, state, names, lr, eps, float(np.float32(b1)), float(np.float32(b2)))
    p64, m64, v64, n64 = _clip_adam64(p, g, m, v, float(np.float32(max_norm)), lr,
                                      float(np.float32(b1)), float(np.float32(b2)),
                                      float(np.float32(eps)), step)
    assert abs(float(out_norm.item()) - total) <= 1e-6 * total
    assert abs(total - n64) <= 1e-6 * n64
    for got, r32, r64, rtol, atol, what in [(gp, params["x"], p64, 1e-6, 1e-7, "params"),
                                            (gm, state["m"]["x"], m64, 1e-5, 0.0, "m"),
                                            (gv, state["v"]["x"], v64, 1e-5, 0.0, "v")]:
        tol = _allowance(r32.astype(np.float64), r64, rtol, atol)
        err = np.abs(got.astype(np.float64) - r32)
        assert (err <= tol).all(), (what, float(err.max()), float(np.max(err - tol)))
