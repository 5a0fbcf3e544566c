"""GPU parity of the fused kernels in the numerical regimes of a trained policy.

Every other GPU test draws weights that keep tanh units in their active range, logits near 0,
unit-scale observations, O(1) rewards and Gaussian actions within a few sigma.  Here the same
kernels run on tests/regime_cases.py's inputs -- saturated layers (obs30, hidden6, obs1000),
pre-activations near 0 (obs1e-3), near-deterministic categorical policies (peaked20 / 30 / 60: logit
gaps of 55 to 250, exp(log p) underflowing, entropy near 0), narrow and wide Gaussians (sigma.05,
sigma4.5), actions four sigma out (tail4), returns in the hundreds (returns100) -- where the
kernels' exp2-based tanh, bare-log logsumexp, p * log p entropy and fast-exp ratio depart most from
the reference's arithmetic.  tests/test_regimes_cpu.py shows with the oracle alone that every
regime is reached and that the reference's own float32 arithmetic meets the bounds used here.

a. the minibatch gradient of all four families (dppo_prepare_f32 + dppo_minibatch_grad_f32 as
   tests/test_gpu_shapes.py runs them; dppo_gru_minibatch_grad_f32 as tests/test_gpu_gru.py, at
   gru_hidden_dim 16 and, with the scales of regime_cases.GRU_WIDE_REGIMES, at 32 and 64)
   against the float64 oracle: on-policy in every regime, off-policy (gpu_helpers.offpolicy_inputs
   with the regime's transform) in the near ones.  Near regimes: the bounds of
   tests/test_gpu_production.py -- err_kernel <= 2e-5, err_kernel <= 4 err_oracle32 + 1e-6, each
   tensor within 1e-4 of max(own scale, 1e-3 scale), the four loss terms within 2e-5 max(1, |x|).
   Far regimes (float32 itself degrades): everything finite, err_kernel <= 4 err_oracle32 + 1e-6,
   loss terms within 4 |loss32 - loss64| + 2e-5 max(1, |x|); err_oracle32 is the float32 oracle's
   own distance from the float64 one on the same records.  One (family, regime) misses that and
   has the bound of FAR_MEASURED instead.  The wide GRU's hidden6 rows are far (the recurrent map
   is chaotic there: regime_cases.GRU_WIDE_FAR) and keep the rule as it stands.
b. the old-policy evaluation behind dppo_prepare_f32 (eval_kernel, the wide eval): log-probs,
   values and next values within 2e-5 max(1, |exact|) + 4 |oracle32 - exact| of the float64 oracle
   per element (combined: a max-norm bound, see EVAL_MAX_NORM); returns == values + gae(values)
   bit for bit.
c. the rollout samplers (act_kernel, wide_act_kernel, the GRU act and next-value kernels of all
   three widths) at n = 33: heads / log-probs / values with the bound of b, discrete draws equal
   to the inverse CDF of the float64 softmax on every sample (all are clear of the CDF
   boundaries), Gaussian draws and the squash as tests/test_gpu_wide_act.py checks them.
d. one whole learn() per MLP family under obs30 and peaked20 (test_gpu_production.learn_vs_oracle
   with the regime's transform).

Measured figures: DESIGN.md §4.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diamond import _native as N
from oracle import ppo_np as P

import gpu_helpers as G
import gru_cases
import regime_cases as R
import wide_act_cases as W
from gpu_helpers import _figures, _within, dev, hparams, sample_split, stream, to_device
from test_gpu_rollout_ckpt import oracle_gaussian_draws, philox4x32_10, u01

_KEYS = ("log_probs", "values", "next_values", "advantages", "returns")


def _check_family(h, shape, m):
    fam, Hd, D, A, cont = shape
    plan = h.fused_plan(m)
    if fam == "wide":
        assert plan["shape_class"] == "wide"
    else:
        assert plan["shape_class"] == "tuned" and Hd == 64
        assert sample_split(D, A, cont) == (fam == "sample-split")


def _prepare_and_grad(shape, host, old_flat, new_flat, idx, hp, m_total):
    """dppo_prepare_f32 with old_flat, then one dppo_minibatch_grad_f32 with new_flat on idx:
    (records dict, flat gradient, the four loss words)."""
    B = R.T * R.NN
    h = N.Handle(0, R.dims(shape))
    _check_family(h, shape, len(idx))
    ro = to_device(host)
    old_d = torch.from_numpy(old_flat).to(dev())
    new_d = torch.from_numpy(new_flat).to(dev())
    outs = {k: torch.empty(B, device=dev()) for k in _KEYS}
    lo = N.LearnOutputs(*[outs[k].data_ptr() for k in _KEYS])
    N.check(h.lib.dppo_prepare_f32(h.h, ctypes.byref(ro.as_struct()), old_d.data_ptr(),
                                   ctypes.byref(hp), ctypes.byref(lo), stream()))
    idx_d = torch.from_numpy(idx).to(dev())
    g = torch.zeros(h.layout.total, device=dev())
    loss4 = (ctypes.c_float * 4)()
    N.check(h.lib.dppo_minibatch_grad_f32(h.h, new_d.data_ptr(), idx_d.data_ptr(), len(idx),
                                          m_total, ctypes.byref(hp), g.data_ptr(), loss4,
                                          stream()))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}, g.cpu().numpy(), tuple(loss4)


# (regime, family) whose kernel misses the far bound: finite, err_kernel <= 2 x the measured
# err_kernel / err_oracle32, err_kernel <= 1e-3.  combined on the sample-split kernel, measured on
# an MI355X: 8.87e-4 / 2.22e-4 = 4.00 at (D 8, A 4) -- on the 4 x bound itself, where the oracle's
# BLAS decides -- and 9.77e-4 / 4.90e-4 at (16, 8); over five more seeds of each shape 0.8-2.7,
# all in base.0.weight.  The other families: at most 1.0.  From the code (mbwave.hip tanh4,
# pk_dtanh, the g1 factor of layer 1): h = 1 - 2 rcp(2^x + 1) is rounded to the grid of 2^-24
# next to +-1 and carries up to an ulp of v_exp / v_rcp error before that, where libm's tanhf
# is within half an ulp; 1 - h^2 of a unit at 1 - 1e-5 turns an ulp of h into 1 % of the factor, and
# the x 30 observations and x 6 weights of this regime make those units the largest terms of
# base.0.weight's gradient.  The factor could be formed without the cancellation as 4 r (1 - r)
# from r = rcp(2^x + 1), at the price of keeping r live through the backward pass.
FAR_MEASURED = {("combined", "sample-split"): 4.00}


def _check_gradient(tag, far, L, names, got_flat, loss4, res, err32, measured=None):
    """The bounds of the regime's class on one gradient and its four loss words."""
    l32, c32, _ = res[np.float32]
    l64, c64, g64 = res[np.float64]
    exact = {n: g64[sum(L.numel[:k]):][:L.numel[k]] for k, n in enumerate(names)}
    err, per = G.gradient_errors(L, names, got_flat, exact)
    worst = max(per, key=per.get)
    print(f"REGIME {tag}: err_kernel {err:.3g} err_oracle32 {err32:.3g} worst tensor "
          f"{per[worst]:.3g} ({worst})")
    want = [(l64, l32)] + [(c64[k], c32[k]) for k in ("loss_policy", "loss_value", "entropy")]
    assert np.isfinite(got_flat).all() and np.isfinite(loss4).all()
    if measured is not None:
        assert far and err <= 2 * measured * err32 and err <= 1e-3, (err, err32)
        return
    assert err <= 4 * err32 + 1e-6, (err, err32)
    if far:
        for got, (x64, x32) in zip(loss4, want):
            assert abs(got - x64) <= 4 * abs(x32 - x64) + 2e-5 * max(1.0, abs(x64)), (loss4, want)
        return
    assert err <= 2e-5, (err, err32)
    for n in names:
        assert per[n] <= 1e-4, (n, per[n])
    for got, (x64, _) in zip(loss4, want):
        assert abs(got - x64) <= 2e-5 * max(1.0, abs(x64)), (loss4, want)


# ---------------------------------------------------------------------------------------------
# a / b. MLP families, on-policy: one prepare + gradient per case, shared by both tests
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _onpolicy(name, shape):
    c = R.build_onpolicy(R.REGIMES[name], shape)
    o, g, loss4 = _prepare_and_grad(shape, c["host"], c["flat"], c["flat"], c["idx"], hparams(),
                                    len(c["idx"]))
    return c, o, g, loss4


@pytest.mark.parametrize("case", R.mlp_cases(), ids=R.case_id)
def test_onpolicy_minibatch_gradient_in_regime(case):
    regime, shape = case
    _, Hd, D, A, cont = shape
    c, o, g, loss4 = _onpolicy(regime.name, shape)
    B, idx = R.T * R.NN, c["idx"]
    obs, _, act, *_ = c["host"]
    args = (obs.reshape(B, D)[idx], act.reshape(B, *act.shape[2:])[idx], o["log_probs"][idx],
            o["advantages"][idx], o["returns"][idx])
    res, err32 = R.oracle_pair(c["params"], args, P.Hyper(), cont)
    _check_gradient(f"on {R.case_id(case)}", regime.far, c["L"], c["names"], g, loss4, res, err32,
                    FAR_MEASURED.get((regime.name, shape[0])))


# combined (far): the per-element bound of b does not hold, in any family.  Measured on an MI355X,
# log-probs: max |kernel - f64| 3.6e-4 .. 1.0e-3 against max |oracle32 - f64| 2.8e-4 .. 2.1e-3, with
# 1 to 4 of the 1,536 elements beyond the bound by 6e-7 .. 2.5e-4 (values: one element of one shape
# by 1.2e-5).  The first layer's pre-activations are sums of terms near 1,000, so the few units that
# are not saturated carry a float32 rounding error of 1e-4 that the x 6 and x 20 layers pass on to
# the logits; it falls on other elements in the kernel (weights pre-scaled by kTS, another
# summation order) than in NumPy, and 4 x the oracle's error AT THE SAME ELEMENT does not cover
# that: a NumPy float32 forward with kTS-scaled weights and tanh = 1 - 2 / (2^x + 1) misses the
# bound on 1 to 4 elements of these inputs as well.  So, as for a far gradient that misses its
# bound: finite, max |kernel - f64| <= 2 x the measured ratio to max |oracle32 - f64| of the
# family (largest over the three outputs and the family's shapes; no less than the usual 4 x, the
# oracle's side moving with its BLAS), and <= 1e-3 of the output's scale.  Measured max |kernel -
# f64| / max |oracle32 - f64| (log_probs, values, next_values):
#   sample-split D8 A4    4.37e-4 / 2.85e-4   2.16e-5 / 2.36e-5   1.76e-5 / 3.39e-5
#   sample-split D16 A8   1.03e-3 / 1.13e-3   1.01e-4 / 4.42e-5   3.14e-5 / 5.12e-5
#   two-team D32 A16      6.59e-4 / 2.08e-3   2.53e-5 / 5.33e-5   3.06e-5 / 5.68e-5
#   wide H128 D8 A4       3.59e-4 / 2.77e-4   1.19e-5 / 1.62e-5   2.38e-5 / 1.79e-5
#   wide H64 D40 A5       6.50e-4 / 1.03e-3   5.39e-5 / 2.89e-5   6.73e-5 / 3.84e-5
EVAL_MAX_NORM = {"combined": {"sample-split": 2.29, "two-team": 0.54, "wide": 1.87}}


@pytest.mark.parametrize("case", R.mlp_cases(), ids=R.case_id)
def test_old_policy_eval_in_regime(case):
    regime, shape = case
    _, Hd, D, A, cont = shape
    c, o, _, _ = _onpolicy(regime.name, shape)
    obs, nobs, act, rew, te, tr = c["host"]
    p64 = {k: v.astype(np.float64) for k, v in c["params"].items()}
    f = P.forward(p64, obs, cont, np.float64)
    if cont:
        lp64 = P.normal_logp_entropy(f["out"], p64["actor_log_std"], act, np.float64)[0]
    else:
        lp64 = P.categorical_logp_entropy(f["out"], act, np.float64)[0]
    nv64 = P.forward(p64, nobs, cont, np.float64)["v"]
    lp32, v32, nv32, _ = P.old_policy(c["params"], obs, act, nobs, cont)
    outs = (("log_probs", lp64, lp32), ("values", f["v"], v32), ("next_values", nv64, nv32))
    figs = {k: _figures(o[k], x64.ravel(), x32.ravel()) for k, x64, x32 in outs}
    print(f"REGIME eval {R.case_id(case)}: " + " ".join(
        f"{k} max |kernel - f64| {a:.3g} |oracle32 - f64| {b:.3g} beyond {n} by {x:.3g};"
        for k, (a, b, n, x) in figs.items()))
    for k, x64, x32 in outs:
        if regime.name in EVAL_MAX_NORM:
            a, b, _, _ = figs[k]
            assert np.isfinite(o[k]).all(), k
            assert a <= max(2 * EVAL_MAX_NORM[regime.name][shape[0]], 4.0) * b, (k, a, b)
            assert a <= 1e-3 * max(1.0, np.abs(x64).max()), (k, a)
        else:
            _within(o[k], x64.ravel(), x32.ravel(), k)
    vals, nvals = o["values"].reshape(R.T, R.NN), o["next_values"].reshape(R.T, R.NN)
    raw = P.gae(rew, te, tr, vals, nvals)
    assert np.array_equal(o["returns"].reshape(R.T, R.NN), vals + raw)
    np.testing.assert_allclose(o["advantages"], P.normalize_adv(raw).ravel(), rtol=0, atol=2e-6)


# ---------------------------------------------------------------------------------------------
# a. MLP families, off-policy (near regimes)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.mlp_cases(R.NEAR), ids=R.case_id)
def test_offpolicy_minibatch_gradient_in_regime(case):
    regime, shape = case
    cont = shape[4]
    L, names, hy, c = R.build_offpolicy(regime, shape)
    m, idx = R.minibatch_size(), c["idx"]
    G.check_offpolicy_conditions(c["regime"][idx], m, c["near"], c["far"])
    hp = hparams(ppo_clip=hy.ppo_clip, value_loss_weight=hy.value_loss_weight,
                 entropy_beta=hy.entropy_beta, advantage_norm=int(hy.advantage_norm))
    o, g, loss4 = _prepare_and_grad(shape, c["host"], c["old_flat"], c["new_flat"], idx, hp, m)
    # the regimes of the surrogate still hold on the kernel's own records
    logp_new = G.new_policy_logp64(c["new"], c["obs"][idx], c["act"][idx], cont)
    reg, _, _ = G.surrogate_regimes(np.exp(logp_new - o["log_probs"][idx]), o["advantages"][idx],
                                    hy.ppo_clip, near_bound=G.NEAR_BOUND / 2)
    G.check_offpolicy_conditions(reg, m, c["near"], c["far"])
    args = (c["obs"][idx], c["act"][idx], o["log_probs"][idx], o["advantages"][idx],
            o["returns"][idx])
    res, err32 = R.oracle_pair(c["new"], args, hy, cont)
    _check_gradient(f"off {R.case_id(case)}", False, L, names, g, loss4, res, err32)


# ---------------------------------------------------------------------------------------------
# a. GRU
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GRU_CASES + R.GRU_WIDE_CASES, ids=str)
def test_gru_minibatch_gradient_in_regime(case):
    from test_gpu_gru import _kernel_grad
    from oracle import gru_torch as GT
    if hasattr(case, "G"):      # gru_hidden_dim 32 / 64: csrc/grugrad.hip
        from test_gpu_gru_wide import _case_agent
    else:
        from test_gpu_gru import _case_agent
    params, x, mb_idx, m_total = R.gru_build(case)
    gru_cases.guards(case, params, x, mb_idx)
    agent = _case_agent(case, params)
    L = agent.gru.layout
    g = _kernel_grad(agent, x, mb_idx, m_total, case.clip, case.vf, case.ent).cpu().numpy()
    res, err32 = R.gru_oracle_pair(case, params, x, mb_idx, m_total)
    s64, ref = res[torch.float64]
    scale = max(np.abs(r).max() for r in ref.values())
    per = {}
    for i, n in enumerate(GT.GRU_NAMES):
        got = g[L.offset[i]:L.offset[i] + L.numel[i]].reshape(ref[n].shape)
        per[n] = np.abs(got - ref[n]).max()
    err = max(per.values()) / scale
    print(f"REGIME gru {case}: err_kernel {err:.3g} err_oracle32 {err32:.3g}")
    assert np.isfinite(g).all()
    assert err <= 4 * err32 + 1e-6, (err, err32)
    if R.gru_is_far(case):
        # float32 itself degrades (regime_cases.GRU_WIDE_FAR): the far rule of _check_gradient
        assert case.on_policy and err <= 1e-3, (err, err32)
        s32 = res[torch.float32][0]
    else:
        assert err <= 2e-5, (err, err32)
        for n in GT.GRU_NAMES:
            own = max(np.abs(ref[n]).max(), 1e-3 * scale)
            assert per[n] <= 1e-4 * own, (n, per[n] / own)
        s32 = s64

    def terms(s):
        pi, vl, en = (float(v) / m_total for v in s)
        return pi + case.vf * vl - case.ent * en, pi, vl, en

    for got, x64, x32 in zip(terms(g[L.total:L.total + 3]), terms(s64), terms(s32)):
        assert abs(got - x64) <= 4 * abs(x32 - x64) + 2e-5 * max(1.0, abs(x64)), (got, x64)


# ---------------------------------------------------------------------------------------------
# c. rollout samplers
# ---------------------------------------------------------------------------------------------
def _sampler_handle(shape):
    _, Hd, D, A, cont = shape
    return N.Handle(0, W.dims(Hd, D, A, cont))


@pytest.mark.parametrize("case", R.sampler_cases(), ids=R.case_id)
def test_mlp_sampler_in_regime(case):
    from test_gpu_wide_act import _act, _act_squash, _bounds, _heads, _to_dev
    regime, shape = case
    _, Hd, D, A, cont = shape
    n = R.SAMPLER_N
    params, flat, obs = R.sampler_inputs(regime, shape)
    h, pd, od = _sampler_handle(shape), _to_dev(flat), _to_dev(obs)
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    out64 = P.forward(p64, obs, cont, np.float64)["out"]
    out32 = P.forward(params, obs, cont)["out"]
    d, d32 = _within(_heads(h, pd, od, n, A), out64, out32, "heads")
    print(f"REGIME sampler {R.case_id(case)}: max |heads - f64| {d:.3g}, oracle32 {d32:.3g}")
    if not cont:
        got = _act(h, pd, od, n, A, False, R.SEED, R.COUNTER)
        want, clear = W.categorical_oracle(out64, R.SEED, R.COUNTER, philox4x32_10, u01)
        assert clear.mean() >= W.MIN_CLEAR
        assert got.min() >= 0 and got.max() < A
        assert np.array_equal(got[clear], want[clear])
        return
    u = _act(h, pd, od, n, A, True, R.SEED, R.COUNTER)
    want = oracle_gaussian_draws(out64, params["actor_log_std"], R.SEED, R.COUNTER)
    np.testing.assert_allclose(u, want, rtol=1e-4, atol=1e-4)
    if regime.name == "sigma4.5":
        assert (np.abs(u) > 3).any()   # tanh's tails are hit
    lo, hi = _bounds(A)
    for bounded in (False, True):
        u2, env = _act_squash(h, pd, od, n, A, R.SEED, R.COUNTER, lo if bounded else None,
                              hi if bounded else None)
        assert np.array_equal(u2, u)
        if bounded:
            env_own = P.squash_action(u2, lo.astype(np.float64), hi.astype(np.float64))
            assert np.all(env >= lo) and np.all(env <= hi)
            atol = float(4e-7 * (1 + np.abs(lo).max()))
        else:
            env_own = np.tanh(u2.astype(np.float64))
            assert np.all(np.abs(env) <= 1.0)
            atol = 4e-7
        np.testing.assert_allclose(env, env_own, rtol=0, atol=atol)


@functools.lru_cache(maxsize=None)
def _gru_agent(D, A, G=gru_cases.G):
    from test_gpu_gru_act import _agent
    return _agent(2, 4, D, A, spread=False, G=G)


def _gru_net(agent, params, dt):
    from diamond.recurrent_ppo import RecurrentActorCriticNetwork
    net = RecurrentActorCriticNetwork(agent.envs.single_observation_space,
                                      agent.envs.single_action_space, cfg=agent.cfg).to(dt)
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.copy_(torch.from_numpy(params[n]).to(dt))
    return net


def _gru_step(net, dt, obs, dones, hx):
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dt)
    with torch.no_grad():
        lg, v, h = net.get_logits_values_and_hx(t(obs)[None], t(hx)[None],
                                                torch.from_numpy(np.asarray(dones, bool))[None])
    return lg[0].double().numpy(), v[0].double().numpy(), h[0].double().numpy()


def _gru_value(net, dt, obs, hx):
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dt)
    with torch.no_grad():
        return net.get_values(t(obs)[None], t(hx)[None], None)[0].double().numpy()


def _gru_sampler(regime, D, A, G):
    from test_gpu_gru_act import log_softmax64, run_act, run_value
    n = R.SAMPLER_N
    params, obs, dones, hx, nobs = R.gru_sampler_inputs(regime, D, A, G)
    agent = _gru_agent(D, A, G)
    assert agent.gru is not None and agent.gru.dims.gru_hidden == G == hx.shape[1]
    with torch.no_grad():
        for name, p in agent.network.named_parameters():
            p.copy_(torch.from_numpy(params[name]))
    net64, net32 = (_gru_net(agent, params, dt) for dt in (torch.float64, torch.float32))
    got = run_act(agent, obs, dones, hx, R.SEED, R.COUNTER)
    lg64, v64, h64 = _gru_step(net64, torch.float64, obs, dones, hx)
    lg32, v32, h32 = _gru_step(net32, torch.float32, obs, dones, hx)
    figs = [_within(got[k], x64, x32, k) for k, x64, x32 in
            (("logits", lg64, lg32), ("values", v64, v32), ("hx_out", h64, h32))]
    act = got["actions"]
    want, clear = W.categorical_oracle(lg64, R.SEED, R.COUNTER, philox4x32_10, u01)
    assert clear.mean() >= W.MIN_CLEAR
    assert np.array_equal(act[clear], want[clear])
    i = np.arange(n)
    lp = _within(got["log_probs"], log_softmax64(lg64)[i, act], log_softmax64(lg32)[i, act],
                 "log_probs")
    # V(next_obs) from the step's own new hidden state
    nv = _within(run_value(agent, nobs, got["hx_out"]),
                 _gru_value(net64, torch.float64, nobs, got["hx_out"]),
                 _gru_value(net32, torch.float32, nobs, got["hx_out"]), "next values")
    print(f"REGIME gru sampler {regime}-D{D}-A{A}-G{G}: max |kernel - f64| / |oracle32 - f64| "
          f"logits "
          f"{figs[0][0]:.3g} / {figs[0][1]:.3g} values {figs[1][0]:.3g} / {figs[1][1]:.3g} hx "
          f"{figs[2][0]:.3g} / {figs[2][1]:.3g} log_probs {lp[0]:.3g} / {lp[1]:.3g} next values "
          f"{nv[0]:.3g} / {nv[1]:.3g}")


@pytest.mark.parametrize("D,A", R.GRU_SAMPLER_SHAPES)
@pytest.mark.parametrize("regime", R.GRU_SAMPLER_REGIMES)
def test_gru_sampler_in_regime(regime, D, A):
    _gru_sampler(regime, D, A, gru_cases.G)


@pytest.mark.parametrize("G", R.gru_wide_cases.WIDTHS)
@pytest.mark.parametrize("D,A", R.GRU_SAMPLER_SHAPES)
@pytest.mark.parametrize("regime", R.GRU_SAMPLER_REGIMES)
def test_gru_wide_sampler_in_regime(regime, D, A, G):
    """The same at gru_hidden_dim 32 and 64 (csrc/gruact.hip), with GRU_WIDE_REGIMES' scales."""
    _gru_sampler(regime, D, A, G)


# ---------------------------------------------------------------------------------------------
# d. one whole learn() per MLP family
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.LEARN_SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("name", R.LEARN_REGIMES)
def test_learn_in_regime_vs_oracle(name, shape):
    from test_gpu_production import learn_vs_oracle
    fam, Hd, D, A, cont = shape
    learn_vs_oracle(R.T, R.NN, D, A, cont, seed=R.case_seed(R.REGIMES[name], shape),
                    transform=R.learn_transform(R.REGIMES[name], shape), hidden=Hd)
