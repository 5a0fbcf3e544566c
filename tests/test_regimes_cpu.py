"""The inputs of tests/test_gpu_regimes.py, checked with the oracle alone.

tests/regime_cases.py moves the suites' usual inputs into the numerical regimes of a trained policy.
For every (regime, shape) this module asserts, without a GPU, that

* the regime is reached: the share of saturated units, the logit gap, the smallest log-prob of a
  taken action, the size of the first layer's input term;
* the float32 and the float64 oracle are finite in every gradient entry and loss term;
* err_oracle32 = max|g32 - g64| / max|g64| stays under the cap of the regime's class (near 1e-5,
  far 1e-3), and in the near regimes each tensor of the float32 oracle's gradient is within 5e-5
  of max(own scale, 1e-3 max|g|): the bounds tests/test_gpu_regimes.py holds the kernels to are
  met by the reference's own float32 arithmetic with room to spare, so a kernel that misses them
  is wrong;
* off-policy (near regimes): gpu_helpers.check_offpolicy_conditions holds unchanged at the case's
  noise scale, and the perturbed parameters are still in the regime;
* the rollout samplers' discrete draws are clear of every CDF boundary (wide_act_cases.CLEAR_MARGIN,
  MIN_CLEAR), and the wide Gaussian's draws pass |u| = 3.

obs1e-3: random_params draws the first layer's biases from N(0, 0.1), so the pre-activation itself
is up to 0.33 whatever the observations are; the 0.05 bound is on the observations' term W x, the
part the regime scales, and the whole pre-activation is held under 0.05 + max|b|.
"""
import numpy as np
import pytest

import gpu_helpers as G
import gru_cases
import regime_cases as R
import wide_act_cases as W
from oracle import ppo_np as P
from test_gpu_rollout_ckpt import oracle_gaussian_draws, philox4x32_10, u01


def _assert_reached(regime, r, params, obs):
    name = regime.name
    if regime.obs == 30.0:
        assert r["sat1"] >= 0.8, r
    if regime.hidden == 6.0:
        assert r["sat1"] >= 0.45 and r["sat2"] >= 0.45, r
    if name == "obs1000":
        assert r["sat1"] >= 0.99, r
    if name in ("peaked20", "combined"):
        assert r["gap"] >= 55, r
    if name == "peaked30":
        assert r["gap"] >= 90 and r["min_logp"] <= -80, r
    if name == "peaked60":
        assert r["gap"] >= 160, r
    if name == "tail4":
        assert r["min_logp"] <= -60, r
    if name == "obs1e-3":
        w, b = params["base.0.weight"].astype(np.float64), params["base.0.bias"]
        wx = np.abs(obs.reshape(-1, obs.shape[-1]).astype(np.float64) @ w.T).max()
        assert wx <= 0.05, wx
        assert r["pre1"] <= 0.05 + np.abs(b).max(), r


def _assert_oracles(res, err, cap, L=None, names=None):
    for dt, (loss, comps, g) in res.items():
        assert np.isfinite(g).all() and np.isfinite(loss), dt
        assert all(np.isfinite(v) for v in comps.values()), (dt, comps)
    assert err <= cap, err
    if L is not None:   # near: no tensor so ill-conditioned that float32 itself nears the bound
        off = np.cumsum([0] + [L.numel[k] for k in range(L.count)])
        g32, g64 = res[np.float32][2], res[np.float64][2]
        scale = np.abs(g64).max()
        for k, n in enumerate(names):
            a, b = g32[off[k]:off[k + 1]], g64[off[k]:off[k + 1]]
            per = np.abs(a - b).max() / max(np.abs(b).max(), 1e-3 * scale)
            assert per <= R.TENSOR_CAP, (n, per)


@pytest.mark.parametrize("case", R.mlp_cases(), ids=R.case_id)
def test_onpolicy_regime_is_reached_and_float32_oracle_meets_its_cap(case):
    regime, shape = case
    _, Hd, D, A, cont = shape
    c = R.build_onpolicy(regime, shape)
    obs, nobs, act, rew, te, tr = c["host"]
    B = R.T * R.NN
    logp, v, nv, _ = P.old_policy(c["params"], obs, act, nobs, cont)
    adv = P.gae(rew, te, tr, v, nv)
    ret = v + adv
    adv = P.normalize_adv(adv)
    idx = c["idx"]
    assert len(np.unique(idx)) == idx.size and idx.size % 16 != 0
    args = (obs.reshape(B, D)[idx], act.reshape(B, *act.shape[2:])[idx], logp.ravel()[idx],
            adv.ravel()[idx], ret.ravel()[idx])
    res, err = R.oracle_pair(c["params"], args, P.Hyper(), cont)
    r = R.reached(c["params"], obs, act, cont)
    print(f"{R.case_id(case)}: err_oracle32 {err:.3g} reached {r} "
          f"loss_value {res[np.float64][1]['loss_value']:.4g}")
    _assert_reached(regime, r, c["params"], obs)
    if regime.far:
        _assert_oracles(res, err, R.FAR_CAP)
    else:
        _assert_oracles(res, err, R.NEAR_CAP, c["L"], c["names"])
    if regime.rewards == 100.0:
        assert res[np.float64][1]["loss_value"] >= 1e5
    if regime.log_std is not None:
        assert np.all(c["params"]["actor_log_std"] == np.float32(regime.log_std))
        assert abs(regime.log_std) <= 6


@pytest.mark.parametrize("case", R.mlp_cases(R.NEAR), ids=R.case_id)
def test_offpolicy_regime_conditions_hold(case):
    regime, shape = case
    cont = shape[4]
    L, names, hy, c = R.build_offpolicy(regime, shape)
    m, idx = R.minibatch_size(), c["idx"]
    share = G.check_offpolicy_conditions(c["regime"][idx], m, c["near"], c["far"])
    obs = c["host"][0]
    for which in ("old", "new"):
        _assert_reached(regime, R.reached(c[which], obs, c["host"][2], cont), c[which], obs)
    if cont:
        assert np.abs(c["new"]["actor_log_std"]).max() <= 6
    # the reference's own backward stays finite: no ratio near exp(88)
    assert (np.log(c["ratio"][idx]) < 80).all()
    args = (c["obs"][idx], c["act"][idx], c["logp_old"][idx], c["adv"][idx], c["ret"][idx])
    res, err = R.oracle_pair(c["new"], args, hy, cont)
    print(f"{R.case_id(case)}: s {R.OFFPOLICY_S[(regime.name, R.shape_id(shape))]} shares "
          f"{np.round(share, 3)} near {c['near']:.4f} far {c['far']:.4f} ratio "
          f"{c['ratio'].min():.3g}..{c['ratio'].max():.3g} err_oracle32 {err:.3g}")
    _assert_oracles(res, err, R.NEAR_CAP, L, names)


@pytest.mark.parametrize("case", R.GRU_CASES + R.GRU_WIDE_CASES, ids=str)
def test_gru_regime_is_reached_and_float32_oracle_meets_its_cap(case):
    import torch
    params, x, mb_idx, m_total = R.gru_build(case)
    assert params["gru.weight_hh_l0"].shape[1] == x["hx0"].shape[1] == getattr(case, "G", 16)
    edge, share = gru_cases.guards(case, params, x, mb_idx)
    res, err = R.gru_oracle_pair(case, params, x, mb_idx, m_total)
    r = R.gru_reached(params, x)
    print(f"{case}: m {len(mb_idx)} nearest edge {edge:.3g} clipped share {share:.2f} "
          f"err_oracle32 {err:.3g} reached {r}")
    name = R.gru_regime(case)
    if name == "obs30":
        assert r["sat1"] >= 0.8, r
    if name == "hidden6":
        assert r["gates"] >= 0.45 and r["cand"] >= 0.45, r
    if name == "peaked20":
        assert r["gap"] >= 55, r
    if name == "peaked30":
        assert r["gap"] >= 90 and r["min_logp"] <= -80, r
    if name == "returns100":
        assert res[torch.float64][0][1] / m_total >= 1e3     # the value loss
    for dt, (sums, g) in res.items():
        assert np.isfinite(sums).all() and all(np.isfinite(t).all() for t in g.values()), dt
    if R.gru_is_far(case):
        # float32 itself degrades: on-policy only, held to the far cap -- and so is the float32
        # oracle with its weights an ulp away, or the row was a lucky draw of a chaotic map
        nudged = R.gru_oracle32_nudged(case, params, x, mb_idx, m_total)
        print(f"{case}: err_oracle32 nudged {nudged}")
        assert case.on_policy and name == "hidden6"
        assert R.NEAR_CAP < err <= R.FAR_CAP and max(nudged) <= R.FAR_CAP, (err, nudged)
    else:
        assert err <= R.NEAR_CAP, err


@pytest.mark.parametrize("case", R.sampler_cases(), ids=R.case_id)
def test_sampler_inputs(case):
    regime, shape = case
    _, Hd, D, A, cont = shape
    params, flat, obs = R.sampler_inputs(regime, shape)
    assert np.isfinite(flat).all()
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    out = P.forward(p64, obs, cont, np.float64)["out"]
    if cont:
        u = oracle_gaussian_draws(out, params["actor_log_std"], R.SEED, R.COUNTER)
        z = (u - out) / np.exp(p64["actor_log_std"])
        assert np.abs(z).max() < 6
        if regime.name == "sigma4.5":
            assert (np.abs(u) > 3).any()
    else:
        want, clear = W.categorical_oracle(out, R.SEED, R.COUNTER, philox4x32_10, u01)
        assert clear.mean() >= W.MIN_CLEAR, clear.mean()
        if regime.actor_out > 1:   # peaked: the boundaries sit next to 0 and 1
            p = np.exp(P.log_softmax(out, np.float64))
            assert np.median(p.max(1)) > 0.9


def _gru_sampler_inputs(regime, D, A, G):
    params, obs, dones, hx, nobs = R.gru_sampler_inputs(regime, D, A, G)
    assert hx.shape == (R.SAMPLER_N, G) and params["gru.weight_hh_l0"].shape == (3 * G, G)
    lg = R.gru_step_logits(params, obs, dones, hx)
    want, clear = W.categorical_oracle(lg, R.SEED, R.COUNTER, philox4x32_10, u01)
    assert np.isfinite(lg).all()
    assert clear.mean() >= W.MIN_CLEAR, clear.mean()
    if regime.startswith("peaked"):     # the scale of the gradient case carries over to one step
        assert (lg.max(1) - lg.min(1)).max() >= (20 if regime == "peaked20" else 30)


@pytest.mark.parametrize("D,A", R.GRU_SAMPLER_SHAPES)
@pytest.mark.parametrize("regime", R.GRU_SAMPLER_REGIMES)
def test_gru_sampler_inputs(regime, D, A):
    _gru_sampler_inputs(regime, D, A, gru_cases.G)


@pytest.mark.parametrize("G", R.gru_wide_cases.WIDTHS)
@pytest.mark.parametrize("D,A", R.GRU_SAMPLER_SHAPES)
@pytest.mark.parametrize("regime", R.GRU_SAMPLER_REGIMES)
def test_gru_wide_sampler_inputs(regime, D, A, G):
    _gru_sampler_inputs(regime, D, A, G)


@pytest.mark.parametrize("shape", R.LEARN_SHAPES, ids=R.shape_id)
@pytest.mark.parametrize("name", R.LEARN_REGIMES)
def test_learn_inputs_are_in_regime(name, shape):
    _, Hd, D, A, cont = shape
    regime = R.REGIMES[name]
    seed = R.case_seed(regime, shape)
    host = G.synth_host(R.T, R.NN, D, A, cont, seed)
    L = R.N.param_layout(R.dims(shape))
    init, _ = G.random_params(L, R.names_of(cont), D, A, cont, np.random.default_rng(0))
    params, obs, nobs, act, rew = R.learn_transform(regime, shape)(init, *host[:4])
    _assert_reached(regime, R.reached(params, obs, act, cont), params, obs)


@pytest.mark.parametrize("name", ["regime-obs100", "regime-peaked20"])
def test_recurrent_learn_rows_are_in_regime(name):
    """The two regime rows of tests/test_gpu_gru_learn.py: the base layer saturated as obs30 asks
    (>= 0.8 beyond 0.999), the initial policy as sharp as peaked20 (gap >= 55) and on-policy."""
    import test_gpu_gru_learn as TL
    from oracle import gru_torch as GT
    T, Nn, D, A = TL.CASES[name][0]
    x = GT.stack_experience(TL._experience(name, 0, "cpu"))
    params = TL._initial_params(name, D, A, TL._config(name).seed)
    r = R.gru_reached(params, x)
    if name == "regime-obs100":
        assert r["sat1"] >= 0.8, r
    else:
        assert r["gap"] >= 55, r
        lp = GT.log_probs(params, x["obs"], x["actions"], x["prev_dones"], x["hx0"])
        assert np.abs(np.exp(lp - x["log_probs"]) - 1).max() <= 1e-5
    assert np.isfinite(TL._oracle(name)[0]["losses"]).all()


def test_tables_cover_every_path_and_class():
    assert {s[0] for s in R.SHAPES} == {"sample-split", "two-team", "wide"}
    for fam in ("sample-split", "two-team", "wide"):
        assert {s[4] for s in R.SHAPES if s[0] == fam} == {False, True}
    assert [r.name for r in R.REGIMES.values() if r.far] == ["obs1000", "peaked60", "combined"]
    assert set(R.OFFPOLICY_S) == {(r.name, R.shape_id(s)) for r, s in R.mlp_cases(R.NEAR)}
    # the existing GRU cases keep their ids and inputs: every regime field defaults to identity
    for c in gru_cases.CASES + R.gru_wide_cases.CASES + R.gru_wide_cases.LONG_CASES:
        assert (c.obs_scale, c.gru_scale, c.actor_scale, c.ret_scale, c.old_noise) \
            == (1.0, 1.0, 1.0, 1.0, 0.0)
        assert c.seed_shift == R.gru_wide_cases.SEED_SHIFT.get((getattr(c, "G", 16), c.name), 0)
    # the wide regime table: both widths on both shapes, all five regimes, the far rows on-policy
    assert set(R.GRU_WIDE_REGIMES) == {(g, s) for g in R.gru_wide_cases.WIDTHS
                                       for s in R.GRU_SHAPES}
    assert all(set(row) == set(R.GRU_REGIMES) for row in R.GRU_WIDE_REGIMES.values())
    assert all(r == "hidden6" for r, _, _ in R.GRU_WIDE_FAR)
    assert len(R.GRU_WIDE_CASES) == 2 * 20 - len(R.GRU_WIDE_FAR)
    assert all(not R.gru_is_far(c) for c in R.GRU_CASES)
