"""GPU checks of the wide family's large heads: hidden 64 with obs_dim up to 384 and up to 32
actions (csrc/mbwide.hip wide_mb_kernel<64, CONT, NB1 in 2..24, false, AB in 1, 2>,
wide_eval_kernel<64, CONT, 2>, wide_act_kernel<64, CONT, 2>; csrc/dispatch.cpp wide_large_shape).
Cases and inputs: tests/wide_large_cases.py; tests/test_wide_large_cpu.py asserts the tables'
coverage, that the float32 oracle meets the same bounds on the same inputs, and that the bounds
turn down a gradient without dW1's columns from 128 on, without the second action block or
without the last action.

The yardstick is oracle/ppo_np.py in float64.  Bounds are the wide family's
(wide_mb_cases.check_gradient: overall 2e-5 max|g|, each tensor 1e-4 of its own scale floored at
1e-3 max|g|, loss and entropy 2e-5 max(1, |x|); evaluation and heads rtol = atol = 2e-5; learn():
test_gpu_wide_mb.test_ragged_learn_vs_oracle's), the sampler's are tests/test_gpu_wide_act.py's and
the regimes' tests/test_gpu_regimes.py's (near: 2e-5 max(1, |exact|) + 4 |oracle32 - exact| per
element of the heads, every clear discrete draw equal, Gaussian draws rtol = atol = 1e-4).

1  dppo_fused_plan and fused_shape_class agree at the new shapes; dppo_prepare_f32 runs where the
   class applies and raises NotImplementedError past it
2  old-policy evaluation and records, every width and action case, B = 128 and B = 105
3  minibatch gradient: every new instantiation at m = 379 on- and off-policy; widths at m = 71
   (one workgroup, three tiles), action counts at m = 135 (workgroups of three and two tiles),
   both at m = 7; two launches give the same bits
4  learn() through ContinuousPPO / PPO at 348 x 17 and 136 x 20 against the oracle's learn, and a
   checkpoint round trip
5  wide_act_kernel: heads, Gaussian draws with both squash modes, categorical draws that reach
   the second action block and the last action, a second tile per workgroup
6  regimes: a logit gap of 230 at 32 actions, sigma 0.05 and 4.5 at 17

Measured on an MI355X (largest overall error / max|g| and largest per-tensor error / own scale
over the group's cases; every case is printed by its test):

    group                      overall  worst tensor
    I  on-policy, m = 379      6.1e-6   2.9e-5  (D190 A32 Gaussian, actor_log_std)
    I  off-policy, m = 379     1.2e-5   2.1e-5  (D190 A32 Gaussian, base.0.weight)
    W  m = 71                  3.7e-6   1.3e-5  (D348 A17 Gaussian, output bias)
    W  m = 7                   4.3e-6   6.6e-6
    C  m = 135                 1.1e-5   3.1e-5  (D8 A32 Gaussian, output bias)
    C  m = 7                   1.5e-5   1.5e-5  (D8 A32 Gaussian, actor_log_std)

Heads: within 3.9e-5 of float64 at the 230 logit gap (the float32 oracle: 3.0e-5), 6e-7 in the
sigma regimes; Gaussian draws within 1.3e-6 of the NumPy restatement.  Nothing missed a bound.
"""
import ctypes
import pathlib
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diamond
from diamond import _native as N
from diamond.engine import fused_shape_class
from oracle import ppo_np as P

import gpu_helpers as G
import wide_act_cases as W
import wide_large_cases as LC
import wide_mb_cases as C
from gpu_helpers import SpecEnvs, dev, hparams, stream, synth, to_device
from test_gpu_rollout_ckpt import oracle_gaussian_draws, philox4x32_10, u01
from test_gpu_wide_act import _bounds, _to_dev
from test_gpu_wide_mb import _check_minibatch, _check_records, _gradient, _plan, _prepare

GUARD = 64   # sentinel elements on each side of a guarded output


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _ids(cases):
    return [LC.case_id(c) for c in cases]


def _handle(case):
    _grp, _seed, Hd, D, A, cont, T, Nn, M, _mb = case
    return N.Handle(0, C.dims(Hd, D, A, cont, T, Nn, M))


# ---------------------------------------------------------------------------------------------
# 1. the predicate
# ---------------------------------------------------------------------------------------------
_CLASS = [(64, 129, 2, 1), (64, 384, 32, 1), (64, 376, 17, 1), (64, 348, 17, 1), (64, 8, 17, 1),
          (64, 32, 32, 1), (64, 128, 17, 1), (64, 136, 16, 1),
          (64, 385, 2, 1), (64, 8, 33, 1), (128, 129, 2, 1), (128, 8, 17, 1),
          (64, 376, 17, 2), (64, 8, 17, 2)]
_RAISES = [(64, 385, 2, 1), (64, 8, 33, 1), (128, 129, 2, 1), (128, 8, 17, 1)]


@pytest.mark.parametrize("Hd,D,A,world", _CLASS)
@pytest.mark.parametrize("cont", [False, True])
def test_python_and_c_agree_on_the_large_heads(Hd, D, A, world, cont):
    T, Nn = 4, 32
    want = fused_shape_class(Hd, D, A, world)
    assert want == ("wide" if LC.is_large(Hd, D, A) and world == 1 else None)
    assert ((Hd, D, A, world) in _RAISES) == (want is None and world == 1)
    for wide_ranks in (0, 1):
        h = N.Handle(0, N.Dims(T, Nn, D, A, int(cont), Hd, 1, 1, world, 0, 0, wide_ranks))
        assert h.fused_plan(T * Nn)["shape_class"] == \
            fused_shape_class(Hd, D, A, world, bool(wide_ranks)) == want
    if world != 1:
        return
    ro, _ = synth(T, Nn, D, A, cont, seed=1)
    pd = torch.zeros(h.layout.total, device=dev())
    hp = hparams()
    call = lambda: N.check(h.lib.dppo_prepare_f32(h.h, ctypes.byref(ro.as_struct()),
                                                  pd.data_ptr(), ctypes.byref(hp), None, stream()))
    if want is None:
        with pytest.raises(NotImplementedError):
            call()
    else:
        call()
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# 2. old-policy evaluation and records
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LC.sweep_cases(), ids=_ids(LC.sweep_cases()))
def test_old_policy_and_records_vs_oracle(case):
    """wide_eval_kernel (AB = 2 from 17 actions on) and wide_pack_kernel's record at every width
    and action case: four whole tiles, then B = 105 with a partial fourth."""
    _grp, _seed, _Hd, D, A, cont, *_ = case
    for t, n in LC.EVAL_TN:
        h = N.Handle(0, LC.eval_dims(D, A, cont, t, n))
        assert h.fused_plan(t * n)["shape_class"] == "wide"
        params, flat, host = LC.eval_inputs(case, t, n)
        _pd, _hp, o = _prepare(h, flat, host)
        for k, v in o.items():
            assert np.isfinite(v).all(), k
        _check_records(o, params, host, cont)


# ---------------------------------------------------------------------------------------------
# 3. minibatch gradient
# ---------------------------------------------------------------------------------------------
def _run(case, mb=None):
    _grp, seed, Hd, D, A, cont, T, Nn, M, m = case
    m = m if mb is None else mb
    h = _handle(case)
    tile, grid = _plan(h, m)
    _L, _names, _params, flat, host = C.inputs(seed, Hd, D, A, cont, T, Nn, M)
    pd, hp, o = _prepare(h, flat, host)
    _check_minibatch(h, case, pd, hp, o, C.minibatch_idx(seed, T * Nn, m))
    return tile, grid


@pytest.mark.parametrize("case", LC.cases_of("I"), ids=_ids(LC.cases_of("I")))
def test_every_new_instantiation_on_policy(case):
    """One shape per new wide_mb_kernel<64, CONT, NB1, false, AB> (wide_large_cases.nb1 / ab: not
    visible through the ABI): twelve tiles on six workgroups, the last tile partial."""
    tile, grid = _run(case)
    assert (tile, grid) == (C.S, 6)
    assert C.tiles_per_group(case[9], tile, grid) == (2, 2) and case[9] % tile != 0


@pytest.mark.parametrize("case", LC.cases_of("I"), ids=_ids(LC.cases_of("I")))
def test_every_new_instantiation_off_policy(case):
    """The same eighteen with the parameters moved after prepare(): the old log-probs are the old
    parameters', so the ratio leaves 1 and every branch of the clipped surrogate carries samples."""
    _grp, seed, Hd, D, A, cont, T, Nn, M, m = case
    h = _handle(case)
    assert _plan(h, m) == (C.S, 6)
    L, names, _params, flat, host = C.inputs(seed, Hd, D, A, cont, T, Nn, M)
    _pd, hp, o = _prepare(h, flat, host)
    new, new_flat = LC.offpolicy_params(case)
    idx, reg = LC.offpolicy_idx(case, new, o)
    assert idx.size == m and (reg >= 0).all() and (reg == 0).any() and (reg > 0).any()
    got, loss4 = _gradient(h, torch.from_numpy(new_flat).to(dev()), hp, idx)
    ref64 = C.oracle_gradient(new, host, cont, o, idx, np.float64)
    C.check_gradient(L, names, got, loss4, ref64, f"off-policy {LC.case_id(case)}")
    want = C.loss_terms(ref64)
    for k in (1, 2):   # the policy and value terms too, as tests/test_gpu_offpolicy.py
        assert abs(loss4[k] - want[k]) <= 2e-5 * max(1.0, abs(want[k])), (tuple(loss4), want)


@pytest.mark.parametrize("case", LC.cases_of("W"), ids=_ids(LC.cases_of("W")))
def test_first_layer_widths(case):
    """D on each side of a 16-column block boundary of every new NB1 and the Humanoid widths, 17
    actions: one workgroup with three tiles."""
    assert _run(case) == (C.S, 1)


@pytest.mark.parametrize("case", LC.cases_of("C"), ids=_ids(LC.cases_of("C")))
def test_action_counts(case):
    """A around the second block of 16 at D = 136 and D = 8: five tiles, a workgroup with three and
    one with two."""
    tile, grid = _run(case)
    assert (tile, grid) == (C.S, 2) and C.tiles_per_group(case[9], tile, grid) == (2, 3)


@pytest.mark.parametrize("case", LC.sweep_cases(), ids=_ids(LC.sweep_cases()))
def test_one_partial_tile(case):
    assert _run(case, LC.TINY_MB) == (C.S, 1)


@pytest.mark.parametrize("case", [LC.cases_of("W")[11], LC.cases_of("C")[10]],
                         ids=_ids([LC.cases_of("W")[11], LC.cases_of("C")[10]]))
def test_two_launches_give_the_same_bits(case):
    _grp, seed, Hd, D, A, cont, T, Nn, M, _m = case
    assert (D, A, cont) in ((376, 17, True), (136, 32, False))
    h = _handle(case)
    _L, _names, _params, flat, host = C.inputs(seed, Hd, D, A, cont, T, Nn, M)
    pd, hp, _o = _prepare(h, flat, host)
    idx = C.minibatch_idx(seed, T * Nn, LC.MB)
    g1, l1 = _gradient(h, pd, hp, idx)
    g2, l2 = _gradient(h, pd, hp, idx)
    assert np.isfinite(g1).all() and np.any(g1 != 0)
    assert np.array_equal(g1, g2) and l1 == l2


# ---------------------------------------------------------------------------------------------
# 4. learn() through the public classes
# ---------------------------------------------------------------------------------------------
def _agent(D, A, cont):
    Cfg = diamond.ContinuousPPOConfig if cont else diamond.PPOConfig
    Agent = diamond.ContinuousPPO if cont else diamond.PPO
    cfg = Cfg(rollout_steps=LC.LEARN_T, num_envs=LC.LEARN_N, num_epochs=LC.LEARN_E,
              num_minibatches=LC.LEARN_M, verbose=False)
    assert cfg.network_hidden_dim == LC.HID
    return Agent(None, cfg, envs=SpecEnvs(D, A, cont)), cfg


def _state(agent):
    out = [p.detach().cpu().numpy().ravel() for p in agent.network.parameters()]
    for p in agent.network.parameters():
        s = agent.optimizer.state[p]
        out += [s["exp_avg"].cpu().numpy().ravel(), s["exp_avg_sq"].cpu().numpy().ravel()]
    return np.concatenate(out)


@pytest.mark.parametrize("D,A,cont", LC.LEARN_SHAPES, ids=[LC.shape_id(s) for s in LC.LEARN_SHAPES])
def test_learn_vs_oracle_and_checkpoint_round_trip(D, A, cont):
    """The default network at a Humanoid shape is fused: E x M = 8 Adam steps of the wide kernels
    against the oracle's learn (the bounds of test_ragged_learn_vs_oracle); then a checkpoint
    save / load / next-learn round trip continues bit-identically."""
    T, Nn, E, M = LC.LEARN_T, LC.LEARN_N, LC.LEARN_E, LC.LEARN_M
    torch.manual_seed(21)
    a1, cfg = _agent(D, A, cont)
    L = a1._learner
    assert L.fused and L.shape_class == "wide" and not L.fused_act
    names = [n for n, _ in a1.network.named_parameters()]
    params = {n: p.detach().cpu().numpy().copy() for n, p in a1.network.named_parameters()}
    seed = 900 + D + A
    ro, host = synth(T, Nn, D, A, cont, seed)
    np.random.seed(seed)
    st = np.random.get_state()
    a1.learn_device(ro)
    tr = a1.learn_trace()
    torch.cuda.synchronize()
    after = np.random.get_state()
    np.random.set_state(st)
    adam = P.new_adam_state(params, names)
    ref = P.learn(params, adam, list(host), P.Hyper(num_epochs=E, num_minibatches=M), cfg.lr, cont,
                  rng=np.random)
    assert len(ref["loss"]) == E * M == tr.shape[0]
    np.testing.assert_allclose(tr[:, 0], ref["loss"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(tr[:, 4], ref["norm"], rtol=1e-4, atol=1e-5)
    for n, p in a1.network.named_parameters():
        np.testing.assert_allclose(p.detach().cpu().numpy(), params[n], rtol=0, atol=2e-5,
                                   err_msg=n)
    # checkpoint round trip
    with tempfile.TemporaryDirectory() as d:
        a1.checkpointer.folder = pathlib.Path(d)
        a1.checkpointer.save(1, a1.network, a1.optimizer)
        path = sorted(pathlib.Path(d).glob("*.pt"))[0]
        a2, _ = _agent(D, A, cont)
        a2.load_checkpoint(path)
    assert a2._learner.shape_class == "wide"
    assert np.array_equal(_state(a1), _state(a2))
    np.random.set_state(after)
    a1.learn_device(ro)
    np.random.set_state(after)
    a2.learn_device(ro)
    torch.cuda.synchronize()
    s1, s2 = _state(a1), _state(a2)
    assert np.isfinite(s1).all() and np.array_equal(s1, s2)


# ---------------------------------------------------------------------------------------------
# 5. the rollout sampler
# ---------------------------------------------------------------------------------------------
def _act_handle(D, A, cont):
    h = N.Handle(0, W.dims(LC.HID, D, A, cont))
    assert h.fused_plan(32)["shape_class"] == "wide"
    return h


def _guarded(shape, dtype, fill):
    """(the whole buffer, the view a kernel writes) with GUARD sentinels on each side"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev())
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_intact(buf, fill):
    b = buf.cpu().numpy()
    for edge in (b[:GUARD], b[-GUARD:]):
        assert np.all(np.isnan(edge)) if isinstance(fill, float) and np.isnan(fill) \
            else np.all(edge == fill)


def _heads(h, pd, od, n, A):
    buf, out = _guarded((n, A), torch.float32, float("nan"))
    N.check(h.lib.dppo_actor_forward_f32(h.h, pd.data_ptr(), od.data_ptr(), n, out.data_ptr(),
                                         stream()))
    torch.cuda.synchronize()
    _guards_intact(buf, float("nan"))
    return out.cpu().numpy()


def _act(h, pd, od, n, A, cont, seed, counter):
    if cont:
        buf, act = _guarded((n, A), torch.float32, float("nan"))
    else:
        buf, act = _guarded((n,), torch.int32, -7)
    N.check(h.lib.dppo_act_f32(h.h, pd.data_ptr(), od.data_ptr(), n, seed, counter,
                               act.data_ptr(), stream()))
    torch.cuda.synchronize()
    _guards_intact(buf, float("nan") if cont else -7)
    return act.cpu().numpy()


def _act_squash(h, pd, od, n, A, seed, counter, lo, hi):
    ubuf, u = _guarded((n, A), torch.float32, float("nan"))
    ebuf, env = _guarded((n, A), torch.float32, float("nan"))
    N.check(h.lib.dppo_act_squash_f32(
        h.h, pd.data_ptr(), od.data_ptr(), n, seed, counter,
        None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data,
        u.data_ptr(), env.data_ptr(), stream()))
    torch.cuda.synchronize()
    _guards_intact(ubuf, float("nan"))
    _guards_intact(ebuf, float("nan"))
    return u.cpu().numpy(), env.cpu().numpy()


@pytest.mark.parametrize("shape", LC.ACT_SHAPES, ids=LC.shape_id)
def test_actor_heads_vs_float64(shape):
    D, A, cont = shape
    n = LC.ACT_N
    params, flat, obs = LC.act_inputs(D, A, cont)
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    want = P.forward(p64, obs, cont, np.float64)["out"]
    got = _heads(_act_handle(D, A, cont), _to_dev(flat), _to_dev(obs), n, A)
    print(f"{LC.shape_id(shape)}: max |heads - f64| {np.abs(got - want).max():.3g}")
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=2e-5)


def _check_squash(h, pd, od, n, A, u):
    """Both squash modes on the kernel's own draws, per-dim bounds, the cap at `high`"""
    lo, hi = _bounds(A)
    assert len(set(lo)) == A and len(set(hi)) == A   # per-dim: a swapped dim would show
    for bounded in (False, True):
        u2, env = _act_squash(h, pd, od, n, A, LC.SEED, LC.COUNTER, lo if bounded else None,
                              hi if bounded else None)
        assert np.array_equal(u2, u)   # bit for bit the plain call's draws
        if bounded:
            env_own = P.squash_action(u2, lo.astype(np.float64), hi.astype(np.float64))
            assert np.all(env >= lo) and np.all(env <= hi)
            atol = float(4e-7 * (1 + np.abs(lo).max()))
        else:
            env_own = np.tanh(u2.astype(np.float64))
            assert np.all(np.abs(env) <= 1.0)
            atol = 4e-7
        np.testing.assert_allclose(env, env_own, rtol=0, atol=atol)


@pytest.mark.parametrize("shape", LC.GAUSS_DRAW_SHAPES, ids=LC.shape_id)
def test_gaussian_draws_and_squash(shape):
    """A = 17 and 32: the Philox blocks of dims 16 .. 31 (k0 << 24 in the counter's high sample
    word) against the NumPy restatement; the first 16 dims draw what they drew before."""
    D, A, cont = shape
    n = LC.ACT_N
    params, flat, obs = LC.act_inputs(D, A, cont)
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    out = P.forward(p64, obs, True, np.float64)["out"]
    h, pd, od = _act_handle(D, A, cont), _to_dev(flat), _to_dev(obs)
    u = _act(h, pd, od, n, A, True, LC.SEED, LC.COUNTER)
    want = oracle_gaussian_draws(out, params["actor_log_std"], LC.SEED, LC.COUNTER)
    print(f"{LC.shape_id(shape)}: max |u - oracle| {np.abs(u - want).max():.3g}")
    np.testing.assert_allclose(u, want, rtol=1e-4, atol=1e-4)
    _check_squash(h, pd, od, n, A, u)


def test_squash_caps_at_high():
    """Draws far in tanh's upper tail (sigma 4.5 and a mean pushed to +40 sigma by the output
    bias) land on `high` itself in every one of 32 dims, never an ulp above."""
    D, A = 136, 32
    params, _flat, obs = LC.act_inputs(D, A, True)
    params = {k: np.array(v) for k, v in params.items()}
    params["actor_log_std"][:] = 1.5
    params["actor_mean_head.2.bias"][:] = 180.0
    L = N.param_layout(W.dims(LC.HID, D, A, True))
    flat = G.flat32(L, P.CONTINUOUS_NAMES, params)
    lo, hi = _bounds(A)
    h = _act_handle(D, A, True)
    u, env = _act_squash(h, _to_dev(flat), _to_dev(obs), LC.ACT_N, A, LC.SEED, LC.COUNTER, lo, hi)
    assert u.min() > 20.0   # tanhf(u) == 1 in float32
    # without the cap, float32 low + 2 * ((high - low) / 2) is above `high` in some of the dims
    uncapped = lo + np.float32(2) * (np.float32(0.5) * (hi - lo))
    assert (uncapped > hi).any()
    assert np.all(env <= hi) and np.all(env >= lo)
    np.testing.assert_allclose(env, np.broadcast_to(hi, env.shape), rtol=0,
                               atol=float(4e-7 * (1 + np.abs(lo).max())))
    assert np.array_equal(env[:, uncapped > hi], np.broadcast_to(hi, env.shape)[:, uncapped > hi])


def test_categorical_draws_reach_the_second_block_and_the_last_action():
    D, A, cont = LC.CAT_DRAW_SHAPE
    params, flat, obs = LC.peaked_last_inputs()
    n = obs.shape[0]
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    out = P.forward(p64, obs, False, np.float64)["out"]
    got = _act(_act_handle(D, A, cont), _to_dev(flat), _to_dev(obs), n, A, False, LC.SEED,
               LC.COUNTER)
    want, clear = W.categorical_oracle(out, LC.SEED, LC.COUNTER, philox4x32_10, u01)
    assert clear.mean() >= W.MIN_CLEAR
    assert got.min() >= 0 and got.max() == A - 1
    assert ((got >= 16) & (got < A - 1)).any() and (got < 16).any()
    assert np.array_equal(got[clear], want[clear])


@pytest.mark.parametrize("shape", [s for s in LC.ACT_SHAPES if not s[2]], ids=LC.shape_id)
def test_categorical_draws_are_the_documented_stream(shape):
    D, A, cont = shape
    params, flat, obs = LC.act_inputs(D, A, cont)
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    out = P.forward(p64, obs, False, np.float64)["out"]
    got = _act(_act_handle(D, A, cont), _to_dev(flat), _to_dev(obs), LC.ACT_N, A, False, LC.SEED,
               LC.COUNTER)
    want, clear = W.categorical_oracle(out, LC.SEED, LC.COUNTER, philox4x32_10, u01)
    assert clear.mean() >= W.MIN_CLEAR
    assert got.min() >= 0 and got.max() < A
    assert np.array_equal(got[clear], want[clear])


@pytest.mark.parametrize("shape", LC.GRID_STRIDE_SHAPES, ids=LC.shape_id)
def test_every_workgroup_takes_a_second_tile(shape):
    """n = 32 CUs + 7: the grid is capped at the CU count, so every workgroup strides to a second
    tile (the last one partial)."""
    D, A, cont = shape
    n = W.real_n(W.BIG, _cus())
    params, flat, obs = LC.act_inputs(D, A, cont, n)
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    out = P.forward(p64, obs, cont, np.float64)["out"]
    h, pd, od = _act_handle(D, A, cont), _to_dev(flat), _to_dev(obs)
    np.testing.assert_allclose(_heads(h, pd, od, n, A), out, rtol=2e-5, atol=2e-5)
    got = _act(h, pd, od, n, A, cont, LC.SEED, LC.COUNTER)
    if cont:
        want = oracle_gaussian_draws(out, params["actor_log_std"], LC.SEED, LC.COUNTER)
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)
    else:
        want, clear = W.categorical_oracle(out, LC.SEED, LC.COUNTER, philox4x32_10, u01)
        assert clear.mean() >= W.MIN_CLEAR
        assert got.min() >= 0 and got.max() == A - 1
        assert np.array_equal(got[clear], want[clear])


def test_learner_act_serves_32_action_dims():
    """NativeLearner.act / the squashing sampler at 32 Gaussian dims, through the public class"""
    D, A, n = 136, 32, 33
    cfg = diamond.ContinuousPPOConfig(rollout_steps=4, num_envs=32, verbose=False)
    agent = diamond.ContinuousPPO(None, cfg, envs=SpecEnvs(D, A, True))
    L = agent._learner
    assert L.shape_class == "wide" and not L.fused_act and not L.wide_act
    obs = np.random.default_rng(5).standard_normal((n, D), dtype=np.float32)
    with pytest.raises(RuntimeError):
        L.act(obs, 9)
    L.wide_act = True
    seed = 0x0123_4567_89AB_CDEF
    a0 = L.act(obs, seed)
    lo, hi = _bounds(A)
    u1, env1 = L.act(obs, seed, squash=(lo, hi))
    assert a0.dtype == np.float32 and a0.shape == (n, A) and L._act_counter == 2
    od = _to_dev(obs)
    assert np.array_equal(a0, _act(L.handle, L.flat.flat, od, n, A, True, seed, 0))
    assert np.array_equal(u1, _act(L.handle, L.flat.flat, od, n, A, True, seed, 1))
    env_own = P.squash_action(u1, lo.astype(np.float64), hi.astype(np.float64))
    np.testing.assert_allclose(env1, env_own, rtol=0, atol=float(4e-7 * (1 + np.abs(lo).max())))


# ---------------------------------------------------------------------------------------------
# 6. regimes
# ---------------------------------------------------------------------------------------------
def test_sampler_with_peaked_logits():
    """32 actions, a logit gap of 230: exp(logit - max) underflows for most actions.  The heads
    keep the regimes' per-element bound and every clear draw is the float64 inverse CDF's."""
    params, flat, obs, cont = LC.regime_sampler_inputs("peaked")
    D, A, _ = LC.PEAKED_SHAPE
    n = obs.shape[0]
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    out64 = P.forward(p64, obs, False, np.float64)["out"]
    out32 = P.forward(params, obs, False)["out"]
    assert (out64.max(1) - out64.min(1)).max() > 229
    h, pd, od = _act_handle(D, A, cont), _to_dev(flat), _to_dev(obs)
    d, d32 = G._within(_heads(h, pd, od, n, A), out64, out32, "heads")
    print(f"REGIME sampler peaked230 A32: max |heads - f64| {d:.3g}, oracle32 {d32:.3g}")
    got = _act(h, pd, od, n, A, False, LC.SEED, LC.COUNTER)
    want, clear = W.categorical_oracle(out64, LC.SEED, LC.COUNTER, philox4x32_10, u01)
    assert clear.mean() >= W.MIN_CLEAR
    assert got.min() >= 0 and got.max() < A
    assert np.array_equal(got[clear], want[clear])


@pytest.mark.parametrize("name", sorted(LC.SIGMA_LOG_STD))
def test_sampler_with_narrow_and_wide_sigma(name):
    params, flat, obs, cont = LC.regime_sampler_inputs(name)
    D, A, _ = LC.SIGMA_SHAPE
    n = obs.shape[0]
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    out64 = P.forward(p64, obs, True, np.float64)["out"]
    out32 = P.forward(params, obs, True)["out"]
    h, pd, od = _act_handle(D, A, cont), _to_dev(flat), _to_dev(obs)
    d, d32 = G._within(_heads(h, pd, od, n, A), out64, out32, "heads")
    print(f"REGIME sampler {name} A17: max |heads - f64| {d:.3g}, oracle32 {d32:.3g}")
    u = _act(h, pd, od, n, A, True, LC.SEED, LC.COUNTER)
    want = oracle_gaussian_draws(out64, params["actor_log_std"], LC.SEED, LC.COUNTER)
    np.testing.assert_allclose(u, want, rtol=1e-4, atol=1e-4)
    if name == "sigma4.5":
        assert (np.abs(u) > 3).any()   # tanh's tails are hit
    _check_squash(h, pd, od, n, A, u)
