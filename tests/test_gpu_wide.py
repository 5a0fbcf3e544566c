"""GPU checks of the wide kernel family (csrc/mbwide.hip): the fused learn() of the default
network at hidden 128 (obs_dim <= 128) and at hidden 64 with 32 < obs_dim <= 128.

* one minibatch gradient through dppo_minibatch_grad_f32 against the NumPy oracle evaluated in
  float64 (reference ppo.py:261-283, continuous_ppo.py:273-295), with the bounds of
  tests/test_gpu_shapes.py: within 2e-5 * max|g| overall, each tensor within 1e-4 of its own
  scale (floored at 1e-3 * max|g|), loss and entropy within 2e-5;
* prepare(): old-policy log-probs / values / next-values against the oracle (rtol = atol = 2e-5),
  returns bit-equal to values + GAE on the kernel's own values, normalised advantages within 2e-6
  (the assertions of test_full_size_old_policy_and_records_vs_oracle);
* the whole learn() through the public API against the oracle's learn (test_gpu_production's
  learn_vs_oracle bounds), bit-reproducibility, the rollout / checkpoint / act() surface, the
  DPPO_WIDE=0 escape hatch, and shapes of neither class staying unsupported.
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
from diamond.engine import DeviceRollout
from oracle import ppo_np as P

from conftest import GOLDEN, PKG, ROOT
from gpu_helpers import SpecEnvs, dev, hparams, random_params, stream, synth


def wide_plan(Hd, D, A, cont, T, Nn, M, m):
    """(tile, grid) the library itself plans for a minibatch of m samples at this shape
    (dppo_fused_plan: mbwide.hip's own S and wide_grid, not a restatement)."""
    h = N.Handle(0, N.Dims(T, Nn, D, A, int(cont), Hd, 4, M, 1, 0))
    p = h.fused_plan(m)
    assert p["shape_class"] == "wide"
    return p["tile"], p["grid"]


def wide_tiles_per_group(m, tile, grid):
    """(fewest, most) tiles any workgroup runs: workgroup b takes tiles b, b + grid, ..."""
    tiles = (m + tile - 1) // tile
    return tiles // grid, (tiles + grid - 1) // grid


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _prepare(h, D, A, cont, T, Nn, seed, ro=None, host=None):
    B = T * Nn
    L = h.layout
    names = P.CONTINUOUS_NAMES if cont else P.DISCRETE_NAMES
    params, flat = random_params(L, names, D, A, cont, np.random.default_rng(1000 + seed))
    if ro is None:
        ro, host = synth(T, Nn, D, A, cont, seed=2000 + seed)
    pd = torch.from_numpy(flat).to(dev())
    keys = ("log_probs", "values", "next_values", "advantages", "returns")
    outs = {k: torch.empty(B, device=dev()) for k in keys}
    lo = N.LearnOutputs(*[outs[k].data_ptr() for k in keys])
    hp = hparams()
    N.check(h.lib.dppo_prepare_f32(h.h, ctypes.byref(ro.as_struct()), pd.data_ptr(),
                                   ctypes.byref(hp), ctypes.byref(lo), stream()))
    torch.cuda.synchronize()
    return params, names, pd, hp, host, {k: v.cpu().numpy() for k, v in outs.items()}


def _check(i, Hd, D, A, cont, T, Nn, M, mb):
    """test_gpu_shapes._check with the hidden width as a parameter and an explicit size."""
    B = T * Nn
    h = N.Handle(0, N.Dims(T, Nn, D, A, int(cont), Hd, 4, M, 1, 0))
    L = h.layout
    params, names, pd, hp, host, o = _prepare(h, D, A, cont, T, Nn, i)
    idx = np.random.RandomState(3000 + i).permutation(B)[:mb].astype(np.int32)
    idx_d = torch.from_numpy(idx).to(dev())
    g = torch.zeros(L.total, device=dev())
    loss4 = (ctypes.c_float * 4)()
    N.check(h.lib.dppo_minibatch_grad_f32(h.h, pd.data_ptr(), idx_d.data_ptr(), mb, mb,
                                          ctypes.byref(hp), g.data_ptr(), loss4, stream()))
    torch.cuda.synchronize()
    got_flat = g.cpu().numpy()
    got = np.concatenate([got_flat[L.offset[k]:L.offset[k] + L.numel[k]] for k in range(L.count)])
    obs, _, act, *_ = host
    obs_f = obs.reshape(B, D)
    act_f = act.reshape(B, A) if cont else act.reshape(B)
    args = (obs_f[idx], act_f[idx], o["log_probs"][idx], o["advantages"][idx], o["returns"][idx])
    loss, comps, grads = P.minibatch_loss_grads(params, *args, P.Hyper(), cont, dt=np.float64)
    exact = np.concatenate([np.asarray(grads[n], np.float64).ravel() for n in names])
    scale = np.abs(exact).max()
    print(f"H={Hd} D={D} A={A} cont={cont} mb={mb}: overall {np.abs(got - exact).max() / scale:.3g}")
    assert np.abs(got - exact).max() <= 2e-5 * scale, np.abs(got - exact).max() / scale
    for k, n in enumerate(names):
        a = got[sum(L.numel[j] for j in range(k)):][:L.numel[k]]
        b = exact[sum(L.numel[j] for j in range(k)):][:L.numel[k]]
        s = max(np.abs(b).max(), 1e-3 * scale)
        print(f"  {n}: {np.abs(a - b).max() / s:.3g}")
        assert np.abs(a - b).max() <= 1e-4 * s, (n, np.abs(a - b).max() / s)
    assert abs(loss4[0] - loss) <= 2e-5 * max(1.0, abs(loss)), (loss4[0], loss)
    assert abs(loss4[3] - comps["entropy"]) <= 2e-5 * max(1.0, abs(comps["entropy"]))


_SHAPES = [(128, 4, 2, False), (128, 1, 2, False), (128, 8, 4, False), (128, 17, 6, True),
           (128, 33, 3, True), (128, 105, 8, True), (128, 128, 16, False), (128, 128, 16, True),
           (128, 30, 1, True), (64, 33, 2, False), (64, 40, 5, False), (64, 105, 8, True),
           (64, 128, 16, False), (64, 128, 16, True)]


@pytest.mark.parametrize("j,Hd,D,A,cont", [(j, *s) for j, s in enumerate(_SHAPES)])
def test_wide_minibatch_gradient_vs_oracle(j, Hd, D, A, cont):
    T, Nn, M, ragged = 16, 96, 4, 5
    _check(j, Hd, D, A, cont, T, Nn, M, T * Nn // M - ragged)


@pytest.mark.parametrize("Hd,D,A,cont", [(128, 8, 4, False), (128, 17, 6, True)])
@pytest.mark.parametrize("mb", [1, 7])
def test_wide_minibatch_smaller_than_a_tile(Hd, D, A, cont, mb):
    """1 and 7 samples: less than one tile, idle sample slots in every wave."""
    _check(50 + mb, Hd, D, A, cont, 16, 96, 4, mb)


@pytest.mark.parametrize("Hd,D,A,cont", [(128, 8, 4, False), (128, 17, 6, True)])
def test_wide_minibatch_two_tiles_per_workgroup_last_partial(Hd, D, A, cont):
    """Sized from the kernel's own tile and grid (dppo_fused_plan): every workgroup accumulates
    at least two tiles in its registers, more than one workgroup runs, and the last tile is
    partial."""
    T, Nn, M = 16, 96, 1
    mb = T * Nn - 5
    tile, grid = wide_plan(Hd, D, A, cont, T, Nn, M, mb)
    assert 1 < grid <= _cus()
    assert wide_tiles_per_group(mb, tile, grid)[0] >= 2
    assert mb % tile != 0
    _check(60, Hd, D, A, cont, T, Nn, M, mb)


# ---------------------------------------------------------------------------------------------
def _chained_rollout(T, Nn, D, A, cont, seed):
    """A rollout whose next_obs[t] is obs[t + 1] except where an episode ended (about 3 % of the
    rows) and in the last step: the layout a vector env produces."""
    ro, host = synth(T, Nn, D, A, cont, seed)
    obs, nobs, act, rew, te, tr = host
    rng = np.random.default_rng(seed + 1)
    keep = rng.random((T - 1, Nn)) < 0.03
    nobs = nobs.copy()
    nobs[:-1] = np.where(keep[..., None], nobs[:-1], obs[1:])
    g = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev())
    return (DeviceRollout(g(obs), g(nobs), g(act), g(rew), g(te), g(tr)),
            (obs, nobs, act, rew, te, tr))


@pytest.mark.parametrize("Hd,D,A,cont,chained", [
    (128, 8, 4, False, False), (128, 105, 8, True, False), (64, 128, 16, False, False),
    (128, 8, 4, False, True)])
def test_wide_old_policy_and_records_vs_oracle(Hd, D, A, cont, chained):
    T, Nn = 16, 160
    h = N.Handle(0, N.Dims(T, Nn, D, A, int(cont), Hd, 4, 4, 1, 0))
    ro = host = None
    if chained:
        ro, host = _chained_rollout(T, Nn, D, A, cont, 77)
    params, names, pd, hp, host, o = _prepare(h, D, A, cont, T, Nn, 7, ro, host)
    obs, nobs, act, rew, te, tr = host
    logp, v, nv, _ = P.old_policy(params, obs, act, nobs, cont)
    np.testing.assert_allclose(o["log_probs"], logp.ravel(), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(o["values"], v.ravel(), rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(o["next_values"], nv.ravel(), rtol=2e-5, atol=2e-5)
    vals = o["values"].reshape(T, Nn)
    adv = P.gae(rew, te, tr, vals, o["next_values"].reshape(T, Nn))
    assert np.array_equal(o["returns"].reshape(T, Nn), vals + adv)
    np.testing.assert_allclose(o["advantages"], P.normalize_adv(adv).ravel(), rtol=0, atol=2e-6)


# ---------------------------------------------------------------------------------------------
def _agent(Hd, D, A, cont, T=16, Nn=256, envs=None, **kw):
    Cfg = diamond.ContinuousPPOConfig if cont else diamond.PPOConfig
    Agent = diamond.ContinuousPPO if cont else diamond.PPO
    cfg = Cfg(network_hidden_dim=Hd, rollout_steps=T, num_envs=Nn, verbose=False, **kw)
    return Agent(None, cfg, envs=envs if envs is not None else SpecEnvs(D, A, cont)), cfg


@pytest.mark.parametrize("Hd,D,A,cont", [(128, 8, 4, False), (128, 17, 6, True),
                                         (128, 128, 16, False), (128, 128, 16, True),
                                         (64, 105, 8, True)])
def test_wide_learn_vs_oracle(Hd, D, A, cont):
    """learn_vs_oracle (tests/test_gpu_production.py) at wide shapes: 32 Adam steps."""
    T, Nn = 16, 256
    agent, cfg = _agent(Hd, D, A, cont, T, Nn)
    assert agent._learner.fused
    assert agent._learner.shape_class == "wide"
    assert not agent._learner.fused_act
    names = [n for n, _ in agent.network.named_parameters()]
    params = {n: p.detach().cpu().numpy().copy() for n, p in agent.network.named_parameters()}
    seed = Hd + D
    ro, host = synth(T, Nn, D, A, cont, seed)
    np.random.seed(seed)
    st = np.random.get_state()
    agent.learn_device(ro)
    tr = agent.learn_trace()
    torch.cuda.synchronize()
    np.random.set_state(st)
    adam = P.new_adam_state(params, names)
    ref = P.learn(params, adam, list(host), P.Hyper(), cfg.lr, cont, rng=np.random)
    np.testing.assert_allclose(tr[:, 0], ref["loss"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(tr[:, 4], ref["norm"], rtol=1e-4, atol=1e-5)
    for n, p in agent.network.named_parameters():
        np.testing.assert_allclose(p.detach().cpu().numpy(), params[n], rtol=0, atol=2e-5,
                                   err_msg=n)


def _state(agent):
    out = [p.detach().cpu().numpy().ravel() for p in agent.network.parameters()]
    for p in agent.network.parameters():
        s = agent.optimizer.state[p]
        out += [s["exp_avg"].cpu().numpy().ravel(), s["exp_avg_sq"].cpu().numpy().ravel()]
    return np.concatenate(out)


@pytest.mark.parametrize("Hd,D,A,cont", [(128, 17, 6, True), (64, 40, 5, False)])
def test_wide_learn_is_deterministic(Hd, D, A, cont):
    """Two agents from the same seed, three learns each on the same rollout: parameters and Adam
    moments bit-identical (fixed-order sums, no float atomics)."""
    T, Nn = 16, 256
    ro, _ = synth(T, Nn, D, A, cont, 5)
    res = []
    for _ in range(2):
        torch.manual_seed(11)
        np.random.seed(11)
        agent, _cfg = _agent(Hd, D, A, cont, T, Nn)
        assert agent._learner.shape_class == "wide"
        np.random.seed(12)
        for _k in range(3):
            agent.learn_device(ro)
        torch.cuda.synchronize()
        res.append(_state(agent))
    assert np.array_equal(res[0], res[1])
    assert np.all(np.isfinite(res[0]))


# ---------------------------------------------------------------------------------------------
def _stub_agent(Hd=128, D=8, A=4, T=16, Nn=32):
    import gym_stub
    envs = gym_stub.SyncVectorEnv([lambda: gym_stub.SyntheticEnv(D, A)] * Nn)
    agent, _ = _agent(Hd, D, A, False, T, Nn, envs=envs)
    return agent


def test_wide_rollout_checkpoint_and_act_surface():
    """rollout() samples with network.get_actions and stages the steps for learn(); a checkpoint
    save / load_checkpoint / next-learn round trip is bit-identical to the uninterrupted agent;
    act() is not offered for the wide class."""
    import pathlib
    import tempfile
    torch.manual_seed(3)
    np.random.seed(3)
    a1 = _stub_agent()
    L = a1._learner
    assert L.fused and L.shape_class == "wide" and not L.fused_act
    with pytest.raises(RuntimeError):
        L.act(np.zeros((32, 8), np.float32), 1)
    before = _state(a1)
    a1.current_observations, _ = a1.envs.reset(seed=5)
    exp = a1.rollout()
    assert len(exp) == 16 and exp[0][2].shape == (32,)
    a1.learn(exp)
    torch.cuda.synchronize()
    after = _state(a1)
    assert np.all(np.isfinite(after)) and not np.array_equal(before, after)
    with tempfile.TemporaryDirectory() as d:
        a1.checkpointer.folder = pathlib.Path(d)
        a1.checkpointer.save(1, a1.network, a1.optimizer)
        path = sorted(pathlib.Path(d).glob("*.pt"))[0]
        a2 = _stub_agent()
        a2.load_checkpoint(path)
    exp_h = [[np.array(x) for x in row] for row in exp]
    st = np.random.get_state()
    a1.learn(exp_h)
    np.random.set_state(st)
    a2.learn([[np.array(x) for x in row] for row in exp_h])
    torch.cuda.synchronize()
    assert np.array_equal(_state(a1), _state(a2))
    for p1, p2 in zip(a1.network.parameters(), a2.network.parameters()):
        assert float(a1.optimizer.state[p1]["step"]) == float(a2.optimizer.state[p2]["step"])


_CHILD = r"""
import sys
sys.path[:0] = {paths!r}
import numpy as np, torch
import diamond
from gpu_helpers import SpecEnvs, synth
cfg = diamond.PPOConfig(network_hidden_dim=128, rollout_steps=16, num_envs=64, verbose=False)
agent = diamond.PPO(None, cfg, envs=SpecEnvs(8, 4, False))
L = agent._learner
assert L.fused is False and L.shape_class is None and not L.fused_act, (L.fused, L.shape_class)
before = np.concatenate([p.detach().cpu().numpy().ravel() for p in agent.network.parameters()])
ro, _ = synth(16, 64, 8, 4, False, 1)
np.random.seed(0)
agent.learn_device(ro)
torch.cuda.synchronize()
after = np.concatenate([p.detach().cpu().numpy().ravel() for p in agent.network.parameters()])
assert np.all(np.isfinite(after)) and not np.array_equal(before, after)
agent.close()   # release the device workspace before the interpreter starts tearing down
print("GENERIC-OK", flush=True)
"""


def test_dppo_wide_0_takes_the_generic_path():
    """DPPO_WIDE=0 (set before the process starts): the same config is not fused and learns."""
    env = dict(os.environ, DPPO_WIDE="0")
    paths = [ROOT, PKG, GOLDEN, os.path.join(ROOT, "tests")]
    r = subprocess.run([sys.executable, "-c", _CHILD.format(paths=paths)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "GENERIC-OK" in r.stdout, r.stdout + r.stderr


_CLASS_SHAPES = [(64, 32, 16, 1), (128, 1, 2, 1), (128, 128, 16, 1), (64, 33, 2, 1),
                 (64, 128, 16, 1), (128, 129, 2, 1), (256, 8, 4, 1), (96, 8, 4, 1), (128, 8, 17, 1),
                 (128, 8, 4, 2), (64, 8, 4, 2)]


@pytest.mark.parametrize("Hd,D,A,world", _CLASS_SHAPES)
@pytest.mark.parametrize("cont", [False, True])
def test_python_and_c_shape_classes_agree(Hd, D, A, world, cont):
    """engine.fused_shape_class and dppo_create hold the same predicate: the class a handle
    reports (dppo_fused_plan) is the one Python computes, and on one rank dppo_prepare_f32 runs
    exactly where a class applies and raises NotImplementedError elsewhere."""
    from diamond.engine import fused_shape_class
    T, Nn = 4, 32
    h = N.Handle(0, N.Dims(T, Nn, D, A, int(cont), Hd, 1, 1, world, 0))
    want = fused_shape_class(Hd, D, A, world)
    assert h.fused_plan(T * Nn)["shape_class"] == want
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


def test_hidden_256_stays_unsupported():
    T, Nn, D, A = 16, 64, 8, 4
    h = N.Handle(0, N.Dims(T, Nn, D, A, 0, 256, 4, 4, 1, 0))
    ro, _ = synth(T, Nn, D, A, False, seed=1)
    pd = torch.zeros(h.layout.total, device=dev())
    hp = hparams()
    with pytest.raises(NotImplementedError):
        N.check(h.lib.dppo_prepare_f32(h.h, ctypes.byref(ro.as_struct()), pd.data_ptr(),
                                       ctypes.byref(hp), None, stream()))
