"""RecurrentContinuousPPO.learn() and rollout() against tests/gru_gauss_oracle.py: the comparisons
and bounds of tests/test_gpu_gru_wide_learn.py on (T, N, D, A) = (8, 20, 8, 3) at every G and
(8, 9, 100, 6) at G = 32 with wide_observations; 2 epochs x 2 minibatches, two learn() calls
under a decaying LR.  Both paths, the fused kernel (fused_gru=True) and torch autograd
(fused_gru=False, also with fused_loss and with fused_core), are compared with the oracle.

Per learn() call, fused path: the returns == values + ppo_np.gae bit for bit, the normalised
advantages within 2e-6 of the oracle's, the minibatch indices, the Adam step and the LR handed to
the update; last_losses within rtol 1e-5 + atol 1e-5.  Both paths: the LR after the call.  At the
end, parameters: the fused path within max(2e-5, 2 x the torch path's deviation); the torch path
within 2e-5 grown in proportion to steps x lr (4e-5 at 8 steps).  Adam m and v relative to their
largest entry: floors 1e-3 and 2e-3.

Rollout: the fused rollout's surface and reproducibility, the default rollout on torch's
generator, the cached log-probs against the oracle's recomputation, and a clip fraction of 0 in
the first minibatch of the learn() that follows.  Two ranks on one GPU against one process and the
oracle on the union batch."""
import functools
import multiprocessing as mp
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diamond
import gru_gauss_cases as C
import gru_gauss_oracle as GO
from oracle import ppo_np

import test_gpu_gru_gauss_act as ACT

SHAPE = (8, 20, 8, 3)
WIDE = (8, 9, 100, 6)
CASES = [(G, SHAPE) for G in C.WIDTHS] + [(32, WIDE)]
SEEDS = (3, 4)      # one rollout, one learn() each
KW = dict(num_epochs=2, num_minibatches=2, decay_lr=True)
MODES = ("fused", "torch", "torch-loss", "torch-core")


def _id(case):
    G, shape = case
    return str(G) if shape == SHAPE else f"{G}-" + "x".join(map(str, shape))


def _config(G, shape):
    return diamond.RecurrentContinuousPPOConfig(
        rollout_steps=shape[0], num_envs=shape[1], verbose=False, gru_hidden_dim=G,
        wide_observations=shape[2] > 32, total_steps=3 * shape[0] * shape[1], **KW)


def _envs(shape, **kw):
    import gym_stub
    T, Nn, D, A = shape
    return gym_stub.SyncVectorEnv(
        [lambda: gym_stub.SyntheticEnv(D, continuous=True, act_dim=A, **kw)] * Nn)


@functools.lru_cache(maxsize=None)
def _experience_np(G, shape, call):
    """The call's synthetic rollout on the CPU, drawn around the INITIAL parameters' means."""
    from dist_scripts.recurrent_gauss_dp import synth_experience
    init = C.initial_params(shape[2], shape[3], G, _config(G, shape).seed)
    return synth_experience(*shape, G, "cpu", init, seed=SEEDS[call])


def _perms(shape, call):
    rs = np.random.RandomState(5 + call)     # as np.random.seed(5 + call) before agent.learn
    return np.stack([rs.permutation(shape[0] * shape[1]) for _ in range(KW["num_epochs"])])


@functools.lru_cache(maxsize=None)
def _oracle(G, shape):
    """The oracle's learn() calls, computed once and shared by every path."""
    cfg = _config(G, shape)
    params = C.initial_params(shape[2], shape[3], G, cfg.seed)
    adam = ppo_np.new_adam_state(params, GO.PARAM_NAMES)
    lr, calls = cfg.lr, []
    for call in range(len(SEEDS)):
        x = GO.stack_experience(_experience_np(G, shape, call))
        out = GO.learn(params, adam, x, cfg, lr, _perms(shape, call))
        raw = ppo_np.gae(x["rewards"], x["terms"], x["truncs"], x["values"], x["next_values"],
                         cfg.gamma, cfg.gae_lambda)
        lr_used, lr = lr, GO.lr_after_learn(lr, call + 1, cfg)
        calls.append(dict(out, x=x, raw_adv=raw, lr_used=lr_used, lr_after=lr,
                          step_before=adam["step"] - len(out["losses"]),
                          params={n: v.copy() for n, v in params.items()},
                          m={n: v.copy() for n, v in adam["m"].items()},
                          v={n: v.copy() for n, v in adam["v"].items()}))
    return calls


@functools.lru_cache(maxsize=None)
def _run(G, shape, mode):
    T, Nn, D, A = shape
    agent = diamond.RecurrentContinuousPPO(None, _config(G, shape), envs=_envs(shape))
    assert agent.gru is not None and agent.gru.gauss
    fused = mode == "fused"
    agent.fused_gru = fused
    agent.fused_loss = mode == "torch-loss"
    agent.fused_core = mode == "torch-core"
    names = [n for n, _ in agent.network.named_parameters()]
    assert names == GO.PARAM_NAMES
    init = C.initial_params(D, A, G, agent.cfg.seed)
    for n, p in agent.network.named_parameters():
        assert np.array_equal(p.detach().cpu().numpy(), init[n]), n
    captured = []
    inner = agent._learn_fused

    def capture(observations, actions, log_probs, advantages, returns, prev_dones, hx, idx, step,
                lr, *rest):
        assert actions.dtype == torch.float32 and tuple(actions.shape) == (T * Nn, A)
        captured.append(dict(adv=advantages.cpu().numpy().copy(), ret=returns.cpu().numpy().copy(),
                             idx=idx.cpu().numpy().copy(), step=step, lr=lr))
        return inner(observations, actions, log_probs, advantages, returns, prev_dones, hx, idx,
                     step, lr, *rest)

    agent._learn_fused = capture
    for call, ref in enumerate(_oracle(G, shape)):
        exp = [[x.to(agent.device) if isinstance(x, torch.Tensor) else x for x in row]
               for row in _experience_np(G, shape, call)]
        np.random.seed(5 + call)
        agent.learn(exp)
        torch.cuda.synchronize()
        assert agent.optimizer.param_groups[0]["lr"] == ref["lr_after"]
        if not fused:
            assert not captured
            continue
        got = captured.pop()
        assert not captured
        x = ref["x"]
        assert np.array_equal(got["ret"], (x["values"] + ref["raw_adv"]).reshape(-1))
        d_adv = np.abs(got["adv"] - ref["adv"].reshape(-1)).max()
        print(f"G={G} {shape} call {call}: max|adv - oracle| {d_adv:.2e}")
        assert d_adv <= 2e-6
        assert np.array_equal(got["idx"], ref["idx"])
        assert got["step"] == ref["step_before"] and got["lr"] == ref["lr_used"]
        losses = agent.last_losses.cpu().numpy()
        assert losses.shape == ref["losses"].shape
        np.testing.assert_allclose(losses, ref["losses"], rtol=1e-5, atol=1e-5)
    steps = KW["num_epochs"] * KW["num_minibatches"] * len(SEEDS)
    if mode == "torch-loss":
        assert agent.loss_head_calls == steps
    else:
        assert agent.loss_head_calls == 0
    if mode == "torch-core":
        assert agent.core_scan_calls == steps
        np.testing.assert_allclose(agent.last_losses.cpu().numpy(), _oracle(G, shape)[-1]["losses"],
                                   rtol=1e-5, atol=1e-5)
    else:
        assert agent.core_scan_calls == 0
    ref = _oracle(G, shape)[-1]
    assert ref["lr_after"] < ref["lr_used"] < _config(G, shape).lr
    flat = lambda d: np.concatenate([d[n].ravel() for n in names])
    mine = lambda buf: np.concatenate([v.cpu().numpy().ravel() for v in agent.flat.views(buf)])
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    dev = dict(p=float(np.abs(mine(agent.flat.flat) - flat(ref["params"])).max()),
               m=rel(mine(agent.m), flat(ref["m"])), v=rel(mine(agent.v), flat(ref["v"])))
    moved = np.abs(flat(ref["params"]) - flat(init)).max()
    assert moved > 1e-4          # the update itself is far above every bound below
    assert np.abs(ref["params"]["actor_log_std"]).max() > 1e-4   # log_std moved too
    d_ls = np.abs(agent.network.actor_log_std.detach().cpu().numpy()
                  - ref["params"]["actor_log_std"]).max()
    print(f"G={G} {shape} {mode}: max|param - oracle| {dev['p']:.2e} (moved {moved:.1e}, log_std "
          f"{d_ls:.2e}), m {dev['m']:.2e}, v {dev['v']:.2e}")
    return dev, mine(agent.flat.flat), mine(agent.m)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gauss_recurrent_learn_matches_oracle(case, mode):
    G, shape = case
    torch_dev = _run(G, shape, "torch")[0]
    dev = _run(G, shape, mode)[0]
    if mode == "fused":
        bound = dict(p=max(2e-5, 2 * torch_dev["p"]), m=max(1e-3, 2 * torch_dev["m"]),
                     v=max(2e-3, 2 * torch_dev["v"]))
    else:
        steps = KW["num_epochs"] * KW["num_minibatches"] * len(SEEDS)
        bound = dict(p=2e-5 * max(1.0, steps * 3e-4 / (4 * 3e-4)), m=1e-3, v=2e-3)
    for k in ("p", "m", "v"):
        assert dev[k] <= bound[k], (k, dev[k], bound[k], torch_dev[k])


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_gauss_recurrent_learn_fused_matches_torch_path(case):
    _, p1, m1 = _run(*case, "fused")
    _, p2, m2 = _run(*case, "torch")
    assert np.abs(p1 - p2).max() <= 2e-5
    np.testing.assert_allclose(m1, m2, rtol=1e-3, atol=1e-7)


def test_unsupported_shape_and_custom_network_take_the_torch_path():
    class Mine(diamond.RecurrentContinuousActorCriticNetwork):
        pass

    shape = (4, 3, 40, 2)       # 40 observations without wide_observations
    cfg = diamond.RecurrentContinuousPPOConfig(rollout_steps=4, num_envs=3, verbose=False)
    assert diamond.RecurrentContinuousPPO(None, cfg, envs=_envs(shape)).gru is None
    agent = diamond.RecurrentContinuousPPO(None, cfg, network_cls=Mine, envs=_envs((4, 3, 8, 2)))
    assert agent.gru is None
    ACT_start(agent)
    agent.fused_rollout = True          # asked for, not served: the torch rollout runs
    p0 = agent.flat.flat.clone()
    agent.learn(agent.rollout())
    torch.cuda.synchronize()
    assert agent._act_counter == 0
    assert torch.isfinite(agent.flat.flat).all()
    assert float((agent.flat.flat - p0).abs().max()) > 1e-5


# ---- rollout
def ACT_start(agent, env_seed=7):
    """What train() sets up before its first rollout()."""
    cfg = agent.cfg
    agent.current_observations, _ = agent.envs.reset(seed=env_seed)
    agent.prev_dones = np.zeros(cfg.num_envs, dtype=bool)
    agent.current_hx = torch.zeros(1, cfg.num_envs, cfg.gru_hidden_dim, device=agent.device)


def _rollout_agent(shape, fused, G=16, **kw):
    T, Nn, D, A = shape
    np.random.seed(0)
    torch.manual_seed(0)
    cfg = diamond.RecurrentContinuousPPOConfig(rollout_steps=T, num_envs=Nn, verbose=False,
                                               gru_hidden_dim=G, **kw)
    # episodes end often enough for several hidden resets inside T steps
    agent = diamond.RecurrentContinuousPPO(None, cfg, envs=_envs(shape, p_term=0.1, p_trunc=0.05))
    assert agent.gru is not None
    with torch.no_grad():       # a log_std away from 0, so sigma shows in every log-prob
        agent.network.actor_log_std.copy_(torch.linspace(-1.0, 0.4, A).reshape(1, A))
    agent.fused_rollout = fused
    ACT_start(agent)
    return agent


@pytest.mark.parametrize("G", C.WIDTHS)
def test_fused_rollout_surface_and_first_minibatch_is_on_policy(G):
    shape = T, Nn, D, A = (16, 20, 7, 3)
    agent = _rollout_agent(shape, True, G, num_epochs=2)
    seen = []
    step = agent.envs.step
    agent.envs.step = lambda a: (seen.append(a), step(a))[1]
    exp = agent.rollout()
    torch.cuda.synchronize()
    dev = agent.device
    assert len(exp) == T and agent._act_counter == T
    assert all(a.dtype == np.float32 and a.shape == (Nn, A) for a in seen)
    f32 = torch.float32
    for t, row in enumerate(exp):
        assert len(row) == 10
        obs, act, rew, term, trunc, pd, lp, v, nv, hx = row
        for x, shp, dt in ((obs, (Nn, D), f32), (act, (Nn, A), f32), (pd, (Nn,), torch.bool),
                           (lp, (Nn,), f32), (v, (Nn,), f32), (nv, (Nn,), f32),
                           (hx, (1, Nn, G), f32)):
            assert isinstance(x, torch.Tensor) and tuple(x.shape) == shp and x.dtype == dt
            assert x.device.type == dev.type and x.device.index == dev.index
        for x in (rew, term, trunc):
            assert isinstance(x, np.ndarray) and x.shape == (Nn,)
        assert np.array_equal(seen[t], act.cpu().numpy())
        again = ACT.run_act(agent, obs.cpu().numpy(), pd.cpu().numpy(), hx[0].cpu().numpy(),
                            agent._act_seed, t)
        nxt = exp[t + 1][9] if t + 1 < T else agent.current_hx
        assert np.array_equal(again["hx_out"], nxt[0].cpu().numpy()), t
        assert np.array_equal(again["actions"], act.cpu().numpy()), t
        assert np.array_equal(again["log_probs"], lp.cpu().numpy()), t
        assert np.array_equal(again["values"], v.cpu().numpy()), t
    assert torch.all(exp[0][9] == 0)
    assert any(bool(row[5].any()) for row in exp[1:])       # resets happened
    # the cached log-probs and values against the oracle's recomputation of the sequence, beside
    # the torch path's float32 outputs: within 4x the torch path's own distance (floor 2e-5)
    x = GO.stack_experience(exp)
    params = {n: p.detach().cpu().numpy() for n, p in agent.network.named_parameters()}
    lp64 = GO.log_probs(params, x["obs"], x["actions"], x["prev_dones"], x["hx0"])
    _, v64 = GO.forward(params, x["obs"], x["prev_dones"], x["hx0"])
    with torch.no_grad():
        obs_t = torch.stack([r[0] for r in exp])
        mean, ls, v32, _ = agent.network.get_means_log_stds_values_and_hx(
            obs_t, exp[0][9], torch.stack([r[5] for r in exp]))
        lp32 = diamond.continuous_ppo.JointNormal(mean, ls.exp()).log_prob(
            torch.stack([r[1] for r in exp]))
    d_fused = max(np.abs(x["log_probs"] - lp64).max(), np.abs(x["values"] - v64).max())
    d_torch = max(np.abs(lp32.cpu().double().numpy() - lp64).max(),
                  np.abs(v32.cpu().double().numpy() - v64).max())
    print(f"G={G}: d_fused = {d_fused:.3e}  d_torch = {d_torch:.3e}")
    assert d_fused <= max(4 * d_torch, 2e-5), (d_fused, d_torch)
    # learn() at unchanged parameters recomputes a ratio of 1 to rounding: nothing is clipped in
    # the first minibatch, on either path
    ratio64 = np.exp(lp64 - x["log_probs"].astype(np.float64))
    assert np.abs(ratio64 - 1).max() <= 1e-4
    for fused_gru in (True, False):
        agent.fused_gru = fused_gru
        agent.fused_loss = not fused_gru        # the loss head reports the clip fraction
        state = agent.flat.flat.clone(), agent.m.clone(), agent.v.clone()
        seen_parts = []
        if fused_gru:
            # the kernel's policy sum over an unclipped minibatch is -sum(adv * ratio)
            np.random.seed(3)
            agent.learn(exp)
            torch.cuda.synchronize()
            first = agent.last_losses[0].cpu().numpy()
            ref = GO.learn({n: v.copy() for n, v in params.items()},
                           ppo_np.new_adam_state(params, GO.PARAM_NAMES), x, agent.cfg,
                           agent.cfg.lr, _np_perms(3, T * Nn, agent.cfg.num_epochs))
            np.testing.assert_allclose(first, ref["losses"][0], rtol=1e-5, atol=1e-5)
            adv = ref["adv"].reshape(-1)[ref["idx"][0, 0]]
            # every ratio is within max|ratio - 1| of 1, so the mean moves by at most that x mean|adv|
            np.testing.assert_allclose(first[1], -adv.mean(), rtol=0,
                                       atol=np.abs(adv).mean() * np.abs(ratio64 - 1).max() + 1e-6)
        else:
            import diamond.recurrent_ppo as RP
            inner = RP.fused_ppo_loss

            def spy(*a, **k):
                loss, parts = inner(*a, **k)
                seen_parts.append(parts.detach().clone())
                return loss, parts

            RP.fused_ppo_loss = spy
            try:
                np.random.seed(3)
                agent.learn(exp)
                torch.cuda.synchronize()
            finally:
                RP.fused_ppo_loss = inner
            assert float(seen_parts[0][4]) == 0.0, "clip fraction of the first minibatch"
        with torch.no_grad():       # back to the rollout's parameters for the other path
            agent.flat.flat.copy_(state[0])
            agent.m.copy_(state[1])
            agent.v.copy_(state[2])


def _np_perms(seed, B, epochs):
    rs = np.random.RandomState(seed)
    return np.stack([rs.permutation(B) for _ in range(epochs)])


def test_fused_rollout_is_reproducible_from_the_seed():
    shape = (8, 8, 4, 2)
    rows = []
    for _ in range(2):
        agent = _rollout_agent(shape, True)
        exp = agent.rollout() + agent.rollout()
        torch.cuda.synchronize()
        rows.append(([[x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
                       for x in row] for row in exp], agent.current_hx.cpu().numpy()))
    (e1, h1), (e2, h2) = rows
    assert np.array_equal(h1, h2)
    for r1, r2 in zip(e1, e2):
        for x, y in zip(r1, r2):
            assert np.array_equal(x, y)


def test_default_rollout_still_draws_from_torch():
    shape = T, Nn, D, A = (8, 8, 4, 2)
    assert diamond.RecurrentContinuousPPO.fused_rollout is False
    outs = []
    for s in (1234, 1234, 99):
        agent = _rollout_agent(shape, False)
        torch.manual_seed(s)
        exp = agent.rollout()
        assert agent._act_counter == 0
        outs.append(torch.stack([r[1] for r in exp]).cpu().numpy())
        assert outs[-1].dtype == np.float32 and outs[-1].shape == (T, Nn, A)
        # the log-prob of row 0 is JointNormal's on the network's own outputs
        with torch.no_grad():
            mean, ls, v, _ = agent.network.get_means_log_stds_values_and_hx(
                exp[0][0][None], exp[0][9], exp[0][5][None])
            lp = diamond.continuous_ppo.JointNormal(mean[0], ls[0].exp()).log_prob(exp[0][1])
        assert torch.equal(lp, exp[0][6]) and torch.equal(v[0], exp[0][7])
    assert np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2])


# ---- two ranks on one GPU
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(300)
def test_gauss_two_ranks_match_one_and_the_oracle(tmp_path):
    from dist_scripts import recurrent_gauss_dp as DP
    G, (T, Ng, D, A) = 16, (6, 2 * 17, 5, 3)
    ctx = mp.get_context("spawn")
    outs = {}
    for world in (1, 2):
        port = _free_port()
        procs = []
        for r in range(world):
            path = str(tmp_path / f"w{world}_r{r}.npz")
            outs[(world, r)] = path
            procs.append(ctx.Process(target=DP.run, args=(r, world, port, T, Ng, D, A, path, G)))
        for p in procs:
            p.start()
        for p in procs:
            p.join(120)     # each child under its own time limit
        alive = [p for p in procs if p.is_alive()]
        for p in alive:
            p.kill()
        assert not alive and all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    one = np.load(outs[(1, 0)])
    r0, r1 = np.load(outs[(2, 0)]), np.load(outs[(2, 1)])
    assert np.array_equal(r0["init"], one["init"]) and np.array_equal(r1["init"], one["init"])
    assert np.array_equal(r0["final"], r1["final"])      # replicated clip + Adam on one gradient
    assert np.array_equal(r0["grad"], r1["grad"])
    assert np.all(np.isfinite(r0["final"]))
    assert np.abs(one["final"] - one["init"]).max() > 1e-4
    np.testing.assert_allclose(r0["final"], one["final"], rtol=0, atol=2e-5)
    # the oracle on the union batch: num_minibatches = 1, so every epoch's minibatch is the whole
    # batch whatever the permutation
    cfg = diamond.RecurrentContinuousPPOConfig(rollout_steps=T, num_envs=Ng, num_epochs=3,
                                               num_minibatches=1, gru_hidden_dim=G)
    init = C.initial_params(D, A, G, cfg.seed)
    x = GO.stack_experience(DP.synth_experience(T, Ng, D, A, G, "cpu", init))
    params = {n: v.copy() for n, v in init.items()}
    GO.learn(params, ppo_np.new_adam_state(params, GO.PARAM_NAMES), x, cfg, cfg.lr,
             _np_perms(0, T * Ng, cfg.num_epochs))
    ls_oracle = params["actor_log_std"].reshape(-1)
    assert np.abs(ls_oracle).max() > 1e-4
    for got in (r0["final"], one["final"]):
        assert np.abs(got[:A] - ls_oracle).max() <= 2e-5
    # the hand-made gradient at the final parameters, the two ranks' slabs all-reduced: the union
    # minibatch's, with the entropy bonus's -entropy_beta per log_std dimension once
    adv, ret, dlp = DP.probe_batch(T, Ng, A)
    flat = r0["final"]
    off, final = 0, {}
    for n in GO.PARAM_NAMES:
        final[n] = flat[off:off + init[n].size].reshape(init[n].shape)
        off = (off + init[n].size + 15) // 16 * 16
    sums, ref = GO.minibatch_grads(final, x["obs"], x["actions"], x["log_probs"] + dlp, adv, ret,
                                   x["prev_dones"], x["hx0"], np.arange(T * Ng), T * Ng,
                                   cfg.ppo_clip, cfg.value_loss_weight, cfg.entropy_beta)
    scale = max(np.abs(g).max() for g in ref.values())
    for g in (r0["grad"], one["grad"]):
        d = np.abs(g[:A] - ref["actor_log_std"].reshape(-1)).max()
        print(f"log_std gradient: max|diff| / max|g| = {d / scale:.2e}; "
              f"entropy term {cfg.entropy_beta} against {np.abs(ref['actor_log_std']).max():.3f}")
        assert d <= 2e-5 * scale
        np.testing.assert_allclose(g[off:off + 3], sums, rtol=1e-5, atol=1e-5 * T * Ng)
    # a doubled or missing entropy term would be 0.01 off: far outside the bound
    assert cfg.entropy_beta > 100 * 2e-5 * scale
