#!/usr/bin/env python3
"""Time RecurrentPPO.learn() with the fused minibatch kernel against the torch-autograd path.

    python tools/bench_recurrent_learn.py --out profiles/recurrent_wide_learn.json

Stub env (tests/golden/gym_stub.py), T = 32, D = 8, A = 4, the default 10 epochs x 1 minibatch;
gru_hidden_dim G in {16, 32, 64} (`--gru-hidden`), N in {32, 1024, 8192} (`--sizes`).  Per (G, N)
two agents with the same weights, `fused_gru` on and off, learn the same synthetic rollout
alternately (whatever else loads the host hits both alike): `--warmup` untimed learns each, then
`--learns` timed ones, every one bracketed by a device synchronisation and the host wall clock.
Reported: the median ms per learn() of each path with min / max, torch / fused, and whether the
two medians lie inside each other's min-max spread (then neither path is ahead).

All three widths run gru_grad_kernel<G> (csrc/grugrad.hip).  With `fused_gru` off an agent runs exactly what it ran before the fused
kernel existed for its G.

`--obs-dim D --act-dim A` set the observation width and the action count.  Past 32 observations
the fused kernels are asked for with `--wide-observations` (RecurrentPPOConfig.wide_observations),
and the yardstick is the same shape without the flag, which runs what it always ran, the torch
loop: three agents then alternate, `fused` (flag on), `torch` (flag off) and `torch_core` (flag
off, `fused_core` on: GRUCore on the scan kernels), and each row says whether the fused path's
slowest learn is below the other's fastest:

    python tools/bench_recurrent_learn.py --obs-dim 128 --act-dim 6 --wide-observations \
        --sizes 32 8192 --out bench_out/recurrent_wide_obs_learn.json

`--continuous` times RecurrentContinuousPPO (the Gaussian head; `--act-dim` = action dimensions)
the same way: `fused` (gru_grad_kernel<G, WIDE_OBS, true>), `torch` (fused_gru off) and
`torch_core` (that with `fused_core`) share the weights and alternate; the rollout's actions are
drawn from the agent's own policy and carry its log-probs:

    python tools/bench_recurrent_learn.py --continuous --obs-dim 17 --act-dim 6 \
        --sizes 32 8192 --out profiles/recurrent_gauss_learn.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "diamond-ppo_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import diamond
import gym_stub

T, D, A = 32, 8, 4      # D, A: the defaults of --obs-dim / --act-dim
SIZES = [32, 1024, 8192]
WIDTHS = [16, 32, 64]


def make_agent(Nn, G, fused, D=D, A=A, wide_obs=False, core=False, continuous=False):
    """fused: the minibatch kernel (with wide_obs: asked for through the config flag).  Not fused:
    the torch loop, by fused_gru = False or, where wide_obs is tested, by leaving the flag off."""
    np.random.seed(0)
    torch.manual_seed(0)
    if continuous:
        envs = gym_stub.SyncVectorEnv(
            [lambda: gym_stub.SyntheticEnv(D, continuous=True, act_dim=A)] * Nn)
        cfg = diamond.RecurrentContinuousPPOConfig(rollout_steps=T, num_envs=Nn, verbose=False,
                                                   gru_hidden_dim=G, wide_observations=wide_obs)
        agent = diamond.RecurrentContinuousPPO(None, cfg, envs=envs)
        assert agent.gru is not None
        agent.fused_gru = fused
        agent.fused_core = core
        return agent
    envs = gym_stub.SyncVectorEnv([lambda: gym_stub.SyntheticEnv(D, A)] * Nn)
    cfg = diamond.RecurrentPPOConfig(rollout_steps=T, num_envs=Nn, verbose=False,
                                     gru_hidden_dim=G, wide_observations=wide_obs and fused)
    agent = diamond.RecurrentPPO(None, cfg, envs=envs)
    assert (agent.gru is not None) == (fused or not wide_obs)
    agent.fused_gru = fused
    agent.fused_core = core
    return agent


def experience(Nn, G, device, seed=0, D=D, A=A):
    """One rollout in RecurrentPPO.rollout()'s layout, random contents."""
    rng = np.random.default_rng(seed)
    g = lambda x, dt=torch.float32: torch.as_tensor(x, dtype=dt, device=device)
    hx = g(rng.standard_normal((1, Nn, G)) * 0.5)
    return [[g(rng.standard_normal((Nn, D))), g(rng.integers(0, A, Nn), torch.int64),
             rng.normal(1.0, 1.0, Nn), rng.random(Nn) < 0.05, rng.random(Nn) < 0.02,
             g(rng.random(Nn) < 0.1, torch.bool), g(-rng.uniform(0.3, 1.0, Nn)),
             g(rng.standard_normal(Nn)), g(rng.standard_normal(Nn)), hx] for _ in range(T)]


def gaussian_experience(agent, exp):
    """`exp` with float32 actions [N, A] drawn from the agent's own policy and their log-probs."""
    from diamond.continuous_ppo import JointNormal
    with torch.no_grad():
        mean, ls, _, _ = agent.network.get_means_log_stds_values_and_hx(
            torch.stack([r[0] for r in exp]), exp[0][9], torch.stack([r[5] for r in exp]))
        dist = JointNormal(mean, ls.exp())
        act = dist.sample()
        lp = dist.log_prob(act)
    return [[r[0], act[t], *r[2:6], lp[t], *r[7:]] for t, r in enumerate(exp)]


def timed_learn(agent, exp):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    agent.learn(exp)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def run(Nn, G, warmup, learns, D=D, A=A, wide_obs=False, continuous=False):
    agents = {"fused": make_agent(Nn, G, True, D, A, wide_obs, continuous=continuous),
              "torch": make_agent(Nn, G, False, D, A, wide_obs, continuous=continuous)}
    three = wide_obs or continuous
    if three:
        agents["torch_core"] = make_agent(Nn, G, False, D, A, wide_obs, core=True,
                                          continuous=continuous)
    exp = experience(Nn, G, agents["fused"].device, D=D, A=A)
    if continuous:
        exp = gaussian_experience(agents["fused"], exp)
    ms = {k: [] for k in agents}
    for r in range(warmup + learns):
        for k, agent in agents.items():
            t = timed_learn(agent, exp)
            if r >= warmup:
                ms[k].append(t)
    cfg = agents["fused"].cfg
    out = {"G": G, "N": Nn, "T": T, "D": D, "A": A, "epochs": cfg.num_epochs,
           "minibatches": cfg.num_minibatches, "warmup": warmup, "learns": learns}
    for k, v in ms.items():
        out[k + "_ms_median"] = statistics.median(v)
        out[k + "_ms_min"], out[k + "_ms_max"] = min(v), max(v)
    out["torch_over_fused"] = out["torch_ms_median"] / out["fused_ms_median"]
    out["fused_is_slower"] = out["torch_over_fused"] < 1.0
    inside = lambda a, b: out[b + "_ms_min"] <= out[a + "_ms_median"] <= out[b + "_ms_max"]
    out["medians_inside_each_others_spread"] = inside("fused", "torch") and inside("torch", "fused")
    if continuous:
        out["continuous"] = True
    if wide_obs:
        out["wide_observations"] = True
    if three:
        out["torch_core_over_fused"] = out["torch_core_ms_median"] / out["fused_ms_median"]
        for k in ("torch", "torch_core"):
            out[f"fused_max_below_{k}_min"] = out["fused_ms_max"] < out[k + "_ms_min"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--learns", type=int, default=20)
    ap.add_argument("--gru-hidden", type=int, nargs="+", default=WIDTHS)
    ap.add_argument("--sizes", type=int, nargs="+", default=SIZES)
    ap.add_argument("--obs-dim", type=int, default=D)
    ap.add_argument("--act-dim", type=int, default=A)
    ap.add_argument("--wide-observations", action="store_true")
    ap.add_argument("--continuous", action="store_true")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "env": "tests/golden/gym_stub.py", "rows": []}
    for G in a.gru_hidden:
        for Nn in a.sizes:
            r = run(Nn, G, a.warmup, a.learns, a.obs_dim, a.act_dim, a.wide_observations,
                    a.continuous)
            print(json.dumps(r), flush=True)
            res["rows"].append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
