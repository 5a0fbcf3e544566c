#!/usr/bin/env python3
"""Time RecurrentPPO.rollout() with the fused step kernels against the torch path.

    python tools/bench_recurrent_rollout.py --out profiles/recurrent_rollout.json

Stub env (tests/golden/gym_stub.py: NumPy draws, no simulation, so the host side of a step is as
cheap as an env gets), T = 32, N in {32, 1024, 8192}, D = 8, A = 4.  Per N two agents with the
same weights, `fused_rollout` on and off, run their rollouts alternately (whatever else loads the
host hits both alike): `--warmup` untimed rollouts each, then `--rollouts` timed ones, every one
bracketed by a device synchronisation and the host wall clock (a rollout is 2-100 ms).  Reported:
the median ms per rollout() of each path with min / max, and torch / fused.
`--gru-hidden G [G ...]` (default 16) runs other GRU widths, one after the other; 32 and 64 use
csrc/gruact.hip's kernels at G = 32 / 64, and a result row of a width other than 16 carries "G":

    python tools/bench_recurrent_rollout.py --gru-hidden 32 64 \
        --out profiles/recurrent_wide_rollout.json

In a separate pass (events on every launch slow the host) the library's timing mode
(dppo_gru_set_timing) gives the two kernels' own execution time per launch.

`--obs-dim D --act-dim A --sizes N [N ...]` set the shape.  Past 32 observations the fused
kernels are asked for with `--wide-observations` (RecurrentPPOConfig.wide_observations); the
yardstick is the same shape without the flag, the torch rollout it always ran, without and with
`fused_core` (`torch_core`), and each row says whether the fused path's slowest rollout is below
the other's fastest:

    python tools/bench_recurrent_rollout.py --gru-hidden 16 32 64 --obs-dim 128 --act-dim 6 \
        --wide-observations --sizes 32 8192 --out bench_out/recurrent_wide_obs_rollout.json

`--continuous` times RecurrentContinuousPPO (the Gaussian head; `--act-dim` = action dimensions):
`fused` (dppo_gru_gauss_act_f32 + dppo_gru_value_f32), `torch` and `torch_core` alternate.
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


def make_agent(Nn, fused, G=16, D=D, A=A, wide_obs=False, core=False, continuous=False):
    """fused: the step kernels (with wide_obs: asked for through the config flag).  Not fused:
    the torch rollout; where wide_obs is tested the flag stays off, so no fused path exists."""
    np.random.seed(0)
    torch.manual_seed(0)
    if continuous:
        envs = gym_stub.SyncVectorEnv(
            [lambda: gym_stub.SyntheticEnv(D, continuous=True, act_dim=A)] * Nn)
        cfg = diamond.RecurrentContinuousPPOConfig(rollout_steps=T, num_envs=Nn, verbose=False,
                                                   gru_hidden_dim=G, wide_observations=wide_obs)
        agent = diamond.RecurrentContinuousPPO(None, cfg, envs=envs)
        assert agent.gru is not None
    else:
        envs = gym_stub.SyncVectorEnv([lambda: gym_stub.SyntheticEnv(D, A)] * Nn)
        cfg = diamond.RecurrentPPOConfig(rollout_steps=T, num_envs=Nn, verbose=False,
                                         gru_hidden_dim=G, wide_observations=wide_obs and fused)
        agent = diamond.RecurrentPPO(None, cfg, envs=envs)
        assert (agent.gru is not None) == (fused or not wide_obs)
    agent.fused_rollout = fused
    agent.fused_core = core
    agent.current_observations, _ = agent.envs.reset(seed=1)
    agent.prev_dones = np.zeros(Nn, dtype=bool)
    agent.current_hx = torch.zeros(1, Nn, cfg.gru_hidden_dim, device=agent.device)
    return agent


def timed_rollout(agent):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    agent.rollout()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def run(Nn, warmup, rollouts, kernel_rollouts, G=16, D=D, A=A, wide_obs=False, continuous=False):
    agents = {"fused": make_agent(Nn, True, G, D, A, wide_obs, continuous=continuous),
              "torch": make_agent(Nn, False, G, D, A, wide_obs, continuous=continuous)}
    three = wide_obs or continuous
    if three:
        agents["torch_core"] = make_agent(Nn, False, G, D, A, wide_obs, core=True,
                                          continuous=continuous)
    ms = {k: [] for k in agents}
    for r in range(warmup + rollouts):
        for k, agent in agents.items():
            t = timed_rollout(agent)
            if r >= warmup:
                ms[k].append(t)
    out = {"N": Nn, "T": T, "D": D, "A": A, "warmup": warmup, "rollouts": rollouts}
    if G != 16:
        out = {"G": G, **out}
    for k, v in ms.items():
        out[k + "_ms_median"] = statistics.median(v)
        out[k + "_ms_min"], out[k + "_ms_max"] = min(v), max(v)
    out["torch_over_fused"] = out["torch_ms_median"] / out["fused_ms_median"]
    out["fused_is_slower"] = out["torch_over_fused"] < 1.0
    if continuous:
        out["continuous"] = True
    if wide_obs:
        out["wide_observations"] = True
    if three:
        out["torch_core_over_fused"] = out["torch_core_ms_median"] / out["fused_ms_median"]
        for k in ("torch", "torch_core"):
            out[f"fused_max_below_{k}_min"] = out["fused_ms_max"] < out[k + "_ms_min"]
    gru = agents["fused"].gru
    gru.set_timing(True)
    for _ in range(kernel_rollouts):
        agents["fused"].rollout()
    kt = gru.timing()
    gru.set_timing(False)
    for k, (total, launches) in kt.items():
        out[f"{k}_kernel_us_per_launch"] = 1e3 * total / max(launches, 1)
        out[f"{k}_kernel_launches"] = launches
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rollouts", type=int, default=20)
    ap.add_argument("--kernel-rollouts", type=int, default=5)
    ap.add_argument("--gru-hidden", type=int, nargs="+", default=[16])
    ap.add_argument("--sizes", type=int, nargs="+", default=SIZES)
    ap.add_argument("--obs-dim", type=int, default=D)
    ap.add_argument("--act-dim", type=int, default=A)
    ap.add_argument("--wide-observations", action="store_true")
    ap.add_argument("--continuous", action="store_true")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "env": "tests/golden/gym_stub.py", "sizes": []}
    for G in a.gru_hidden:
        for Nn in a.sizes:
            r = run(Nn, a.warmup, a.rollouts, a.kernel_rollouts, G, a.obs_dim, a.act_dim,
                    a.wide_observations, a.continuous)
            print(json.dumps(r), flush=True)
            res["sizes"].append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
