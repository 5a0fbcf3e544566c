#!/usr/bin/env python3
"""Time rollout() of a wide-class agent with the fused sampler (fused_actions_wide) against the
default torch sampling path.

    python tools/bench_wide_rollout.py --out profiles/wide_rollout.json

Stub env (tests/golden/gym_stub.py: NumPy draws, no simulation, so the host side of a step is as
cheap as an env gets), T = 32, N in {32, 1024, 8192}, three shapes: LunarLander-128 (D 8, 4 discrete
actions, hidden 128), Ant-64 (D 105, 8 Gaussian actions, hidden 64) and Humanoid-64 (D 376, 17
Gaussian actions, hidden 64: the large heads).  `--only NAME` runs one shape.  Per shape and N two
agents with the same weights, the flag on and off, run their rollouts alternately (whatever else
loads the host hits both alike): `--warmup` untimed rollouts each, then `--rollouts` timed ones,
every one bracketed by a device synchronisation and the host wall clock.  Reported: the median ms
per rollout() of each path with min / max, torch / fused, and the part of a rollout spent inside
the sampling call itself (network.get_actions or NativeLearner.act, both of which return host
arrays and so include their own synchronisation).

The flag is read with getattr: on a tree without it both agents take the torch path (the record
says so in "flag_available"), which is how the parent commit's numbers are taken.
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

T = 32
SIZES = [32, 1024, 8192]
# (name, hidden, D, A, Gaussian head)
SHAPES = [("LunarLander-128", 128, 8, 4, False), ("Ant-64", 64, 105, 8, True),
          ("Humanoid-64", 64, 376, 17, True)]


class SampleClock:
    """Seconds spent inside the agent's sampling call (whichever path rollout() takes)."""

    def __init__(self, agent):
        self.s = 0.0
        for obj, name in ((agent.network, "get_actions"), (agent._learner, "act")):
            setattr(obj, name, self._timed(getattr(obj, name)))

    def _timed(self, fn):
        def call(*a, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                self.s += time.perf_counter() - t0
        return call


def make_agent(Hd, D, A, cont, Nn, fused):
    np.random.seed(0)
    torch.manual_seed(0)
    env = (lambda: gym_stub.SyntheticEnv(D, continuous=True, act_dim=A)) if cont else \
          (lambda: gym_stub.SyntheticEnv(D, A))
    envs = gym_stub.SyncVectorEnv([env] * Nn)
    Cfg = diamond.ContinuousPPOConfig if cont else diamond.PPOConfig
    Agent = diamond.ContinuousPPO if cont else diamond.PPO
    cfg = Cfg(network_hidden_dim=Hd, rollout_steps=T, num_envs=Nn, verbose=False)
    agent = Agent(None, cfg, envs=envs)
    assert agent._learner.shape_class == "wide"
    available = getattr(type(agent), "fused_actions_wide", None) is not None
    if available:
        agent.fused_actions_wide = fused
    agent.current_observations, _ = agent.envs.reset(seed=1)
    return agent, available


def timed_rollout(agent, clock):
    torch.cuda.synchronize()
    clock.s = 0.0
    t0 = time.perf_counter()
    agent.rollout()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, clock.s * 1e3


def run(name, Hd, D, A, cont, Nn, warmup, rollouts):
    agents, available = {}, True
    for k, fused in (("fused", True), ("torch", False)):
        agents[k], available = make_agent(Hd, D, A, cont, Nn, fused)
    clocks = {k: SampleClock(a) for k, a in agents.items()}
    ms = {k: [] for k in agents}
    sample = {k: [] for k in agents}
    for r in range(warmup + rollouts):
        for k, agent in agents.items():
            t, s = timed_rollout(agent, clocks[k])
            if r >= warmup:
                ms[k].append(t)
                sample[k].append(s)
    out = {"shape": name, "hidden": Hd, "D": D, "A": A, "continuous": cont, "N": Nn, "T": T,
           "warmup": warmup, "rollouts": rollouts, "flag_available": available}
    for k, v in ms.items():
        out[k + "_ms_median"] = statistics.median(v)
        out[k + "_ms_min"], out[k + "_ms_max"] = min(v), max(v)
        out[k + "_sample_ms_median"] = statistics.median(sample[k])
    out["torch_over_fused"] = out["torch_ms_median"] / out["fused_ms_median"]
    out["fused_is_slower"] = out["torch_over_fused"] < 1.0
    out["torch_sample_share"] = out["torch_sample_ms_median"] / out["torch_ms_median"]
    for a in agents.values():
        a.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rollouts", type=int, default=20)
    ap.add_argument("--only", default=None, help="run one shape")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "env": "tests/golden/gym_stub.py", "runs": []}
    for name, Hd, D, A, cont in SHAPES:
        if a.only and name != a.only:
            continue
        for Nn in SIZES:
            r = run(name, Hd, D, A, cont, Nn, a.warmup, a.rollouts)
            print(json.dumps(r), flush=True)
            res["runs"].append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
