#!/usr/bin/env python3
"""Time learn_device() on a resident rollout at shapes outside the tuned class.

    python tools/bench_wide.py --out profiles/wide_learn.json
    python tools/bench_wide.py --only Humanoid-348 --only Humanoid-376 --compare-generic \
        --out profiles/wide_learn_large.json

At a commit with the wide kernel family (csrc/mbwide.hip) these shapes run the fused HIP learn; at
an earlier commit -- or with DPPO_WIDE=0 -- they take the generic path (network under torch
autograd, GAE / normalisation / clip + Adam in HIP).  The script is self-contained so the same
file runs against either tree: it reports which path ran.

Per shape: `--warmup` untimed learns, then `--learns` timed ones, each bracketed by a device
synchronisation and host wall clock (a learn is 10-1000 ms, far above timer resolution); the median
is reported with min and max.  With the fused path it also reads the library's per-kernel-class
timing for one learn and derives the minibatch kernel's time per launch and its fraction of the
157.3 TF fp32 MFMA peak in SURVEY §8(d)'s unit: 2 (3F - D H) FLOP per sample,
F = D H + 3 H^2 + H (A + 1).

`--compare-generic` adds, per shape, the generic path as a child process with DPPO_WIDE=0 runs it
(the same script and tree, `--fused-loss` off and on), and whether the fused learn's slowest run is
below the generic path's fastest.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "diamond-ppo_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import diamond
from gpu_helpers import SpecEnvs, synth

SHAPES = [
    ("LunarLander-128", 128, 8192, 8, 4, False, 128),
    ("HalfCheetah-128", 128, 4096, 17, 6, True, 128),
    ("Ant-64", 128, 4096, 105, 8, True, 64),
    # the large heads (hidden 64, obs_dim <= 384, act_dim <= 32): Humanoid / HumanoidStandup
    ("Humanoid-348", 128, 4096, 348, 17, True, 64),
    ("Humanoid-376", 128, 4096, 376, 17, True, 64),
]
PEAK_TF = 157.3


def flop_per_sample(D, A, H):
    F = D * H + 3 * H * H + H * (A + 1)
    return 2 * (3 * F - D * H)


def kernel_times(agent, ro):
    """{class: [total ms, launches]} of one learn from the library's own event timing."""
    h = agent._learner.handle
    try:
        h.set_timing(True)
        agent.learn_device(ro)
        torch.cuda.synchronize()
        t = h.timing()
        h.set_timing(False)
        return {k: list(v) for k, v in t.items() if v[1]}
    except Exception as e:  # an older tree without the accessor: the wall clock still stands
        return {"error": repr(e)}


def run(label, T, Nn, D, A, cont, H, warmup, learns, fused_loss=False):
    Cfg = diamond.ContinuousPPOConfig if cont else diamond.PPOConfig
    Agent = diamond.ContinuousPPO if cont else diamond.PPO
    cfg = Cfg(network_hidden_dim=H, rollout_steps=T, num_envs=Nn, verbose=False)
    torch.manual_seed(0)
    np.random.seed(0)
    agent = Agent(None, cfg, envs=SpecEnvs(D, A, cont))
    agent.fused_loss = fused_loss   # the generic path's loss head in HIP; the fused path has none
    L = agent._learner
    ro, _ = synth(T, Nn, D, A, cont, seed=1)
    for _ in range(warmup):
        agent.learn_device(ro)
    torch.cuda.synchronize()
    ms = []
    for _ in range(learns):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        agent.learn_device(ro)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    med = statistics.median(ms)
    out = {"label": label, "T": T, "N": Nn, "D": D, "A": A, "continuous": cont, "H": H,
           "fused": bool(L.fused), "shape_class": getattr(L, "shape_class", None),
           "fused_loss": bool(fused_loss),
           "epochs": cfg.num_epochs, "minibatches": cfg.num_minibatches,
           "learns": learns, "warmup": warmup,
           "ms_median": med, "ms_min": min(ms), "ms_max": max(ms),
           "env_steps_per_s": T * Nn / (med * 1e-3)}
    if L.fused:
        kt = kernel_times(agent, ro)
        out["kernel_ms"] = kt
        grad = kt.get("grad")
        if grad:
            per = grad[0] / grad[1]
            mb = T * Nn // cfg.num_minibatches
            out["mb_kernel_ms_per_launch"] = per
            out["mb_kernel_fraction_of_fp32_mfma_peak"] = (
                flop_per_sample(D, A, H) * mb / (per * 1e-3) / (PEAK_TF * 1e12))
    agent.close()
    return out


def generic_child(label, warmup, learns, fused_loss):
    """The shape's row from a fresh process with DPPO_WIDE=0: the generic path, unchanged code"""
    cmd = [sys.executable, os.path.abspath(__file__), "--only", label, "--warmup", str(warmup),
           "--learns", str(learns)] + (["--fused-loss"] if fused_loss else [])
    r = subprocess.run(cmd, env=dict(os.environ, DPPO_WIDE="0"), capture_output=True, text=True,
                       timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"generic child failed ({r.returncode}):\n{r.stdout}\n{r.stderr}")
    row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert not row["fused"] and row["fused_loss"] == fused_loss, row
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--learns", type=int, default=20)
    ap.add_argument("--only", action="append", default=None, help="run this label (repeatable)")
    ap.add_argument("--fused-loss", action="store_true",
                    help="set the agents' fused_loss (it matters on the generic path only)")
    ap.add_argument("--compare-generic", action="store_true",
                    help="also time each shape's generic path in DPPO_WIDE=0 child processes")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "dppo_wide": os.environ.get("DPPO_WIDE"),
           "shapes": []}
    for s in SHAPES:
        if a.only and s[0] not in a.only:
            continue
        r = run(*s, a.warmup, a.learns, a.fused_loss)
        if a.compare_generic:
            r["generic"] = generic_child(s[0], a.warmup, a.learns, False)
            r["generic_fused_loss"] = generic_child(s[0], a.warmup, a.learns, True)
            fastest = min(r["generic"]["ms_min"], r["generic_fused_loss"]["ms_min"])
            r["fused_max_below_generic_min"] = bool(r["fused"] and r["ms_max"] < fastest)
            r["generic_median_over_fused_median"] = \
                min(r["generic"]["ms_median"], r["generic_fused_loss"]["ms_median"]) / r["ms_median"]
        print(json.dumps(r), flush=True)
        res["shapes"].append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
