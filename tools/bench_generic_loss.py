#!/usr/bin/env python3
"""Time learn_device() on the generic path with the loss head as torch ops (fused_loss = False)
and as the HIP kernels of csrc/losshead.hip (fused_loss = True).

    python tools/bench_generic_loss.py --out profiles/generic_loss_head.json

Conventions of tools/bench_wide.py: spaces-only envs, a resident synthetic rollout of T = 128,
`--warmup` untimed learns, then `--learns` timed ones, each bracketed by a device synchronisation
and the host wall clock; median with min and max.  Per shape two agents with equal initial weights
(same seeds) run in ONE process and alternate learn by learn, so both see the same machine state;
a difference counts only where the two min-max ranges do not overlap.

Every shape takes the generic path: a subclass of the default discrete network (the plug-in
interface), the default network at a hidden width outside the fused classes, and a
Humanoid-sized Gaussian policy (348 inputs, 17 actions) -- a subclass as well, since the default
network at that shape runs the wide family's fused learn.

Also recorded, with device events over back-to-back calls on minibatch-sized inputs: the stream
time per dppo_ppo_loss_f32 call (its two launches) and per dppo_policy_logp_f32 launch over the
whole batch -- an upper bound on the kernels' own time, since calls this short are paced by the
host's enqueue -- and the loss head's forward + backward through torch ops and through the
autograd.Function.  `--kernels-only` runs just that part, for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats -d OUT -- python tools/bench_generic_loss.py --kernels-only
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "diamond-ppo_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import diamond
from diamond import engine
from gpu_helpers import SpecEnvs, synth

T = 128
# label, N, D, A, continuous, hidden, subclass the default network
SHAPES = [
    ("custom-net D8 A4 H64 N8192", 8192, 8, 4, False, 64, True),
    ("default-net H256 D8 A4 N8192", 8192, 8, 4, False, 256, False),
    ("Humanoid-shaped D348 A17 H64 N4096", 4096, 348, 17, True, 64, True),
]


def make_agent(Nn, D, A, cont, H, custom, fused_loss):
    Cfg = diamond.ContinuousPPOConfig if cont else diamond.PPOConfig
    Agent = diamond.ContinuousPPO if cont else diamond.PPO
    cfg = Cfg(network_hidden_dim=H, rollout_steps=T, num_envs=Nn, verbose=False)
    torch.manual_seed(0)
    np.random.seed(0)
    kw = {}
    if custom:
        base = diamond.continuous_ppo.ContinuousActorCriticNetwork if cont else \
            diamond.ppo.ActorCriticNetwork
        kw["network_cls"] = type("CustomNet", (base,), {})
    agent = Agent(None, cfg, envs=SpecEnvs(D, A, cont), **kw)
    assert not agent._learner.fused, "this shape must take the generic path"
    agent.fused_loss = fused_loss
    return agent


def timed(agent, ro):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    agent.learn_device(ro)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def kernel_events(m, B, A, cont, reps=200):
    """Device-event time per call of the loss head on a minibatch of m (ms), and of the
    forward-only kernel over B samples."""
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    rn = lambda *s: torch.randn(*s, device=dev, generator=g)
    logits_b = rn(B, A)
    acts = rn(B, A) if cont else torch.randint(0, A, (B,), device=dev, generator=g,
                                               dtype=torch.int32)
    ls_row = torch.full((1, A), -0.5, device=dev)
    idx = torch.randperm(B, device=dev, generator=g)[:m]
    logits = logits_b[idx].contiguous()
    ls = torch.broadcast_to(ls_row, logits.shape) if cont else None
    old = engine.policy_log_probs(logits_b, torch.broadcast_to(ls_row, logits_b.shape) if cont
                                  else None, actions=acts, continuous=cont)
    adv, ret, vals = rn(B), rn(B), rn(m)
    kw = dict(actions=acts, old_log_probs=old, advantages=adv, returns=ret, idx=idx, clip=0.2,
              value_loss_weight=1.0, entropy_beta=0.01, scale=1.0, continuous=cont)

    def per_call(fn):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    with torch.no_grad():
        loss_ms = per_call(lambda: engine.fused_ppo_loss(logits, vals, ls, **kw))
        logp_ms = per_call(lambda: engine.policy_log_probs(
            logits_b, torch.broadcast_to(ls_row, logits_b.shape) if cont else None, actions=acts,
            continuous=cont))
    # the same through today's torch ops, forward and backward, for scale
    lg = logits.clone().requires_grad_(True)
    vv = vals.clone().requires_grad_(True)
    lsp = ls_row.clone().requires_grad_(True) if cont else None

    def torch_fb():
        loss, _ = engine._torch_ppo_loss(lg, vv, torch.broadcast_to(lsp, lg.shape) if cont
                                         else None, acts, old, adv, ret, idx, 0.2, 1.0, 0.01,
                                         1.0, cont)
        loss.backward()

    def fused_fb():
        loss, _ = engine.fused_ppo_loss(lg, vv, torch.broadcast_to(lsp, lg.shape) if cont
                                        else None, **kw)
        loss.backward()

    return {"m": m, "B": B, "reps": reps,
            "ppo_loss_call_ms": loss_ms, "policy_logp_call_ms": logp_ms,
            "loss_fwd_bwd_torch_ms": per_call(torch_fb),
            "loss_fwd_bwd_fused_ms": per_call(fused_fb)}


def run(label, Nn, D, A, cont, H, custom, warmup, learns):
    agents = {False: make_agent(Nn, D, A, cont, H, custom, False),
              True: make_agent(Nn, D, A, cont, H, custom, True)}
    p0 = [torch.cat([p.detach().flatten() for p in a.network.parameters()]) for a in agents.values()]
    assert torch.equal(p0[0], p0[1]), "the two agents must start from equal weights"
    ro, _ = synth(T, Nn, D, A, cont, seed=1)
    ms = {False: [], True: []}
    for i in range(warmup + learns):
        st = np.random.get_state()
        for flag in (False, True):
            np.random.set_state(st)     # both agents draw the same minibatch permutations
            t = timed(agents[flag], ro)
            if i >= warmup:
                ms[flag].append(t)
    cfg = agents[True].cfg
    out = {"label": label, "T": T, "N": Nn, "D": D, "A": A, "continuous": cont, "H": H,
           "custom_network": custom, "epochs": cfg.num_epochs, "minibatches": cfg.num_minibatches,
           "learns": learns, "warmup": warmup,
           "loss_head_calls": agents[True]._learner.loss_head_calls}
    for flag, key in ((False, "torch"), (True, "fused")):
        out[key] = {"ms_median": statistics.median(ms[flag]), "ms_min": min(ms[flag]),
                    "ms_max": max(ms[flag])}
    a, b = out["torch"], out["fused"]
    out["ranges_overlap"] = not (a["ms_max"] < b["ms_min"] or b["ms_max"] < a["ms_min"])
    out["fused_over_torch_median"] = b["ms_median"] / a["ms_median"]
    d = (torch.cat([p.detach().flatten() for p in agents[True].network.parameters()])
         - torch.cat([p.detach().flatten() for p in agents[False].network.parameters()]))
    out["max_param_diff_after_run"] = float(d.abs().max())
    for ag in agents.values():
        ag.close()
    out["kernel_events"] = kernel_events(T * Nn // cfg.num_minibatches, T * Nn, A, cont)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--learns", type=int, default=20)
    ap.add_argument("--only", default=None, help="run one label")
    ap.add_argument("--kernels-only", action="store_true",
                    help="only the loss-head calls on minibatch-sized inputs (for a kernel trace)")
    a = ap.parse_args()
    torch.set_num_threads(min(16, torch.get_num_threads()))
    res = {"device": torch.cuda.get_device_name(0), "shapes": []}
    for s in SHAPES:
        if a.only and s[0] != a.only:
            continue
        if a.kernels_only:
            label, Nn, _, A, cont, _, _ = s
            r = {"label": label, "kernel_events": kernel_events(T * Nn // 8, T * Nn, A, cont, 50)}
        else:
            r = run(*s, a.warmup, a.learns)
        print(json.dumps(r), flush=True)
        res["shapes"].append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
