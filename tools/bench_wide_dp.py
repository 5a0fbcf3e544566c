#!/usr/bin/env python3
"""Time learn_device() of two data-parallel ranks at the wide shapes, fused against generic.

    python tools/bench_wide_dp.py --out profiles/wide_learn_dp.json

Two processes on ONE GPU (every rank on device 0, DPPO_COMM=peer: RCCL refuses two ranks on one
device), a stub env (spaces only), T = 128, the three shapes of tools/bench_wide.py at 2,048 and
4,096 envs per rank.  Per shape and size the ranks build the agent with
cfg.wide_data_parallel on (the fused wide learn, csrc/mbwide.hip) and off (the generic
torch-autograd learn, today's default), alternating on, off, on, off (`--rounds`); each build runs
`--warmup` untimed learns and `--learns` timed ones, every learn bracketed by a device
synchronisation, a barrier of the ranks and host wall clock.  Reported per mode: the median of all
timed learns with min and max, and each round's median.

The ranks TIME-SHARE one device: their kernels interleave on the same compute units, so neither
column is a scaling number and nothing here says what a second GPU buys.  The ratio of the two
columns is the figure: the same two ranks, the same device, fused against generic.
"""
import argparse
import json
import multiprocessing as mp
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [
    ("LunarLander-128", 8, 4, False, 128),
    ("HalfCheetah-128", 17, 6, True, 128),
    ("Ant-64", 105, 8, True, 64),
]
SIZES = [2048, 4096]
T = 128


def _paths():
    for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "diamond-ppo_amd"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)


def time_mode(rank, D, A, cont, H, Nl, flag, warmup, learns):
    import numpy as np
    import torch
    import torch.distributed as dist
    import diamond
    from gpu_helpers import SpecEnvs, synth
    Cfg = diamond.ContinuousPPOConfig if cont else diamond.PPOConfig
    Agent = diamond.ContinuousPPO if cont else diamond.PPO
    cfg = Cfg(network_hidden_dim=H, rollout_steps=T, num_envs=Nl, verbose=False,
              wide_data_parallel=flag)
    torch.manual_seed(0)
    agent = Agent(None, cfg, envs=SpecEnvs(D, A, cont))
    np.random.seed(rank)
    L = agent._learner
    assert L.peer and L.fused == flag, (L.peer, L.fused, flag)
    ro, _ = synth(T, Nl, D, A, cont, seed=1 + rank)
    for _ in range(warmup):
        agent.learn_device(ro)
    ms = []
    for _ in range(learns):
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        agent.learn_device(ro)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    torch.cuda.synchronize()
    dist.barrier()
    L.close()
    return ms


def rank_main(rank, world, port, a, q):
    _paths()
    os.environ.update(LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      RANK=str(rank), WORLD_SIZE=str(world), DPPO_COMM="peer")
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        for label, D, A, cont, H in SHAPES:
            if a["only"] and label != a["only"]:
                continue
            for Nl in a["sizes"]:
                rounds = {True: [], False: []}
                for _ in range(a["rounds"]):
                    for flag in (True, False):
                        rounds[flag].append(time_mode(rank, D, A, cont, H, Nl, flag, a["warmup"],
                                                      a["learns"]))
                row = {"label": label, "T": T, "N_per_rank": Nl, "ranks": world, "D": D, "A": A,
                       "continuous": cont, "H": H, "rank": rank, "learns": a["learns"],
                       "warmup": a["warmup"], "rounds": a["rounds"]}
                for flag, key in ((True, "fused"), (False, "generic")):
                    flat = [x for r in rounds[flag] for x in r]
                    row[key] = {"ms_median": statistics.median(flat), "ms_min": min(flat),
                                "ms_max": max(flat),
                                "round_medians": [statistics.median(r) for r in rounds[flag]]}
                row["generic_over_fused"] = row["generic"]["ms_median"] / row["fused"]["ms_median"]
                row["spreads_overlap"] = row["fused"]["ms_max"] >= row["generic"]["ms_min"]
                q.put(row)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--learns", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="*", default=SIZES)
    ap.add_argument("--only", default=None, help="run one label")
    ap.add_argument("--timeout", type=float, default=900.0, help="seconds for the whole sweep")
    a = vars(ap.parse_args())
    world = 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=rank_main, args=(r, world, port, a, q)) for r in range(world)]
    for p in procs:
        p.start()
    n_rows = world * len(a["sizes"]) * sum(1 for s in SHAPES if not a["only"] or s[0] == a["only"])
    rows, deadline = [], time.monotonic() + a["timeout"]
    try:
        while len(rows) < n_rows:
            left = deadline - time.monotonic()
            if left <= 0 or not all(p.is_alive() or p.exitcode == 0 for p in procs):
                break
            try:
                row = q.get(timeout=min(left, 5.0))
            except Exception:
                continue
            print(json.dumps(row), flush=True)
            rows.append(row)
    finally:
        for p in procs:
            p.join(30)
        for p in procs:
            if p.is_alive():
                p.kill()
    ok = len(rows) == n_rows and all(p.exitcode == 0 for p in procs)
    if a["out"] and rows:
        import torch
        _paths()
        res = {"device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else None,
               "note": "two ranks time-share ONE device (DPPO_COMM=peer): not a scaling number",
               "complete": ok, "rows": sorted(rows, key=lambda r: (r["label"], r["N_per_rank"],
                                                                    r["rank"]))}
        os.makedirs(os.path.dirname(os.path.abspath(a["out"])), exist_ok=True)
        with open(a["out"], "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
