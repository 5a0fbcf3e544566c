"""One rank of a two-process job on ONE GPU through the drop-in agents at wide shapes, under
DPPO_COMM=peer (the ranks exchange through csrc/peer.hip; RCCL refuses two ranks on one device),
for tests/test_gpu_wide_dp.py.  Modelled on run_agent of tests/dist_scripts/peer_dp.py.

kind "agent": PPO at (hidden, D, A) with cfg.wide_data_parallel = `flag`; it reports the path
the learner took and, where that is the fused one, runs one learn on this rank's env shard of a
global synthetic rollout, from permutations the test can redraw (np.random seeded with
AGENT_PERM_SEED + rank right before the learn).  kind "capacity":
ContinuousPPO at a layout past the peer exchange's 65,536 elements -- the construction must raise
on every rank.  Results go to `out_path` (npz).  Test infrastructure only."""
import os
import sys

import numpy as np


def _paths():
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for p in (os.path.join(root, "diamond-ppo_amd"), root, os.path.join(root, "tests"),
              os.path.join(root, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)


def run_agent(rank, world, out, Hd, D, A, flag):
    import torch
    import diamond
    import wide_dp_cases as C
    from gpu_helpers import SpecEnvs, synth_host
    g = C.AGENT
    T, Nl, M = g["T"], g["Nl"], g["M"]
    cfg = diamond.PPOConfig(network_hidden_dim=Hd, rollout_steps=T, num_envs=Nl,
                            num_minibatches=M, verbose=False, wide_data_parallel=bool(flag))
    agent = diamond.PPO(None, cfg, envs=SpecEnvs(D, A, False))
    L = agent._learner
    assert L.world == world and L.peer, (L.world, getattr(L, "peer", None))
    res = {"shape_class": str(L.shape_class), "fused": int(L.fused), "wide_ranks": L.dims.wide_ranks}
    for n, p in agent.network.named_parameters():
        res["init/" + n] = p.detach().cpu().numpy().copy()
    if L.fused:
        host = synth_host(T, Nl * world, D, A, False, C.AGENT_DATA_SEED + Hd + D)
        ro = diamond.engine.stage_experience(C.shard(host, rank, Nl), agent.device, False)
        np.random.seed(C.AGENT_PERM_SEED + rank)
        agent.learn_device(ro)
        torch.cuda.synchronize()
        res["trace"] = agent.learn_trace()
        for n, p in agent.network.named_parameters():
            res["final/" + n] = p.detach().cpu().numpy().copy()
    np.savez(out, **res)
    L.close()


def run_capacity(rank, world, out):
    import diamond
    import wide_dp_cases as C
    from gpu_helpers import SpecEnvs
    Hd, D, A, cont = C.OVER_CAPACITY
    cfg = diamond.ContinuousPPOConfig(network_hidden_dim=Hd, rollout_steps=8, num_envs=16,
                                      verbose=False, wide_data_parallel=True)
    err = ""
    try:
        diamond.ContinuousPPO(None, cfg, envs=SpecEnvs(D, A, cont))
    except RuntimeError as e:
        err = str(e)
    np.savez(out, err=err)


def run(rank, world, port, kind, out, args=()):
    _paths()
    os.environ["LOCAL_RANK"] = "0"          # every rank on the one GPU
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"], os.environ["WORLD_SIZE"] = str(rank), str(world)
    os.environ["DPPO_COMM"] = "peer"
    os.environ["DPPO_PEER_TIMEOUT_S"] = "30"
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        {"agent": run_agent, "capacity": run_capacity}[kind](rank, world, out, *args)
        dist.barrier()
    finally:
        dist.destroy_process_group()
