"""One rank of a two-process job on ONE GPU through the drop-in agents on the GENERIC learn
(NativeLearner._learn_generic), under DPPO_COMM=peer, for tests/test_gpu_generic_dp.py.  Modelled
on tests/dist_scripts/wide_peer_dp.py.

One agent per process: PPO or ContinuousPPO with a subclass of the default network (no fused
class claims it), the initial parameters of generic_dp_cases.case_setup.  Two consecutive learns
on this rank's env shard of two different global synthetic rollouts, fused_loss as the case says,
np.random seeded with generic_dp_cases.perm_seed right before each so the test can redraw the
permutations.  After each learn the parameters, the learner's m and v and loss_head_calls go to
`out_path` (npz).  Test infrastructure only."""
import os
import sys

import numpy as np


def _paths():
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for p in (os.path.join(root, "diamond-ppo_amd"), root, os.path.join(root, "tests"),
              os.path.join(root, "tests", "golden")):
        if p not in sys.path:
            sys.path.insert(0, p)


def run_case(rank, world, out, case):
    import torch
    import diamond
    import generic_dp_cases as G
    import wide_dp_cases as C
    from gpu_helpers import SpecEnvs
    c = G.CASES[case]
    g = c["geom"]
    T, Nl, M, cont = g["T"], g["Nl"], g["M"], c["cont"]
    assert world == G.WORLD
    base = diamond.continuous_ppo.ContinuousActorCriticNetwork if cont else \
        diamond.ppo.ActorCriticNetwork

    class CustomNet(base):
        pass

    Cfg = diamond.ContinuousPPOConfig if cont else diamond.PPOConfig
    Agent = diamond.ContinuousPPO if cont else diamond.PPO
    cfg = Cfg(rollout_steps=T, num_envs=Nl, num_minibatches=M, num_epochs=G.E, verbose=False,
              network_hidden_dim=G.HIDDEN, global_minibatches=c["gmb"])
    agent = Agent(None, cfg, network_cls=CustomNet, envs=SpecEnvs(c["D"], c["A"], cont))
    L = agent._learner
    assert L.fused is False and L.shape_class is None, (L.fused, L.shape_class)
    assert L.world == world and L.rank == rank and L.peer, (L.world, L.rank)
    assert L.global_mb == c["gmb"]
    names, params, hosts = G.case_setup(case)
    assert [n for n, _ in agent.network.named_parameters()] == list(names)
    sd = {n: torch.from_numpy(params[n]) for n in names}
    if hasattr(agent.network, "actor_out_layer"):
        sd["actor_out_layer.weight"] = sd["actor_head.2.weight"]
        sd["actor_out_layer.bias"] = sd["actor_head.2.bias"]
    agent.network.load_state_dict(sd)
    res = {}
    for n, p in agent.network.named_parameters():
        res["init/" + n] = p.detach().cpu().numpy().copy()
    for k in range(G.LEARNS):
        agent.fused_loss = c["fused_loss"][k]
        ro = diamond.engine.stage_experience(C.shard(hosts[k], rank, Nl), agent.device, cont)
        np.random.seed(G.perm_seed(case, k, rank))
        agent.learn_device(ro)
        torch.cuda.synchronize()
        for n, p in agent.network.named_parameters():
            res[f"final{k}/" + n] = p.detach().cpu().numpy().copy()
        res[f"m{k}"] = L.m.cpu().numpy().copy()
        res[f"v{k}"] = L.v.cpu().numpy().copy()
        res[f"calls{k}"] = int(L.loss_head_calls)
    np.savez(out, **res)
    L.close()


def run(rank, world, port, case, out):
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
        run_case(rank, world, out, case)
        dist.barrier()
    finally:
        dist.destroy_process_group()
