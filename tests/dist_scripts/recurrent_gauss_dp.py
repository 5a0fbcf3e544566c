"""RecurrentContinuousPPO learn() in one rank of a world of `world` processes (gloo process group,
every rank on cuda:0), for tests/test_gpu_gru_gauss_learn.py: tests/dist_scripts/recurrent_dp.py
with the Gaussian agent.  Each rank learns on its slice of one synthetic rollout of the global env
axis and writes its flat parameters; then it evaluates one more minibatch gradient of its slice by
hand (divisor: the union minibatch), all-reduces it and writes that too, so the caller can hold
the summed actor_log_std gradient against the oracle's on the union batch.  Test infrastructure
only."""
import ctypes
import os
import sys

import numpy as np


def synth_experience(T, Ng, D, A, G, device, params, seed=0):
    """One rollout in RecurrentContinuousPPO.rollout()'s layout for the GLOBAL env axis: the rows of
    recurrent_dp.synth_experience with float32 actions [N, A] = the float64 oracle's mean under
    ``params`` + N(0, 1), and log_probs = the oracle's + 0.2 N(0, 1), so the ratios sit on both
    sides of the clip."""
    import torch
    import gru_gauss_oracle as GO
    rng = np.random.default_rng(seed)
    obs = rng.standard_normal((T, Ng, D)).astype(np.float32)
    hx = (rng.standard_normal((1, Ng, G)) * 0.5).astype(np.float32)
    pd = rng.random((T, Ng)) < 0.1
    mean, _ = GO.forward(params, obs, pd, hx[0])
    sigma = np.exp(np.asarray(params["actor_log_std"], np.float64))
    act = (mean + sigma * rng.standard_normal(mean.shape)).astype(np.float32)
    lp = GO.log_probs(params, obs, act, pd, hx[0]) + 0.2 * rng.standard_normal((T, Ng))
    g = lambda x, dt=torch.float32: torch.as_tensor(x, dtype=dt, device=device)
    exp = []
    hx_t = g(hx)
    for t in range(T):
        exp.append([g(obs[t]), g(act[t]), rng.normal(1.0, 1.0, Ng), rng.random(Ng) < 0.05,
                    rng.random(Ng) < 0.02, g(pd[t], torch.bool), g(lp[t]),
                    g(rng.standard_normal(Ng)), g(rng.standard_normal(Ng)), hx_t])
    return exp


def shard(exp, lo, hi):
    return [[x[lo:hi] for x in row[:9]] + [row[9][:, lo:hi].contiguous()] for row in exp]


def probe_batch(T, Ng, A, seed=9):
    """Advantages, returns and old log-prob offsets of the hand-made gradient call."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((T, Ng)).astype(np.float32),
            rng.standard_normal((T, Ng)).astype(np.float32),
            (0.2 * rng.standard_normal((T, Ng))).astype(np.float32))


def run(rank, world, port, T, Ng, D, A, out_path, gru_hidden_dim=16):
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for p in (os.path.join(root, "diamond-ppo_amd"), os.path.join(root, "tests", "golden"),
              os.path.join(root, "tests"), root):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["LOCAL_RANK"] = "0"          # every rank on the one GPU
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    import diamond
    import gym_stub
    from diamond import _native as N
    from diamond.engine import hparams
    G = gru_hidden_dim
    Nl = Ng // world
    cfg = diamond.RecurrentContinuousPPOConfig(rollout_steps=T, num_envs=Nl, num_epochs=3,
                                               num_minibatches=1, verbose=False,
                                               gru_hidden_dim=G)
    envs = gym_stub.SyncVectorEnv(
        [lambda: gym_stub.SyntheticEnv(D, continuous=True, act_dim=A)] * Nl)
    agent = diamond.RecurrentContinuousPPO(None, cfg, envs=envs)
    assert agent.gru is not None and agent.gru.gauss, "the agent did not take the fused path"
    init = agent.flat.flat.cpu().numpy()
    params = {n: p.detach().cpu().numpy().copy() for n, p in agent.network.named_parameters()}
    exp = synth_experience(T, Ng, D, A, G, agent.device, params)
    lo, hi = rank * Nl, (rank + 1) * Nl
    agent.learn(shard(exp, lo, hi))
    torch.cuda.synchronize()
    final = agent.flat.flat.cpu().numpy()
    # one more gradient by hand: this rank's slice, every sample, divisor = the union's size
    adv, ret, dlp = probe_batch(T, Ng, A)
    dev = agent.device
    c = lambda x: x.contiguous()
    obs = c(torch.stack([r[0] for r in exp])[:, lo:hi])
    act = c(torch.stack([r[1] for r in exp])[:, lo:hi])
    pd = c(torch.stack([r[5] for r in exp])[:, lo:hi].to(torch.uint8))
    old = c(torch.stack([r[6] for r in exp])[:, lo:hi] + torch.from_numpy(dlp[:, lo:hi]).to(dev))
    adv_t, ret_t = (c(torch.from_numpy(x[:, lo:hi]).to(dev)) for x in (adv, ret))
    hx0 = c(exp[0][9][0, lo:hi])
    batch = N.GruGaussBatch(obs.data_ptr(), act.data_ptr(), old.data_ptr(), adv_t.data_ptr(),
                            ret_t.data_ptr(), pd.data_ptr(), hx0.data_ptr())
    idx = torch.arange(T * Nl, dtype=torch.int32, device=dev)
    hp = hparams(cfg, cfg.lr, 0)
    grad = torch.zeros(agent.flat.total + 8, device=dev)
    N.check(agent.gru.lib.dppo_gru_gauss_minibatch_grad_f32(
        agent.gru.h, agent.flat.flat.data_ptr(), ctypes.byref(batch), idx.data_ptr(), T * Nl,
        T * Ng, ctypes.byref(hp), grad.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
        "dppo_gru_gauss_minibatch_grad_f32")
    torch.cuda.synchronize()
    if world > 1:
        dist.all_reduce(grad)
    np.savez(out_path, init=init, final=final, grad=grad.cpu().numpy())
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
