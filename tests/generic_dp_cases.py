"""Cases, seeds and the two-rank NumPy restatement shared by tests/test_generic_dp_cpu.py,
tests/test_gpu_generic_dp.py and tests/dist_scripts/generic_dp.py: the generic learn
(NativeLearner._learn_generic: GAE -> global advantage statistics -> loss scaled by this rank's
share -> all-reduce of the flat gradient -> clip + Adam) on two ranks.  Test infrastructure only;
nothing here touches the GPU.

A case is one spawn of two processes: a drop-in agent with a subclass of the default network (so
no fused class claims it), two consecutive learns on two different synthetic rollouts, one with
the torch loss and one with the loss-head kernel.

case  agent                    minibatches  geometry                        fused_loss per learn
B1    PPO D 8 A 4              local        wide_dp_cases.AGENT (8, 16, 2)  off, on
B2    ContinuousPPO D 17 A 6   local        the same                        on, off
B3    PPO D 8 A 3              global       T 4, 4 envs per rank, M 8       on, off
B4    ContinuousPPO D 5 A 2    global       the same                        off, on

Global minibatches hold 4 samples, so a rank's share is 0 to 4 of them: empty, single-sample and
full shares all occur on both ranks in both learns (asserted in the CPU module for the seeds
below).

np.random is seeded right before each learn: PERM_SEED + 10 * learn + rank with local minibatches,
PERM_SEED + 10 * learn on both ranks with global ones, so the tests redraw what the learn drew.
"""
import numpy as np

from oracle import ppo_np as P

import wide_dp_cases as C
from gpu_helpers import synth_host

WORLD = 2
HIDDEN = 64          # PPOConfig.network_hidden_dim's default
E = C.E              # what wide_dp_cases' helpers assume; the agents' num_epochs is set to it
PERM_SEED = 3        # RandomState(3): the draw of wide_dp_cases.UNEVEN_PERM_SEED
GLOBAL_GEOM = dict(T=4, Nl=4, M=8)
BOUND = 2e-5         # |param - oracle|: test_two_processes_drop_in_agents / check_vs_oracle

CASES = {
    "B1": dict(cont=False, D=8, A=4, gmb=False, geom=C.AGENT, fused_loss=(False, True), data=7100),
    "B2": dict(cont=True, D=17, A=6, gmb=False, geom=C.AGENT, fused_loss=(True, False), data=7200),
    "B3": dict(cont=False, D=8, A=3, gmb=True, geom=GLOBAL_GEOM, fused_loss=(True, False),
               data=7300),
    "B4": dict(cont=True, D=5, A=2, gmb=True, geom=GLOBAL_GEOM, fused_loss=(False, True),
               data=7400),
}
LEARNS = 2


def perm_seed(case, learn, rank):
    return PERM_SEED + 10 * learn + (0 if CASES[case]["gmb"] else rank)


def case_setup(case):
    """(names, initial parameters, [rollout of the global batch per learn])."""
    c = CASES[case]
    g = c["geom"]
    _, names, params, _, host0 = C.setup(HIDDEN, g["T"], g["Nl"], c["D"], c["A"], c["cont"],
                                         c["data"], world=WORLD)
    hosts = [host0]
    for k in range(1, LEARNS):
        h = synth_host(g["T"], g["Nl"] * WORLD, c["D"], c["A"], c["cont"], c["data"] + k)
        hosts.append(tuple(x if x.dtype != np.uint8 else x.astype(bool) for x in h))
    return names, params, hosts


def drawn_perms(case):
    """What each learn draws.  Per learn: the [E][Bg] global permutations (global minibatches),
    or the list of the ranks' [E][B] local ones."""
    c = CASES[case]
    g = c["geom"]
    B = g["T"] * g["Nl"]
    out = []
    for k in range(LEARNS):
        if c["gmb"]:
            out.append(C.global_perms(perm_seed(case, k, 0), B * WORLD)[0])
        else:
            out.append([C.global_perms(perm_seed(case, k, r), B)[0] for r in range(WORLD)])
    return out


def oracle_perms(case):
    """The global permutations the oracle learns with: the drawn ones, or the union of the ranks'
    local minibatches."""
    c = CASES[case]
    g = c["geom"]
    return [p if c["gmb"] else C.union_perms(p, g["T"], g["Nl"], g["M"], world=WORLD)
            for p in drawn_perms(case)]


def oracle(case):
    """wide_dp_cases.oracle_learns of the two-rank global batch: per learn (trace, parameters)."""
    c = CASES[case]
    names, params, hosts = case_setup(case)
    return C.oracle_learns(params, names, hosts, oracle_perms(case), c["cont"], c["geom"]["M"])


def nonempty_minibatches(case, learn, rank):
    """How many of the learn's E * M minibatches hold a sample of this rank."""
    c = CASES[case]
    g = c["geom"]
    if not c["gmb"]:
        return E * g["M"]
    counts = C.share_counts(drawn_perms(case)[learn], g["Nl"], g["M"], world=WORLD)
    return int((counts[:, :, rank] > 0).sum())


MISTAKES = ("weight_1_over_world", "local_stats", "skip_empty", "beta_unweighted")


def two_rank_learns(case, mistake=None):
    """The engine's decomposition restated with the oracle's pieces.  Every rank keeps its own
    replica of the parameters and the Adam state, as the processes do.  Per learn and rank:
    P.old_policy and P.gae of the rank's env shard; statistics from the ranks' summed float64
    {sum, sum^2} finalised with n = T * N * world (csrc/gae.hip mean_std_from); per minibatch
    P.minibatch_loss_grads of the rank's members with m_total chosen so that the means carry the
    engine's weight (k / mbp of a global minibatch, 1 / world of a local one), the float32 sum of
    the ranks' gradients, then P.clip_grad_norm and P.adam_step on every replica.  Returns, per
    learn, the list of the ranks' parameter dicts.

    `mistake` (one of MISTAKES) applies one of the errors the GPU tests exist to catch."""
    assert mistake is None or mistake in MISTAKES
    c = CASES[case]
    g = c["geom"]
    T, Nl, M, cont, gmb = g["T"], g["Nl"], g["M"], c["cont"], c["gmb"]
    names, params0, hosts = case_setup(case)
    hp = P.Hyper(num_minibatches=M, num_epochs=E)
    beta = np.float32(hp.entropy_beta)
    reps = [{n: params0[n].copy() for n in names} for _ in range(WORLD)]
    adams = [P.new_adam_state(reps[r], names) for r in range(WORLD)]
    B = T * Nl
    out = []
    for host, perms in zip(hosts, drawn_perms(case)):
        ranks = []
        for r in range(WORLD):
            sl = slice(r * Nl, (r + 1) * Nl)
            obs, nobs, act, rew, te, tr = (x[:, sl] for x in host)
            logp, v, nv, _ = P.old_policy(reps[r], obs, act, nobs, cont)
            adv = P.gae(rew, te, tr, v, nv, hp.gamma, hp.gae_lambda)
            ranks.append(dict(obs=obs.reshape(B, -1), act=act.reshape(B, *act.shape[2:]),
                              logp=logp.reshape(B), adv=adv, ret=(v + adv).reshape(B)))
        s = sum(x["adv"].astype(np.float64).sum() for x in ranks)
        q = sum((x["adv"].astype(np.float64) ** 2).sum() for x in ranks)
        n = float(B * WORLD)
        mu = s / n
        mean, std = np.float32(mu), np.float32(np.sqrt(max((q - s * mu) / (n - 1.0), 0.0)))
        for x in ranks:
            if mistake == "local_stats":
                x["adv"] = P.normalize_adv(x["adv"]).reshape(B)
            else:
                x["adv"] = ((x["adv"] - mean) / (std + np.float32(1e-6))).reshape(B)
        if gmb:
            Ng = Nl * WORLD
            mbp = B * WORLD // M
            pg = perms.astype(np.int64).reshape(E, M, mbp)
            t_, n_ = np.divmod(pg, Ng)
        else:
            mb = B // M
        for e in range(E):
            for j in range(M):
                grads, ks = [], []
                for r in range(WORLD):
                    if gmb:
                        keep = (n_[e, j] >= r * Nl) & (n_[e, j] < (r + 1) * Nl)
                        ii = t_[e, j][keep] * Nl + n_[e, j][keep] - r * Nl
                        m_total = mbp
                        if mistake == "weight_1_over_world":
                            m_total = max(len(ii), 1) * WORLD
                    else:
                        ii = perms[r][e, j * mb:(j + 1) * mb].astype(np.int64)
                        m_total = mb * WORLD
                    ks.append(len(ii))
                    if len(ii) == 0:
                        grads.append({k: np.zeros_like(reps[r][k]) for k in names})
                        continue
                    x = ranks[r]
                    _, _, gr = P.minibatch_loss_grads(reps[r], x["obs"][ii], x["act"][ii],
                                                      x["logp"][ii], x["adv"][ii], x["ret"][ii],
                                                      hp, cont, m_total=m_total)
                    if cont and mistake != "beta_unweighted":
                        # the oracle subtracts a whole beta: the entropy mean over all m_total
                        # samples; this rank holds len(ii) of them
                        share = np.float32(len(ii) / m_total)
                        gr["actor_log_std"] = (gr["actor_log_std"] + beta) - beta * share
                    grads.append(gr)
                total = {k: (grads[0][k] + grads[1][k]).astype(np.float32) for k in names}
                for r in range(WORLD):
                    if mistake == "skip_empty" and ks[r] == 0:
                        continue
                    gcopy = {k: total[k].copy() for k in names}
                    P.clip_grad_norm(gcopy, names, hp.grad_norm_clip)
                    P.adam_step(reps[r], gcopy, adams[r], names, 3e-4, hp.adam_eps)
        out.append([{n: reps[r][n].copy() for n in names} for r in range(WORLD)])
    return out


def distance(params, ref_params, names):
    return max(float(np.abs(params[n].astype(np.float64) - ref_params[n]).max()) for n in names)


# ---- A.1: the statistics of dppo_gae_f32 as csrc/gae.hip takes them --------------------------
STATS_SHAPES = [(16, 48), (7, 33), (129, 64)]   # (T, envs per shard): pipelined with three
#                                                 16-env tiles, serial, two super-chunks
STATS_REGIMES = ["plain", "large_mean"]


def stats_inputs(T, Nl, regime):
    """(rewards, term, trunc, values, next_values) of the two-shard batch [T][2 * Nl]: the draws
    of test_gae_vs_oracle_sizes, or of test_gae_stats_large_mean (every step terminal,
    v = -1000)."""
    Nn = 2 * Nl
    if regime == "plain":
        rng = np.random.default_rng(T * 31 + Nn)
        r = rng.normal(1, 1, (T, Nn)).astype(np.float32)
        te = (rng.random((T, Nn)) < 0.02).astype(np.uint8)
        tr = (rng.random((T, Nn)) < 0.005).astype(np.uint8)
        v = rng.standard_normal((T, Nn)).astype(np.float32)
        nv = rng.standard_normal((T, Nn)).astype(np.float32)
    else:
        rng = np.random.default_rng(T * 7 + Nn)
        r = rng.standard_normal((T, Nn)).astype(np.float32)
        te = np.ones((T, Nn), np.uint8)
        tr = np.zeros((T, Nn), np.uint8)
        v = np.full((T, Nn), -1000.0, np.float32)
        nv = rng.standard_normal((T, Nn)).astype(np.float32)
    return r, te, tr, v, nv


def _wave_sum(x):
    """common.h wave_sum_f64 over 64 lanes, in its order."""
    x = np.asarray(x, np.float64).copy()
    i = np.arange(64)
    x = x + x[i ^ 1]
    x = x + x[i ^ 2]
    x = x + x[(i & ~7) | (7 - (i & 7))]
    x = x + x[(i & ~15) | (15 - (i & 15))]
    return (x[0] + x[16]) + (x[32] + x[48])


def _partials_sum(p):
    """gae.hip partials_sum256 for up to 256 partials."""
    s = np.zeros(256, np.float64)
    s[:len(p)] = p
    w = 128
    while w >= 1:
        s[:w] = s[:w] + s[w:2 * w]
        w //= 2
    return s[0]


def restated_sums(adv):
    """{sum, sum^2} of one shard's advantages [T][N] as dppo_gae_f32's kernels accumulate them
    (N below the 32- and 64-env tiles' thresholds, as every shape here).

    N % 16 == 0: the pipelined kernel with 16-env tiles -- each lane takes the 4 advantages of one
    step and 4 neighbouring envs in float32, shifted by the first of them (stats4: s += dx,
    q = fma(dx, dx, q)), folds them into its float64 sums (stats_fold), and the sums go lane ->
    wave -> workgroup -> launch in the kernels' fixed order.  Otherwise the serial kernel: one
    lane per env, float64 throughout."""
    adv = np.asarray(adv, np.float32)
    T, Nn = adv.shape
    f32, f64 = np.float32, np.float64
    parts = []
    if Nn % 16 == 0:
        nsup = (T + 127) // 128
        for tile in range(Nn // 16):
            wsum = np.zeros((8, 2))
            for k in range(8):               # chunk k: rows 16 k .. 16 k + 15 of a super-chunk
                lanes = np.zeros((64, 2))
                for lane in range(64):
                    row, e0 = lane // 4, 4 * (lane % 4)
                    ls = lq = 0.0
                    for s in range(nsup):
                        hi = T - s * 128
                        lo = max(hi - 128, 0)
                        nr = min(16, hi - lo - 16 * k)
                        s32, q32, sft, cnt = f32(0), f32(0), f32(0), 0
                        if row < nr:
                            av = adv[lo + 16 * k + row, tile * 16 + e0:tile * 16 + e0 + 4]
                            sft = av[0]
                            for a in av:
                                dx = f32(a - sft)
                                s32 = f32(s32 + dx)
                                q32 = f32(f64(dx) * f64(dx) + f64(q32))   # fmaf
                            cnt = 4
                        ds, dn, dsum = f64(sft), f64(cnt), f64(s32)
                        ls += dsum + dn * ds
                        lq += f64(q32) + ds * (2.0 * dsum + dn * ds)
                    lanes[lane] = ls, lq
                wsum[k] = _wave_sum(lanes[:, 0]), _wave_sum(lanes[:, 1])
            s0 = s1 = 0.0
            for k in range(8):
                s0 += wsum[k, 0]
                s1 += wsum[k, 1]
            parts.append((s0, s1))
    else:
        for tile in range((Nn + 15) // 16):
            lane = np.zeros((16, 2))
            for e in range(16):
                n = tile * 16 + e
                if n >= Nn:
                    continue
                s0 = s1 = 0.0
                for t in range(T - 1, -1, -1):
                    a = f64(adv[t, n])
                    s0 += a
                    s1 += a * a
                lane[e] = s0, s1
            for off in (8, 4, 2, 1):         # __shfl_down within 16 lanes; lane 0 is the result
                nxt = lane.copy()
                nxt[:16 - off] = lane[:16 - off] + lane[off:]
                lane = nxt
            parts.append((lane[0, 0], lane[0, 1]))
    parts = np.array(parts)
    return _partials_sum(parts[:, 0]), _partials_sum(parts[:, 1])


def exact_sums(adv):
    """The float64 sum and sum of squares of the float32 advantages, correctly rounded."""
    import math
    x = np.asarray(adv, np.float64).ravel()
    return math.fsum(x), math.fsum(x * x)
