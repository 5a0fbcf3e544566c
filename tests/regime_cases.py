"""Numerical regimes shared by tests/test_regimes_cpu.py and tests/test_gpu_regimes.py: the inputs
a trained policy produces and the other suites never draw -- saturated hidden units,
near-deterministic categorical policies, narrow and wide Gaussians, actions several sigma from
the mean, observations far from unit scale, returns in the hundreds.  Test infrastructure only;
NumPy, the oracle and the layout query, nothing here touches the GPU.

A regime is a named transform of (params, obs, next_obs, actions, rewards), applied after
gpu_helpers.random_params / synth_host (MLP families) or through gru_cases.Case's scale fields
(GRU).  Near regimes keep the project's float32 bounds; in the far ones float32 itself degrades
(the float32 oracle's own distance from the float64 one reaches 1e-4 of max|g|), so the kernel is
held to a multiple of that distance and they run on-policy only.
"""
from dataclasses import dataclass

import numpy as np

import gru_cases
import gru_wide_cases
from diamond import _native as N
from oracle import gru_torch as GT
from oracle import ppo_np as P

from gpu_helpers import flat32, offpolicy_inputs, random_params, synth_host

f32 = np.float32
T, NN, M, RAGGED = 16, 96, 4, 5     # B = 1536, minibatch B / M - 5 = 379 (no multiple of 16)
SAT = 0.999                         # |tanh| beyond which a unit counts as saturated
NEAR_CAP, FAR_CAP = 1e-5, 1e-3      # on the float32 oracle's gradient error / max|g|
TENSOR_CAP = 5e-5   # near regimes, float32 oracle, per tensor / max(own scale, 1e-3 max|g|): half
#                     the 1e-4 the kernels are held to


@dataclass(frozen=True)
class Regime:
    name: str
    far: bool = False
    head: str | None = None        # "cat" / "gauss": runs on those shapes only
    obs: float = 1.0               # scale on obs and next_obs
    hidden: float = 1.0            # scale on base.0, base.2 and both heads' first weight matrix
    actor_out: float = 1.0         # scale on actor_head.2.weight (the logits)
    rewards: float = 1.0
    log_std: float | None = None   # actor_log_std set to this value
    tail: float | None = None      # actions = mean + tail * sigma * N(0, 1)

    def __str__(self):
        return self.name

    def transform(self):
        """The regime as a function of (params, obs, next_obs, actions, rewards)."""
        def apply(params, obs, next_obs, actions, rewards):
            cont = "actor_log_std" in params
            assert self.head is None or (self.head == "gauss") == cont, self.name
            head = "actor_mean_head" if cont else "actor_head"
            p = {k: np.array(v, f32) for k, v in params.items()}
            for n in ("base.0.weight", "base.2.weight", f"{head}.0.weight",
                      "critic_head.0.weight"):
                p[n] = p[n] * f32(self.hidden)
            p[f"{head}.2.weight"] = p[f"{head}.2.weight"] * f32(self.actor_out)
            if self.log_std is not None:
                p["actor_log_std"] = np.full_like(p["actor_log_std"], self.log_std)
            obs, next_obs = obs * f32(self.obs), next_obs * f32(self.obs)
            rewards = rewards * f32(self.rewards)
            if self.tail is not None:
                p64 = {k: v.astype(np.float64) for k, v in p.items()}
                mean = P.forward(p64, obs, True, np.float64)["out"]
                z = np.random.default_rng(4000 + mean.shape[-1]).standard_normal(mean.shape)
                actions = (mean + self.tail * np.exp(p64["actor_log_std"]) * z).astype(f32)
            return p, obs, next_obs, actions, rewards
        return apply


def identity(params, obs, next_obs, actions, rewards):
    return params, obs, next_obs, actions, rewards


REGIMES = {r.name: r for r in [
    Regime("obs30", obs=30.0),
    Regime("obs1e-3", obs=1e-3),
    Regime("hidden6", hidden=6.0),
    Regime("peaked20", head="cat", actor_out=20.0),
    Regime("peaked30", head="cat", actor_out=30.0),
    Regime("returns100", rewards=100.0),
    Regime("sigma.05", head="gauss", log_std=-3.0, tail=1.0),
    Regime("sigma4.5", head="gauss", log_std=1.5, tail=1.0),
    Regime("tail4", head="gauss", tail=4.0),
    Regime("obs1000", far=True, obs=1000.0),
    Regime("peaked60", far=True, head="cat", actor_out=60.0),
    Regime("combined", far=True, head="cat", obs=30.0, hidden=6.0, actor_out=20.0),
]}
NEAR = [r for r in REGIMES.values() if not r.far]
SAMPLER_REGIMES = ["obs30", "hidden6", "peaked20", "peaked30", "sigma.05", "sigma4.5"]

# (family, hidden, D, A, Gaussian head): one shape per kernel path
SHAPES = [
    ("sample-split", 64, 8, 4, False),
    ("sample-split", 64, 16, 8, False),   # the MFMA heads
    ("sample-split", 64, 3, 1, True),
    ("sample-split", 64, 17, 6, True),
    ("two-team", 64, 32, 16, False),
    ("two-team", 64, 5, 10, True),
    ("wide", 128, 8, 4, False),
    ("wide", 128, 105, 8, True),
    ("wide", 64, 40, 5, False),
]
LEARN_SHAPES = [SHAPES[0], SHAPES[4], SHAPES[6]]   # one categorical shape per family
LEARN_REGIMES = ["obs30", "peaked20"]


def learn_transform(regime, shape):
    """The regime applied to gpu_helpers.random_params' weights in place of the agent's initial
    ones (whose actor output layer has gain 0.01: 20 times that is still a near-uniform policy)."""
    _, Hd, D, A, cont = shape

    def apply(params, *data):
        L = N.param_layout(dims(shape))
        rng = np.random.default_rng(5000 + case_seed(regime, shape))
        drawn, _ = random_params(L, names_of(cont), D, A, cont, rng)
        assert {k: v.shape for k, v in drawn.items()} == {k: v.shape for k, v in params.items()}
        return regime.transform()(drawn, *data)
    return apply


def shape_id(shape):
    fam, Hd, D, A, cont = shape
    return f"{fam}-H{Hd}-D{D}-A{A}-{'gauss' if cont else 'cat'}"


def fits(regime, shape):
    return regime.head is None or (regime.head == "gauss") == shape[4]


def mlp_cases(regimes=None):
    """(regime, shape) of every regime on every shape whose head it applies to."""
    regimes = REGIMES.values() if regimes is None else regimes
    return [(r, s) for r in regimes for s in SHAPES if fits(r, s)]


def case_id(case):
    return f"{case[0].name}-{shape_id(case[1])}"


# cases whose first draw misses a condition of tests/test_regimes_cpu.py take a later seed that
# meets it: a logit gap, the far cap on the float32 oracle's error, and on the one-action Gaussian
# shape a gradient tensor of a single entry that cancels to 1e-3 of max|g|, where the float32
# oracle itself is 1e-4 .. 2e-3 of the floored scale away from the float64 one
SEED_BUMP = {("peaked30", "wide-H128-D8-A4-cat"): 3, ("peaked30", "wide-H64-D40-A5-cat"): 1,
             ("combined", "wide-H64-D40-A5-cat"): 1, ("hidden6", "sample-split-H64-D3-A1-gauss"): 7,
             ("tail4", "sample-split-H64-D3-A1-gauss"): 6,
             ("sigma.05", "sample-split-H64-D3-A1-gauss"): 4}


def case_seed(regime, shape):
    bump = SEED_BUMP.get((regime.name, shape_id(shape)), 0)
    return 100 * list(REGIMES).index(regime.name) + SHAPES.index(shape) + 2000 * bump


def names_of(cont):
    return P.CONTINUOUS_NAMES if cont else P.DISCRETE_NAMES


def dims(shape, E=4):
    _, Hd, D, A, cont = shape
    return N.Dims(T, NN, D, A, int(cont), Hd, E, M, 1, 0)


def minibatch_size():
    return T * NN // M - RAGGED


def build_onpolicy(regime, shape):
    """Parameters, rollout and minibatch indices of one on-policy gradient case, drawn as
    tests/test_gpu_shapes.py _check draws them and then moved into the regime."""
    _, Hd, D, A, cont = shape
    seed = case_seed(regime, shape)
    L = N.param_layout(dims(shape))
    names = names_of(cont)
    params, _ = random_params(L, names, D, A, cont, np.random.default_rng(1000 + seed))
    host = synth_host(T, NN, D, A, cont, 2000 + seed)
    params, *data = regime.transform()(params, *host[:4])
    host = (*data, *host[4:])
    B = T * NN
    idx = np.random.RandomState(3000 + seed).permutation(B)[:minibatch_size()].astype(np.int32)
    return dict(L=L, names=names, params=params, flat=flat32(L, names, params), host=host, idx=idx)


# ---------------------------------------------------------------------------------------------
# Off-policy: gpu_helpers.offpolicy_inputs in the regime.  The noise scale s of a case (table at
# the end of the file) is one of 0.2, 0.1, 0.05, 0.03, 0.02, 0.01 (mostly the largest) at which
# check_offpolicy_conditions holds (tests/test_regimes_cpu.py asserts it): saturated layers and
# sharp heads turn a small step in the weights into a large one in the log-prob, so s is mostly
# below the default regime's 0.2 / 0.03.  Where the observations hardly reach the policy (obs1e-3)
# or the Gaussian is wide (sigma4.5, one action) the ratio moves little and s is up to 1.
# ---------------------------------------------------------------------------------------------
OFFPOLICY_KEY = {False: "clip.1", True: "clip.3"}   # by Gaussian head
OFFPOLICY_S = {}   # filled below: (regime name, shape id) -> s


def offpolicy_hyper(shape):
    from gpu_helpers import offpolicy_hyper as hyper
    return hyper(OFFPOLICY_KEY[shape[4]])


def build_offpolicy(regime, shape, s=None):
    _, Hd, D, A, cont = shape
    L = N.param_layout(dims(shape))
    names = names_of(cont)
    hy = offpolicy_hyper(shape)
    s = OFFPOLICY_S[(regime.name, shape_id(shape))] if s is None else s
    c = offpolicy_inputs(L, names, D, A, cont, T, NN, minibatch_size(), hy, s,
                         case_seed(regime, shape), transform=regime.transform())
    return L, names, hy, c


def reached(params, obs, actions, cont):
    """What a case reaches, from the float64 oracle: the share of layer-1 / layer-2 units beyond
    SAT, the largest layer-1 pre-activation, the largest logit gap of a sample (categorical) and
    the smallest log-prob of a taken action."""
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    D = obs.shape[-1]
    x = np.asarray(obs, np.float64).reshape(-1, D)
    f = P.forward(p64, x, cont, np.float64)
    pre1 = x @ p64["base.0.weight"].T + p64["base.0.bias"]
    out = dict(sat1=float((np.abs(f["h1"]) > SAT).mean()),
               sat2=float((np.abs(f["h2"]) > SAT).mean()), pre1=float(np.abs(pre1).max()))
    if cont:
        a = np.asarray(actions, np.float64).reshape(x.shape[0], -1)
        lp = P.normal_logp_entropy(f["out"], p64["actor_log_std"], a, np.float64)[0]
    else:
        lp, ent, _, _ = P.categorical_logp_entropy(f["out"], np.asarray(actions).reshape(-1),
                                                   np.float64)
        out["gap"] = float((f["out"].max(1) - f["out"].min(1)).max())
        out["entropy"] = float(ent.mean())
    out["min_logp"] = float(lp.min())
    return out


def oracle_pair(params, args, hy, cont, m_total=None):
    """The float32 and the float64 oracle on one minibatch: {dtype: (loss, comps, flat grads)} and
    err_oracle32 = max|g32 - g64| / max|g64|."""
    names = names_of(cont)
    res = {}
    for dt in (np.float32, np.float64):
        loss, comps, grads = P.minibatch_loss_grads(params, *args, hy, cont, m_total=m_total, dt=dt)
        res[dt] = (loss, comps, np.concatenate([np.asarray(grads[n], np.float64).ravel()
                                                for n in names]))
    exact = res[np.float64][2]
    return res, float(np.abs(res[np.float32][2] - exact).max() / np.abs(exact).max())


# ---------------------------------------------------------------------------------------------
# GRU: the same ideas through gru_cases.Case's scale fields, all in the near class, on- and
# off-policy (old log-probs = the parameters' own plus 0.25 * N(0, 1): ratios on both sides of
# 1 +- clip in every regime).  The GRU cases' output layer (gain 0.01 + 0.3 N(0, 1)) is about twice
# the MLP's scale and grows with the shape, so the scale that reaches a regime's range is set per
# shape: logit gaps 59-61 (peaked20) and 91-94 with log-probs to -84 / -90 (peaked30), 0.54-0.57 of
# the gates and 0.69-0.72 of the candidates saturated (hidden6).  seed_shift picks weights and data
# at which the float32 autograd oracle (up to 9 recurrent steps) stays under the near cap with
# room for another BLAS: 2e-6 .. 8.4e-6 here.
# ---------------------------------------------------------------------------------------------
GRU_SHAPES = [gru_cases.MID, (9, 18, 32, 16)]
_MID, _BIG = GRU_SHAPES
GRU_REGIMES = {   # name -> {shape: Case fields}
    "obs30": {_MID: dict(obs_scale=30.0), _BIG: dict(obs_scale=30.0)},
    "hidden6": {_MID: dict(gru_scale=6.0, seed_shift=2000),
                _BIG: dict(gru_scale=5.0, seed_shift=3000)},
    "peaked20": {_MID: dict(actor_scale=11.0, seed_shift=3000),
                 _BIG: dict(actor_scale=8.0, seed_shift=3000)},
    "peaked30": {_MID: dict(actor_scale=17.0, seed_shift=3000),
                 _BIG: dict(actor_scale=12.0, seed_shift=2000)},
    "returns100": {_MID: dict(ret_scale=100.0), _BIG: dict(ret_scale=100.0)},
}
GRU_OLD_NOISE = 0.25
GRU_CASES = [gru_cases.Case(f"{r}-{'x'.join(map(str, s))}-{'on' if on else 'off'}", s,
                            frac=1.0 if on else 0.4, on_policy=on,
                            old_noise=0.0 if on else GRU_OLD_NOISE, **kw)
             for r, row in GRU_REGIMES.items() for s, kw in row.items() for on in (True, False)]


# ---------------------------------------------------------------------------------------------
# The same five regimes at gru_hidden_dim 32 and 64 (csrc/grugrad.hip, csrc/gruact.hip), through
# gru_wide_cases.Case.  The G = 16 scales do not carry over: the heads read 32 / 64 hidden units, so
# the same actor_scale gives gaps of 65 to 157, and the recurrent map at gru_scale 5 - 6 is chaotic
# at these widths (the float32 autograd oracle itself ends 7e-5 .. 2e-2 of max|g| from the float64
# one).  The scales were chosen per (G, shape) with the oracles alone, never with a kernel:
#   peaked20 / peaked30: the smallest actor_scale on a 0.5 grid that reaches the regime;
#   hidden6: the largest gru_scale of 6, 5, 4, 3.5, 3, 2.5, 2 that reaches it;
#   seed_shift: the first of base .. base + 7, base 0, 1000, 2000, 3000, at which the guards hold
#   and the float32 oracle is under 0.85 of the cap (room for another BLAS) both on- and off-policy.
# Reached (float64) and err_oracle32 (on / off):
#   G 32 (7,17,5,3)    peaked20 gap 56.5   2.7e-6 / 3.1e-6    peaked30 gap 103.7 logp -83.1  3.2e-6 / 3.5e-6
#   G 32 (9,18,32,16)  peaked20 gap 56.0   1.5e-6 / 2.3e-6    peaked30 gap  90.8 logp -90.8  5.3e-6 / 6.1e-6
#   G 64 (7,17,5,3)    peaked20 gap 57.3   4.5e-6 / 6.7e-6    peaked30 gap  90.7 logp -90.7  5.6e-6 / 8.0e-6
#   G 64 (9,18,32,16)  peaked20 gap 56.9   2.3e-6 / 3.1e-6    peaked30 gap  98.0 logp -84.7  7.0e-6 / 7.6e-6
#   obs30: 0.84 - 0.95 of the base units saturated, 7.3e-7 .. 7.0e-6; returns100: 3.3e-7 .. 7.1e-7
# Far rows (GRU_WIDE_FAR): hidden6, all four.  At every grid scale that reaches the regime (>= 3.5)
# the recurrent map amplifies rounding from step to step, so the float32 oracle's error is a
# draw from a wide band rather than a property of the case: over seeds 0 .. 7 it spans 1e-5 .. 9e-3
# at G 64 and 4e-6 .. 3e-4 at G 32, a run under NEAR_CAP on one machine is at 2e-5 on another CPU,
# and one ulp on the weights (gru_oracle32_nudged) moves it by a factor of up to 50.  No scale has
# a seed among the 32 at which the float32 oracle and its three nudged draws all meet NEAR_CAP, on-
# and off-policy; so these rows run on-policy only, at gru_scale 6, the largest grid scale at which
# a seed has the float32 oracle and its nudged draws under 0.85 FAR_CAP (the first such seed):
#   G 32 (7,17,5,3)    gates 0.55 candidates 0.69   err_oracle32 1.9e-4, nudged to 3.2e-4
#   G 32 (9,18,32,16)  gates 0.65 candidates 0.79   1.6e-4, nudged to 4.0e-4
#   G 64 (7,17,5,3)    gates 0.60 candidates 0.69   1.4e-4, nudged to 2.2e-4   (seed_shift 3)
#   G 64 (9,18,32,16)  gates 0.66 candidates 0.78   1.6e-4, nudged to 5.9e-4   (seed_shift 6)
# The kernel is held to the far rule there: finite, err <= 4 err_oracle32 + 1e-6, err <= 1e-3.
# ---------------------------------------------------------------------------------------------
GRU_WIDE_REGIMES = {   # (G, shape) -> {name: Case fields}
    (32, _MID): {"obs30": dict(obs_scale=30.0), "hidden6": dict(gru_scale=6.0),
                 "peaked20": dict(actor_scale=6.0), "peaked30": dict(actor_scale=11.0),
                 "returns100": dict(ret_scale=100.0)},
    (32, _BIG): {"obs30": dict(obs_scale=30.0), "hidden6": dict(gru_scale=6.0),
                 "peaked20": dict(actor_scale=6.5), "peaked30": dict(actor_scale=10.5),
                 "returns100": dict(ret_scale=100.0)},
    (64, _MID): {"obs30": dict(obs_scale=30.0), "hidden6": dict(gru_scale=6.0, seed_shift=3),
                 "peaked20": dict(actor_scale=6.0), "peaked30": dict(actor_scale=9.5),
                 "returns100": dict(ret_scale=100.0)},
    (64, _BIG): {"obs30": dict(obs_scale=30.0), "hidden6": dict(gru_scale=6.0, seed_shift=6),
                 "peaked20": dict(actor_scale=4.5),
                 "peaked30": dict(actor_scale=9.0, seed_shift=1001),
                 "returns100": dict(ret_scale=100.0)},
}
GRU_WIDE_FAR = {("hidden6", g, s) for g in gru_wide_cases.WIDTHS for s in GRU_SHAPES}
GRU_WIDE_CASES = [gru_wide_cases.Case(f"{r}-{'x'.join(map(str, s))}-{'on' if on else 'off'}", s,
                                      frac=1.0 if on else 0.4, on_policy=on,
                                      old_noise=0.0 if on else GRU_OLD_NOISE, G=g, **kw)
                  for (g, s), row in GRU_WIDE_REGIMES.items() for r, kw in row.items()
                  for on in (True, False) if on or (r, g, s) not in GRU_WIDE_FAR]


def gru_build(case):
    """gru_cases.build, or gru_wide_cases.build for a case with a G of its own."""
    return (gru_wide_cases.build if hasattr(case, "G") else gru_cases.build)(case)


def gru_regime(case):
    return case.name.split("-")[0]


def gru_is_far(case):
    return (gru_regime(case), getattr(case, "G", gru_cases.G), case.shape) in GRU_WIDE_FAR


def gru_reached(params, x):
    """Float64: share of base units beyond SAT, share of gate values within 1e-3 of 0 or 1, share
    of candidate values beyond SAT, largest logit gap, smallest log-prob of a taken action."""
    import torch
    d = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    p = {k: d(v) for k, v in params.items()}
    obs, pd, h = d(x["obs"]), torch.as_tensor(np.asarray(x["prev_dones"], bool)), d(x["hx0"])
    G = p["gru.weight_hh_l0"].shape[1]
    F = torch.nn.functional
    x1 = torch.tanh(F.linear(obs, p["base.0.weight"], p["base.0.bias"]))
    gi = F.linear(x1, p["gru.weight_ih_l0"], p["gru.bias_ih_l0"])
    gates, cands = [], []
    for t in range(obs.shape[0]):
        h = h * (~pd[t]).to(h.dtype)[:, None]
        gh = F.linear(h, p["gru.weight_hh_l0"], p["gru.bias_hh_l0"])
        r = torch.sigmoid(gi[t, :, :G] + gh[:, :G])
        z = torch.sigmoid(gi[t, :, G:2 * G] + gh[:, G:2 * G])
        n = torch.tanh(gi[t, :, 2 * G:] + r * gh[:, 2 * G:])
        h = (1 - z) * n + z * h
        gates += [r, z]
        cands.append(n)
    gates, cands = torch.stack(gates).numpy(), torch.stack(cands).numpy()
    logits, _ = GT.sequence(p, obs, pd, d(x["hx0"]))
    logits = logits.numpy()
    lp = GT.log_probs(params, x["obs"], x["actions"], x["prev_dones"], x["hx0"])
    return dict(sat1=float((np.abs(x1.numpy()) > SAT).mean()),
                gates=float((np.abs(gates - 0.5) > 0.499).mean()),
                cand=float((np.abs(cands) > SAT).mean()),
                gap=float((logits.max(-1) - logits.min(-1)).max()), min_logp=float(lp.min()))


def gru_oracle_pair(case, params, x, mb_idx, m_total):
    """As oracle_pair, for the GRU: {dtype: (loss sums, grads dict)} and err_oracle32."""
    import torch
    res = {}
    for dt in (torch.float32, torch.float64):
        res[dt] = GT.minibatch_grads(params, x["obs"], x["actions"], x["old_log_probs"],
                                     x["advantages"], x["returns"], x["prev_dones"], x["hx0"],
                                     mb_idx, m_total, case.clip, case.vf, case.ent, dt=dt)
    g32, g64 = res[torch.float32][1], res[torch.float64][1]
    scale = max(np.abs(g).max() for g in g64.values())
    err = max(np.abs(g32[n].astype(np.float64) - g64[n]).max() for n in g64) / scale
    return res, float(err)


def gru_oracle32_nudged(case, params, x, mb_idx, m_total, draws=3):
    """err_oracle32 of the float32 oracle run on weights moved by one float32 ulp each, up or
    down at random (seeded), against the float64 oracle on the weights as they are: what another
    rounding of the same arithmetic does to the figure.  Where the recurrent map is chaotic (large
    gru_scale at gru_hidden_dim 32 / 64) it moves by a factor of up to 50, and one float32 run under
    a cap says little; the wide hidden6 rows are chosen so that these draws meet the cap as well."""
    import torch
    a = (x["obs"], x["actions"], x["old_log_probs"], x["advantages"], x["returns"],
         x["prev_dones"], x["hx0"], mb_idx, m_total, case.clip, case.vf, case.ent)
    g64 = GT.minibatch_grads(params, *a, dt=torch.float64)[1]
    scale = max(np.abs(g).max() for g in g64.values())
    rng = np.random.default_rng(1)
    errs = []
    for _ in range(draws):
        p = {n: np.nextafter(v, np.where(rng.random(v.shape) < 0.5, -np.inf, np.inf).astype(f32))
             for n, v in params.items()}
        g32 = GT.minibatch_grads(p, *a, dt=torch.float32)[1]
        errs.append(float(max(np.abs(g32[n].astype(np.float64) - g64[n]).max() for n in g64)
                          / scale))
    return errs


# ---------------------------------------------------------------------------------------------
# Rollout samplers: n = 33 observations per (regime, shape).
# ---------------------------------------------------------------------------------------------
SAMPLER_N = 33
SAMPLER_SHAPES = [SHAPES[0], SHAPES[3], SHAPES[4], SHAPES[5], SHAPES[6], SHAPES[7], SHAPES[8]]
SEED, COUNTER = 0x0DD5_EED5_1234_ABCD, 1   # a counter at which every discrete case is clear
GRU_SAMPLER_SHAPES = [(5, 3), (32, 16)]   # (D, A)
GRU_SAMPLER_REGIMES = ["obs30", "hidden6", "peaked20", "peaked30"]


def sampler_cases():
    return [(REGIMES[r], s) for r in SAMPLER_REGIMES for s in SAMPLER_SHAPES
            if fits(REGIMES[r], s)]


def sampler_inputs(regime, shape):
    """(params, flat, obs [n][D]) of one sampler case."""
    _, Hd, D, A, cont = shape
    seed = case_seed(regime, shape)
    L = N.param_layout(N.Dims(4, 32, D, A, int(cont), Hd, 1, 1, 1, 0))
    names = names_of(cont)
    params, _ = random_params(L, names, D, A, cont, np.random.default_rng(7000 + seed))
    obs = np.random.default_rng(9000 + seed).standard_normal((SAMPLER_N, D), dtype=np.float32)
    act = np.zeros((SAMPLER_N, A), f32) if cont else np.zeros(SAMPLER_N, np.int32)
    params, obs, *_ = regime.transform()(params, obs, obs, act, np.zeros(SAMPLER_N, f32))
    return params, flat32(L, names, params), obs


def gru_sampler_inputs(regime, D, A, G=gru_cases.G):
    """(params, obs [n][D], prev dones [n], hidden state [n][G], next obs) of one GRU rollout-step
    case: tests/gru_cases.py's weights in the regime (at G = 32 / 64 with the scales of
    GRU_WIDE_REGIMES), the inputs of tests/test_gpu_gru_act.py."""
    table = GRU_REGIMES[regime] if G == gru_cases.G else \
        {s: row[regime] for (g, s), row in GRU_WIDE_REGIMES.items() if g == G}
    kw = next(dict(kw) for s, kw in table.items() if s[2:] == (D, A))
    kw.pop("seed_shift", None)
    case = gru_cases.Case(regime, (1, SAMPLER_N, D, A), **kw)
    rng = np.random.default_rng(600 + D)
    params = {n: (p + 0.3 * rng.standard_normal(p.shape)).astype(f32)
              for n, p in gru_cases.initial_params(D, A, G=G).items()}
    params = gru_cases.scaled_params(params, case)
    k = f32(case.obs_scale)
    obs = rng.standard_normal((SAMPLER_N, D)).astype(f32) * k
    nobs = rng.standard_normal((SAMPLER_N, D)).astype(f32) * k
    dones = rng.random(SAMPLER_N) < 0.3
    hx = (rng.standard_normal((SAMPLER_N, G)) * 0.5).astype(f32)
    return params, obs, dones, hx, nobs


def gru_step_logits(params, obs, dones, hx):
    """Float64 logits [n][A] of one rollout step."""
    import torch
    d = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    with torch.no_grad():
        lg, _ = GT.sequence({k: d(v) for k, v in params.items()}, d(obs)[None],
                            torch.as_tensor(np.asarray(dones, bool))[None], d(hx))
    return lg[0].numpy()


OFFPOLICY_S.update({(r, s): v for r, row in {
    "obs30": {
        "sample-split-H64-D8-A4-cat": 0.2,
        "sample-split-H64-D16-A8-cat": 0.2,
        "sample-split-H64-D3-A1-gauss": 0.05,
        "sample-split-H64-D17-A6-gauss": 0.03,
        "two-team-H64-D32-A16-cat": 0.2,
        "two-team-H64-D5-A10-gauss": 0.02,
        "wide-H128-D8-A4-cat": 0.2,
        "wide-H128-D105-A8-gauss": 0.02,
        "wide-H64-D40-A5-cat": 0.2},
    "obs1e-3": {
        "sample-split-H64-D8-A4-cat": 1.0,
        "sample-split-H64-D16-A8-cat": 1.0,
        "sample-split-H64-D3-A1-gauss": 1.0,
        "sample-split-H64-D17-A6-gauss": 0.1,
        "two-team-H64-D32-A16-cat": 0.2,
        "two-team-H64-D5-A10-gauss": 0.1,
        "wide-H128-D8-A4-cat": 1.0,
        "wide-H128-D105-A8-gauss": 0.07,
        "wide-H64-D40-A5-cat": 0.7},
    "hidden6": {
        "sample-split-H64-D8-A4-cat": 0.2,
        "sample-split-H64-D16-A8-cat": 0.2,
        "sample-split-H64-D3-A1-gauss": 0.1,
        "sample-split-H64-D17-A6-gauss": 0.02,
        "two-team-H64-D32-A16-cat": 0.2,
        "two-team-H64-D5-A10-gauss": 0.02,
        "wide-H128-D8-A4-cat": 0.2,
        "wide-H128-D105-A8-gauss": 0.03,
        "wide-H64-D40-A5-cat": 0.2},
    "peaked20": {
        "sample-split-H64-D8-A4-cat": 0.05,
        "sample-split-H64-D16-A8-cat": 0.05,
        "two-team-H64-D32-A16-cat": 0.03,
        "wide-H128-D8-A4-cat": 0.03,
        "wide-H64-D40-A5-cat": 0.03},
    "peaked30": {
        "sample-split-H64-D8-A4-cat": 0.02,
        "sample-split-H64-D16-A8-cat": 0.03,
        "two-team-H64-D32-A16-cat": 0.02,
        "wide-H128-D8-A4-cat": 0.03,
        "wide-H64-D40-A5-cat": 0.03},
    "returns100": {
        "sample-split-H64-D8-A4-cat": 0.2,
        "sample-split-H64-D16-A8-cat": 0.2,
        "sample-split-H64-D3-A1-gauss": 0.2,
        "sample-split-H64-D17-A6-gauss": 0.05,
        "two-team-H64-D32-A16-cat": 0.2,
        "two-team-H64-D5-A10-gauss": 0.05,
        "wide-H128-D8-A4-cat": 0.2,
        "wide-H128-D105-A8-gauss": 0.05,
        "wide-H64-D40-A5-cat": 0.2},
    "sigma.05": {
        "sample-split-H64-D3-A1-gauss": 0.05,
        "sample-split-H64-D17-A6-gauss": 0.01,
        "two-team-H64-D5-A10-gauss": 0.01,
        "wide-H128-D105-A8-gauss": 0.01},
    "sigma4.5": {
        "sample-split-H64-D3-A1-gauss": 1.0,
        "sample-split-H64-D17-A6-gauss": 0.1,
        "two-team-H64-D5-A10-gauss": 0.1,
        "wide-H128-D105-A8-gauss": 0.2},
    "tail4": {
        "sample-split-H64-D3-A1-gauss": 0.2,
        "sample-split-H64-D17-A6-gauss": 0.01,
        "two-team-H64-D5-A10-gauss": 0.01,
        "wide-H128-D105-A8-gauss": 0.01},
}.items() for s, v in row.items()})
