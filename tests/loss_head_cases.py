"""Inputs, float64 yardstick and bounds shared by the loss-head tests (CPU and GPU files).

A case is one minibatch for ``dppo_ppo_loss_f32``: the network outputs ``logits`` [m, A] (or
Gaussian means with ``log_std``), ``values`` [m], and the rollout-flat arrays ``actions``,
``old_logp``, ``adv``, ``ret`` of length B that the kernel reads through ``idx``.  Every array is
stored as the float32 (or integer) the kernel receives; the yardstick evaluates those same numbers.

Yardstick: float64 torch autograd of the reference's minibatch loss (the text of
``NativeLearner._learn_generic``, restated in ``torch_loss``) on the CPU.

Branch condition: a float32 ratio within rounding of ``1 +- eps`` may take the other branch of
the clipped surrogate, so ``old_logp`` is built from the float64 log-prob and a target ratio, by
thirds of the samples: inside the clip range (1 +- 0.9 eps), above it ((1 + eps) x 1.0083..1.425)
and below it ((1 - eps) x 0.375..0.9875) -- 0.82-1.18, 1.21-1.71 and 0.30-0.79 at eps = 0.2.
``branch_margin`` returns the smallest distance of any sample's ratio from a bound; every case
must keep it >= NEAR_BOUND with no sample left out (tests/test_loss_head_cpu.py).
"""
from types import SimpleNamespace as Case

import numpy as np
import torch

NEAR_BOUND = 1e-3
HYPERS = [(0.2, 1.0, 0.01), (0.1, 0.5, 0.0), (0.3, 2.0, 0.05)]  # (eps, c_v, beta)
M_SIZES = [1, 63, 64, 65, 257, 4099]
A_SIZES = [1, 2, 3, 4, 5, 7, 8, 16, 17, 33, 64]   # plus the cap read from the library
REGIMES = ["plain", "gaps", "sigma_small", "sigma_big", "ret100", "adv0"]


def _logp64(logits, log_std, actions_mb, cont):
    x = logits.astype(np.float64)
    if cont:
        ls = np.broadcast_to(log_std.astype(np.float64), x.shape)
        z = (actions_mb.astype(np.float64) - x) / np.exp(ls)
        return (-0.5 * z * z - ls - 0.5 * np.log(2 * np.pi)).sum(-1)
    mx = x.max(-1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(x - mx).sum(-1))
    return x[np.arange(len(x)), actions_mb] - lse


def make_case(m, A, cont, *, hyper=0, scale=1.0, use_idx=True, ls_stride=0, regime="plain",
              seed=0, on_policy=False):
    eps, cv, beta = HYPERS[hyper]
    rng = np.random.default_rng(1000 * seed + 7 * m + A + (500 if cont else 0))
    B = m + m // 2 + 3 if use_idx else m
    if use_idx:
        idx = rng.integers(0, B, size=m).astype(np.int64)   # duplicates allowed
    else:
        idx = np.arange(m, dtype=np.int64)
    first = {}
    src = np.array([first.setdefault(int(i), s) for s, i in enumerate(idx)])  # row sharing old_logp

    gain = 1.0
    if regime == "gaps" and not cont:
        gain = 60.0
    logits = (rng.standard_normal((m, A)) * gain).astype(np.float32)
    if regime == "gaps" and not cont and A > 1:
        logits = np.clip(logits, -115.0, 115.0)
        logits[0, 0], logits[0, -1] = 115.0, -115.0      # one gap of exactly 230
    logits = logits[src]
    values = rng.standard_normal(m).astype(np.float32)[src]
    log_std = None
    if cont:
        sigma = {"sigma_small": 0.05, "sigma_big": 4.5}.get(regime)
        if sigma is None:
            row = (rng.standard_normal((m if ls_stride else 1, A)) * 0.3 - 0.5)
        else:
            row = np.full((m if ls_stride else 1, A), np.log(sigma))
            row = row + rng.standard_normal(row.shape) * 0.01
        log_std = row.astype(np.float32)
        if ls_stride:
            log_std = log_std[src]
        out = 4.0 if sigma is not None else 1.0            # actions four sigma out
        sgn = np.where(rng.random((B, A)) < 0.5, -1.0, 1.0)
        dev_ = (sgn * out if sigma is not None else rng.standard_normal((B, A)))
        mean_of = np.zeros((B, A))
        mean_of[idx] = logits
        sd_of = np.ones((B, A))
        sd_of[idx] = np.exp(np.broadcast_to(log_std, (m, A)).astype(np.float64))
        actions = (mean_of + dev_ * sd_of).astype(np.float32)
        act_mb = actions[idx]
    else:
        actions = rng.integers(0, A, size=B).astype(np.int32)
        act_mb = actions[idx]

    lp = _logp64(logits, log_std, act_mb, cont)
    third = np.arange(m) % 3 if m >= 3 else np.zeros(m, int)
    third = third[src]
    u = rng.random(m)[src]
    target = np.where(third == 0, 1.0 + 0.9 * eps * (2 * u - 1),
                      np.where(third == 1, (1 + eps) * (1.0083 + u * (1.425 - 1.0083)),
                               (1 - eps) * (0.375 + u * (0.9875 - 0.375))))
    old = np.zeros(B, np.float32)
    old[idx] = (lp - np.log(target)).astype(np.float32)
    if on_policy:
        old[idx] = lp.astype(np.float32)
    adv = rng.standard_normal(B).astype(np.float32)
    # both advantage signs in each ratio third (where the minibatch has six samples to hold them)
    uniq = np.array(sorted(first.values()))
    for t in range(3):
        rows = uniq[third[uniq] == t]
        if len(rows) >= 2:
            adv[idx[rows[0]]] = abs(adv[idx[rows[0]]]) + 0.1
            adv[idx[rows[1]]] = -abs(adv[idx[rows[1]]]) - 0.1
    if regime == "adv0":
        adv[rng.random(B) < 0.5] = 0.0
    ret = rng.standard_normal(B).astype(np.float32)
    if regime == "ret100":
        ret *= 100.0
    return Case(m=m, A=A, B=B, cont=cont, eps=eps, cv=cv, beta=beta, scale=scale,
                idx=idx if use_idx else None, gather=idx, logits=logits, values=values,
                log_std=log_std, ls_stride=A if (cont and ls_stride) else 0, actions=actions,
                old_logp=old, adv=adv, ret=ret, regime=regime, third=third)


def branch_margin(c):
    """Smallest |ratio - (1 +- eps)| over the samples, in float64 on the stored inputs."""
    lp = _logp64(c.logits, c.log_std, c.actions[c.gather], c.cont)
    r = np.exp(lp - c.old_logp[c.gather].astype(np.float64))
    return float(np.minimum(np.abs(r - (1 - c.eps)), np.abs(r - (1 + c.eps))).min())


def torch_loss(c, dtype):
    """The reference's minibatch loss under torch autograd in `dtype` on the CPU (the text of
    NativeLearner._learn_generic): {loss, policy, value, entropy, clipfrac} and the gradients with
    respect to logits [m, A], values [m] and the dense log_std [m, A]."""
    t = lambda a: torch.from_numpy(np.array(a)).to(dtype)
    mb_idx = torch.from_numpy(c.gather)
    lg = t(c.logits).requires_grad_(True)
    new_v = t(c.values).requires_grad_(True)
    log_probs, adv, ret = t(c.old_logp), t(c.adv), t(c.ret)
    ls_full = None
    if c.cont:
        acts = t(c.actions)
        ls_full = t(np.broadcast_to(c.log_std, c.logits.shape)).requires_grad_(True)
        dist = torch.distributions.Normal(loc=lg, scale=ls_full.exp())
        new_lp = dist.log_prob(acts[mb_idx]).sum(-1)
        ent = dist.entropy().sum(-1).mean()
    else:
        acts = torch.from_numpy(c.actions).long()
        dist = torch.distributions.Categorical(logits=lg)
        new_lp = dist.log_prob(acts[mb_idx])
        ent = dist.entropy().mean()
    ratio = (new_lp - log_probs[mb_idx]).exp()
    a_mb = adv[mb_idx]
    l_pi = torch.max(-a_mb * ratio, -a_mb * torch.clamp(ratio, 1.0 - c.eps, 1.0 + c.eps)).mean()
    l_v = 0.5 * torch.nn.functional.mse_loss(new_v, ret[mb_idx])
    loss = l_pi + c.cv * l_v + -c.beta * ent
    loss = loss * c.scale
    loss.backward()
    frac = ((ratio < 1.0 - c.eps) | (ratio > 1.0 + c.eps)).double().mean()
    parts = np.array([loss.item(), l_pi.item(), l_v.item(), ent.item(), frac.item()])
    g = {"d_logits": lg.grad.double().numpy(), "d_values": new_v.grad.double().numpy()}
    if c.cont:
        g["d_log_std"] = ls_full.grad.double().numpy()
    return parts, g


def analytic(c):
    """The kernel's closed-form backward (csrc/losshead.hip) in float64 numpy."""
    x = c.logits.astype(np.float64)
    m, A = x.shape
    i = c.gather
    a = c.adv[i].astype(np.float64)
    w = c.scale / m
    lo, hi = 1.0 - c.eps, 1.0 + c.eps
    if c.cont:
        ls = np.broadcast_to(c.log_std.astype(np.float64), x.shape)
        z = (c.actions[i].astype(np.float64) - x) * np.exp(-ls)
        lp = (-0.5 * z * z - ls - 0.5 * np.log(2 * np.pi)).sum(-1)
        H = (0.5 + 0.5 * np.log(2 * np.pi) + ls).sum(-1)
    else:
        mx = x.max(-1, keepdims=True)
        e = np.exp(x - mx)
        se = e.sum(-1, keepdims=True)
        lpk = x - (mx + np.log(se))
        p = e / se
        lp = lpk[np.arange(m), c.actions[i]]
        plp = np.where(p == 0.0, 0.0, p * lpk)
        H = -plp.sum(-1)
    r = np.exp(lp - c.old_logp[i].astype(np.float64))
    rc = np.clip(r, lo, hi)
    t1, t2 = -a * r, -a * rc
    g1 = np.where(t1 > t2, 1.0, np.where(t1 == t2, 0.5, 0.0))
    passed = ((r >= lo) & (r <= hi)).astype(np.float64)
    dlp = (g1 * -a + (1 - g1) * passed * -a) * r
    dv = c.values.astype(np.float64) - c.ret[i].astype(np.float64)
    g = {"d_values": w * c.cv * dv}
    if c.cont:
        g["d_logits"] = w * dlp[:, None] * z * np.exp(-ls)
        g["d_log_std"] = w * (dlp[:, None] * (z * z - 1.0) - c.beta)
    else:
        onehot = np.zeros_like(x)
        onehot[np.arange(m), c.actions[i]] = 1.0
        dent = np.where(p == 0.0, 0.0, p * (lpk + H[:, None]))
        g["d_logits"] = w * (dlp[:, None] * (onehot - p) + c.beta * dent)
    l_pi, l_v, ent = np.maximum(t1, t2).mean(), 0.5 * (dv * dv).mean(), H.mean()
    parts = np.array([c.scale * (l_pi + c.cv * l_v - c.beta * ent), l_pi, l_v, ent,
                      ((r < lo) | (r > hi)).mean()])
    return parts, g


def grad_bound(exact, f32):
    """Largest allowed |kernel - float64| for one gradient tensor: 4x the float32 torch
    evaluation's own distance from float64, with a floor of 2e-5 max|g|
    (tests/test_gpu_production.py's convention)."""
    scale = np.abs(exact).max()
    return max(4.0 * np.abs(f32 - exact).max(), 2e-5 * scale), scale


DP_SCALES = [("1of3", 1 / 3), ("5of7", 5 / 7), ("1of8", 1 / 8)]
DP_M_SIZES = [1, 2, 5, 65]
# (m, k): one minibatch of m samples split into the shares [0, k) and [k, m) of two ranks
PARTITIONS = [(7, 1), (7, 3), (65, 1), (65, 32)]
# (Gaussian head, per-sample log_std rows): categorical, a broadcast log_std row, per-sample rows
PARTITION_HEADS = [(False, False), (True, False), (True, True)]
PARTITION_HEAD_IDS = ["cat", "gauss-broadcast", "gauss-rows"]


def partition_case(m, cont, rows):
    """The whole minibatch of a partition test (scale 1); `rows`: per-sample log_std rows."""
    return make_case(m=m, A=3 if cont else 4, cont=cont, seed=60 + m, ls_stride=1 if rows else 0)


def share(c, lo, hi):
    """Samples [lo, hi) of minibatch c as the case one rank runs: the same rollout-flat arrays,
    its rows of the network outputs, scale = its share of the minibatch."""
    kw = dict(vars(c))
    kw.update(m=hi - lo, scale=(hi - lo) / c.m, logits=c.logits[lo:hi], values=c.values[lo:hi],
              idx=c.idx[lo:hi], gather=c.gather[lo:hi], third=c.third[lo:hi])
    if c.cont and c.ls_stride:
        kw["log_std"] = c.log_std[lo:hi]
    return Case(**kw)


def sweep_cases(cap):
    """The smallest cases at which each mechanism can go wrong: (label, kwargs of make_case)."""
    out = []
    for cont in (False, True):
        # (67, 131 and cap - 1: rows of two, three and four scalar slots per lane)
        for A in A_SIZES + [cap, 67, 131, cap - 1]:
            # every lane-group width, 16-byte and scalar rows, the in-group loop; a partial group
            # at m = 65 and several blocks at 257
            out.append((f"A{A}", dict(m=65 if A < 64 else 257, A=A, cont=cont, seed=A)))
        for m in M_SIZES:
            out.append((f"m{m}", dict(m=m, A=4 if not cont else 3, cont=cont, seed=m)))
        out.append(("null-idx", dict(m=257, A=5, cont=cont, use_idx=False, seed=3)))
        out.append(("scale", dict(m=65, A=8, cont=cont, scale=0.125, seed=4)))
        # the scale as data parallelism sets it: a rank's share k / mbp of a global minibatch
        # (thirds, sevenths) or 1 / world, down to a single-sample share
        for tag, sc in DP_SCALES:
            for m in DP_M_SIZES:
                out.append((f"scale{tag}-m{m}", dict(m=m, A=4 if not cont else 3, cont=cont,
                                                      scale=sc, seed=50 + m)))
        for h in (1, 2):
            out.append((f"hyper{h}", dict(m=257, A=7, cont=cont, hyper=h, seed=5 + h)))
        out.append(("ret100", dict(m=257, A=4, cont=cont, regime="ret100", seed=8)))
        out.append(("adv0", dict(m=257, A=4, cont=cont, regime="adv0", seed=9)))
    out.append(("gaps", dict(m=257, A=16, cont=False, regime="gaps", seed=10)))
    out.append(("gaps-odd", dict(m=65, A=33, cont=False, regime="gaps", seed=11)))
    for reg in ("sigma_small", "sigma_big"):
        out.append((reg, dict(m=257, A=6, cont=True, regime=reg, seed=12)))
        out.append((reg + "-rows", dict(m=65, A=8, cont=True, regime=reg, ls_stride=1, seed=13)))
    out.append(("ls-rows", dict(m=257, A=17, cont=True, ls_stride=1, seed=14)))
    out.append(("ls-rows-vec", dict(m=65, A=16, cont=True, ls_stride=1, seed=15)))
    return [(f"{'gauss' if kw['cont'] else 'cat'}-{label}", kw) for label, kw in out]
