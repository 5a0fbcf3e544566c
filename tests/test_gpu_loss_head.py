"""Loss-head kernels (csrc/losshead.hip) against float64 torch autograd of the reference's
minibatch loss, evaluated on the CPU on the same inputs (tests/loss_head_cases.py).

Bound (the convention of tests/test_gpu_production.py): a gradient tensor may be no further from
the float64 result than 4x the distance of the float32 torch evaluation of the same inputs,
computed here, with a floor of 2e-5 max|g|; the loss terms are held to rtol 1e-5 + atol 1e-5.
No case has a sample within 1e-3 of a clip bound (checked for every case, without a device, in
tests/test_loss_head_cpu.py), so the float32 kernel and the yardstick take the same branch.
Every output sits between sentinel guard regions, and every case runs twice for equal bits.

Measured on an MI355X over all cases here: the worst gradient error was 0.37 of its bound
(d_logits 1.1e-5 of max|g| against 3.2e-5, d_log_std 2.2e-5 against 6.0e-5, d_values 9.3e-8
against the 2e-5 floor; through the linear head 4.4e-6 / 1.0e-5 / 1.6e-6 of max|g| for weight,
bias and log_std), so the float32 torch evaluation's own distance, not the floor, set the bound
in the worst cases; the loss terms stayed inside rtol 1e-5 + atol 1e-5."""
import ctypes

import numpy as np
import pytest
import torch

from diamond import _native as N
from diamond import engine

import loss_head_cases as C

pytestmark = pytest.mark.gpu

GUARD = 96          # floats on either side of every output
SENTINEL = -7.25e30
CAP = 256


def dev():
    return torch.device("cuda", 0)


def stream():
    return torch.cuda.current_stream(dev()).cuda_stream


class Guarded:
    """n floats between two sentinel regions; `off` floats shift the base off 16-byte alignment."""

    def __init__(self, n, off=0):
        self.n, self.off = n, off
        self.buf = torch.full((2 * GUARD + n + off + 4,), SENTINEL, dtype=torch.float32,
                              device=dev())
        assert self.buf.data_ptr() % 16 == 0
        self.lo = GUARD + off
        self.view = self.buf[self.lo:self.lo + n]
        assert (self.view.data_ptr() % 16 == 0) == (off % 4 == 0)

    def ptr(self):
        return self.view.data_ptr()

    def get(self):
        b = self.buf.cpu().numpy()
        assert (b[:self.lo] == np.float32(SENTINEL)).all(), "guard below was written"
        assert (b[self.lo + self.n:] == np.float32(SENTINEL)).all(), "guard above was written"
        return b[self.lo:self.lo + self.n].copy()


def place(a, off=0):
    """A device copy of `a` whose base is `off` floats past a 16-byte boundary."""
    flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    buf = torch.empty(flat.numel() + off + 4, dtype=flat.dtype, device=dev())
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + flat.numel()]
    v.copy_(flat)
    return v


def run_loss(c, off=0):
    """dppo_ppo_loss_f32 on case c -> (out[8], {d_logits, d_values, d_log_std}), guards checked."""
    m, A = c.m, c.A
    lg, v = place(c.logits, off), place(c.values)
    ls = place(c.log_std, off) if c.cont else None
    idx = place(c.idx) if c.idx is not None else None
    acts = place(c.actions, off if c.cont else 0)
    old, adv, ret = place(c.old_logp), place(c.adv), place(c.ret)
    ws_floats = N.ppo_loss_plan(m, A, c.cont)[0]
    d_lg, d_v, out, ws = Guarded(m * A, off), Guarded(m), Guarded(8), Guarded(ws_floats)
    d_ls = Guarded(m * A, off) if c.cont else None
    args = N.LossArgs(
        logits=lg.data_ptr(), log_std=ls.data_ptr() if c.cont else None, values=v.data_ptr(),
        idx=idx.data_ptr() if idx is not None else None, actions=acts.data_ptr(),
        old_log_probs=old.data_ptr(), advantages=adv.data_ptr(), returns=ret.data_ptr(),
        d_logits=d_lg.ptr(), d_log_std=d_ls.ptr() if c.cont else None, d_values=d_v.ptr(),
        out=out.ptr(), workspace=ws.ptr(), m=m, rollout_len=c.B, workspace_floats=ws_floats,
        act_dim=A, continuous=int(c.cont), log_std_stride=c.ls_stride, ppo_clip=c.eps,
        value_loss_weight=c.cv, entropy_beta=c.beta, scale=c.scale)
    N.check(N.load().dppo_ppo_loss_f32(ctypes.byref(args), stream()), "dppo_ppo_loss_f32")
    torch.cuda.synchronize()
    ws.get()
    g = {"d_logits": d_lg.get().reshape(m, A), "d_values": d_v.get()}
    if c.cont:
        g["d_log_std"] = d_ls.get().reshape(m, A)
    return out.get(), g


def run_logp(c, off=0):
    lg = place(c.logits, off)
    ls = place(c.log_std, off) if c.cont else None
    idx = place(c.idx) if c.idx is not None else None
    acts = place(c.actions, off if c.cont else 0)
    lp = Guarded(c.m)
    N.check(N.load().dppo_policy_logp_f32(
        lg.data_ptr(), ls.data_ptr() if c.cont else None, c.ls_stride,
        idx.data_ptr() if idx is not None else None, acts.data_ptr(), c.m, c.B, c.A, int(c.cont),
        lp.ptr(), stream()), "dppo_policy_logp_f32")
    torch.cuda.synchronize()
    return lp.get()


def check_case(label, c, off=0, yard=None):
    """yard: the case the yardstick evaluates (default c itself)."""
    y = yard if yard is not None else c
    parts64, g64 = C.torch_loss(y, torch.float64)
    _, g32 = C.torch_loss(y, torch.float32)
    out, g = run_loss(c, off)
    out2, g2 = run_loss(c, off)
    assert out.tobytes() == out2.tobytes(), label
    for k in g:
        assert g[k].tobytes() == g2[k].tobytes(), (label, k)
    assert (out[5:] == 0).all()
    figures = {}
    for k in g64:
        bound, scale = C.grad_bound(g64[k], g32[k])
        err = np.abs(g[k].astype(np.float64) - g64[k]).max()
        figures[k] = (err / max(scale, 1e-300), bound / max(scale, 1e-300))
    print(label, "parts", out[:5], parts64, "grad err/bound (of max|g|)", figures)
    np.testing.assert_allclose(out[:5], parts64, rtol=1e-5, atol=1e-5, err_msg=label)
    for k in g64:
        bound, _ = C.grad_bound(g64[k], g32[k])
        assert np.abs(g[k].astype(np.float64) - g64[k]).max() <= bound, (label, k, figures[k])
    return out, g


SWEEP = C.sweep_cases(CAP)


def test_cap_is_what_the_sweep_assumes():
    assert N.ppo_loss_plan(1, 1)[2] == CAP


@pytest.mark.parametrize("label, kw", SWEEP, ids=[c[0] for c in SWEEP])
def test_loss_and_gradients_match_float64(label, kw):
    check_case(label, C.make_case(**kw))


@pytest.mark.parametrize("cont, rows", C.PARTITION_HEADS, ids=C.PARTITION_HEAD_IDS)
@pytest.mark.parametrize("m, k", C.PARTITIONS)
def test_shares_of_a_minibatch_reproduce_the_whole(m, k, cont, rows):
    """`scale` as data parallelism uses it: two ranks run the kernel on their shares [0, k) and
    [k, m) of one minibatch with scale = k / m and (m - k) / m.  The concatenated gradient rows
    must be the float64 gradient of the whole minibatch at scale 1 within grad_bound, and the
    shares' out[0] must add up to the whole loss within 2e-5 max(1, |loss|)."""
    c = C.partition_case(m, cont, rows)
    parts64, g64 = C.torch_loss(c, torch.float64)
    _, g32 = C.torch_loss(c, torch.float32)
    got = [run_loss(s) for s in (C.share(c, 0, k), C.share(c, k, m))]
    loss = float(got[0][0][0]) + float(got[1][0][0])
    print(f"m{m} k{k}: loss {loss} vs {parts64[0]}")
    figures = {}
    for key in g64:
        cat = np.concatenate([g[key] for _, g in got]).astype(np.float64)
        bound, scale = C.grad_bound(g64[key], g32[key])
        figures[key] = (np.abs(cat - g64[key]).max() / scale, bound / scale)
    print(f"m{m} k{k}: grad err/bound (of max|g|)", figures)
    assert abs(loss - parts64[0]) <= 2e-5 * max(1.0, abs(parts64[0]))
    for key, (err, bound) in figures.items():
        assert err <= bound, (key, err, bound)
    # the unscaled terms are each share's own means
    for (out, _), s in zip(got, (C.share(c, 0, k), C.share(c, k, m))):
        np.testing.assert_allclose(out[:5], C.torch_loss(s, torch.float64)[0], rtol=1e-5,
                                   atol=1e-5)


@pytest.mark.parametrize("cont", [False, True])
def test_second_grid_stride_pass(cont):
    """An m the plan says one pass of the capped grid cannot hold."""
    A = 33
    _, grid_cap, _ = N.ppo_loss_plan(1 << 30, A)
    per_block = 256 // 64                      # A = 33 sits on a 64-lane group
    m = grid_cap * per_block + 5
    assert N.ppo_loss_plan(m, A)[1] == grid_cap and N.ppo_loss_plan(m - 5, A)[1] == grid_cap
    check_case("second-pass", C.make_case(m=m, A=A, cont=cont, seed=21))


@pytest.mark.parametrize("cont", [False, True])
@pytest.mark.parametrize("A", [4, 8, 64, 5, CAP])
def test_base_pointers_off_16_byte_alignment(cont, A):
    """Every [.][A] array 4 bytes past a 16-byte boundary: rows that could take 16-byte accesses
    take the scalar form, with the same results."""
    c = C.make_case(m=65, A=A, cont=cont, seed=22, ls_stride=1 if A == 8 else 0)
    out_a, g_a = check_case("aligned", c, off=0)
    out_u, g_u = check_case("unaligned", c, off=1)
    np.testing.assert_allclose(out_u[:5], out_a[:5], rtol=2e-6, atol=2e-6)


@pytest.mark.parametrize("cont", [False, True])
@pytest.mark.parametrize("A, off", [(3, 0), (8, 0), (8, 1), (64, 0), (80, 0), (CAP, 0)])
def test_on_policy_ratio_is_exactly_one(cont, A, off):
    """old = dppo_policy_logp_f32 of the same logits: ratio == 1.0f bit for bit, so with eps = 0
    no sample is strictly outside [1, 1] (clip fraction exactly 0), the maximum ties and clamp
    passes: d_logits is the unclipped analytic value."""
    c = C.make_case(m=257, A=A, cont=cont, seed=23, on_policy=True)
    lp = run_logp(c, off)
    lp64 = C._logp64(c.logits, c.log_std, c.actions[c.gather], c.cont)
    np.testing.assert_allclose(lp, lp64, rtol=1e-5, atol=1e-5)
    assert lp.tobytes() == run_logp(c, off).tobytes()
    c.old_logp = c.old_logp.copy()
    c.old_logp[c.gather] = lp        # duplicates share a row, hence a log-prob
    c.eps = 0.0
    out, _ = run_loss(c, off)
    assert out[4] == 0.0, out
    # the yardstick for the gradient: the same inputs with the clip range wide open
    wide = C.Case(**{**vars(c), "eps": 10.0})
    c2 = C.Case(**{**vars(c)})
    out, g = check_case_grad_only("on-policy", c2, wide, off)
    # policy term: mean(-adv * 1)
    np.testing.assert_allclose(out[1], -c.adv[c.gather].astype(np.float64).mean(), rtol=1e-5,
                               atol=1e-5)


def check_case_grad_only(label, c, yard, off):
    _, g64 = C.torch_loss(yard, torch.float64)
    _, g32 = C.torch_loss(yard, torch.float32)
    out, g = run_loss(c, off)
    for k in g64:
        bound, scale = C.grad_bound(g64[k], g32[k])
        err = np.abs(g[k].astype(np.float64) - g64[k]).max()
        print(label, k, "err", err / scale, "bound", bound / scale)
        assert err <= bound, (label, k, err / scale, bound / scale)
    return out, g


# ---- the autograd.Function ---------------------------------------------------------------------

def _head_case(cont, A=5, m=129, F=12):
    """A case whose logits and values are a linear head's outputs on fixed features."""
    c = C.make_case(m=m, A=A, cont=cont, seed=31)
    rng = np.random.default_rng(5)
    first = {}
    src = np.array([first.setdefault(int(i), s) for s, i in enumerate(c.gather)])
    # rows sharing a rollout index share old_logp: give them the same features
    feat = rng.standard_normal((m, F)).astype(np.float32)[src]
    W = (rng.standard_normal((A + 1, F)) * 0.3).astype(np.float32)
    b = (rng.standard_normal(A + 1) * 0.1).astype(np.float32)
    o = feat.astype(np.float64) @ W.astype(np.float64).T + b
    c.logits, c.values = o[:, :A].astype(np.float32), o[:, A].astype(np.float32)
    lp = C._logp64(c.logits, c.log_std, c.actions[c.gather], c.cont)
    tgt = np.where(np.arange(m) % 3 == 0, 1.05, np.where(np.arange(m) % 3 == 1, 1.4, 0.6))
    c.old_logp = c.old_logp.copy()
    c.old_logp[c.gather] = (lp - np.log(tgt[src])).astype(np.float32)
    assert C.branch_margin(c) >= 1e-2
    return c, feat, W, b


def _head_grads(c, feat, W, b, dtype, device, fused, grad_output=None):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
    lin = torch.nn.Linear(W.shape[1], W.shape[0]).to(device=device, dtype=dtype)
    with torch.no_grad():
        lin.weight.copy_(t(W))
        lin.bias.copy_(t(b))
    ls_par = torch.nn.Parameter(t(c.log_std)) if c.cont else None   # [1, A], as the default net
    o = lin(t(feat))
    lg, v = o[:, :c.A], o[:, c.A]          # non-contiguous views of the head's output
    ls = torch.broadcast_to(ls_par, lg.shape) if c.cont else None
    acts = torch.from_numpy(c.actions).to(device)
    if c.cont:
        acts = acts.to(dtype)
    kw = dict(actions=acts, old_log_probs=t(c.old_logp), advantages=t(c.adv), returns=t(c.ret),
              idx=torch.from_numpy(c.gather).to(device), clip=c.eps, value_loss_weight=c.cv,
              entropy_beta=c.beta, scale=c.scale, continuous=c.cont)
    if fused:
        loss, parts = engine.fused_ppo_loss(lg, v, ls, **kw)
        assert parts.shape == (5,) and not parts.requires_grad and parts.is_cuda
    else:
        loss, parts = engine._torch_ppo_loss(lg, v, ls, kw["actions"], kw["old_log_probs"],
                                             kw["advantages"], kw["returns"], kw["idx"], c.eps,
                                             c.cv, c.beta, c.scale, c.cont)
    if grad_output is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(grad_output, dtype=loss.dtype, device=loss.device))
    g = {"weight": lin.weight.grad, "bias": lin.bias.grad}
    if c.cont:
        g["log_std"] = ls_par.grad
    return (loss.detach().double().cpu().numpy(), parts.double().cpu().numpy(),
            {k: x.double().cpu().numpy() for k, x in g.items()})


@pytest.mark.parametrize("cont", [False, True])
def test_autograd_function_through_a_linear_head(cont):
    c, feat, W, b = _head_case(cont)
    parts_y, _ = C.torch_loss(c, torch.float64)
    loss64, _, g64 = _head_grads(c, feat, W, b, torch.float64, "cpu", fused=False)
    _, _, g32 = _head_grads(c, feat, W, b, torch.float32, "cpu", fused=False)
    loss, parts, g = _head_grads(c, feat, W, b, torch.float32, dev(), fused=True)
    np.testing.assert_allclose(loss, loss64, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(parts, parts_y, rtol=1e-5, atol=1e-5)
    assert loss == np.float64(np.float32(parts[0]))
    for k in g64:
        bound, scale = C.grad_bound(g64[k], g32[k])
        err = np.abs(g[k] - g64[k]).max()
        print(k, "err", err / scale, "bound", bound / scale)
        assert err <= bound, (k, err / scale, bound / scale)
    _, _, gq = _head_grads(c, feat, W, b, torch.float32, dev(), fused=True, grad_output=0.25)
    for k in g:
        np.testing.assert_allclose(gq[k], 0.25 * g[k], rtol=1e-6,
                                   atol=1e-7 * np.abs(g[k]).max())


def _restated(c, lg, v, ls, acts, idx, dt, t):
    """Today's text of the generic learn's loss, on the device."""
    a_mb = acts[idx]
    if c.cont:
        from diamond.continuous_ppo import JointNormal
        dist = JointNormal(loc=lg, scale=ls.exp())
    else:
        dist = torch.distributions.Categorical(logits=lg)
        a_mb = a_mb.long()
    lp = dist.log_prob(a_mb)
    ratio = (lp - t(c.old_logp, dt)[idx]).exp()
    a = t(c.adv, dt)[idx]
    l_pi = torch.max(-a * ratio, -a * torch.clamp(ratio, 1.0 - c.eps, 1.0 + c.eps)).mean()
    l_v = 0.5 * torch.nn.functional.mse_loss(v, t(c.ret, dt)[idx])
    loss = (l_pi + c.cv * l_v + -c.beta * dist.entropy().mean()) * 0.5
    return loss, lp.detach()


@pytest.mark.parametrize("cont", [False, True])
def test_fallbacks_equal_the_torch_expression_exactly(cont):
    """cap + 1 actions, float64 inputs and m == 0 take today's torch ops: the same bits as the
    restated expression on the same device -- or, where torch refuses the input (Categorical
    of an empty batch), the same exception."""
    t = lambda a, dt=torch.float32: torch.from_numpy(np.array(a)).to(dev(), dt)

    def one(c, dt, m, fused):
        lg = t(c.logits, dt)[:m].requires_grad_(True)
        v = t(c.values, dt)[:m].requires_grad_(True)
        ls = t(np.broadcast_to(c.log_std, c.logits.shape), dt)[:m].requires_grad_(True) \
            if c.cont else None
        acts = t(c.actions, dt) if c.cont else torch.from_numpy(c.actions).to(dev())
        idx = torch.from_numpy(c.gather).to(dev())[:m]
        try:
            if fused:
                loss, parts = engine.fused_ppo_loss(
                    lg, v, ls, actions=acts, old_log_probs=t(c.old_logp, dt),
                    advantages=t(c.adv, dt), returns=t(c.ret, dt), idx=idx, clip=c.eps,
                    value_loss_weight=c.cv, entropy_beta=c.beta, scale=0.5, continuous=c.cont)
                assert parts.shape == (5,) and not parts.requires_grad
                lp = engine.policy_log_probs(lg.detach(), ls.detach() if c.cont else None,
                                             actions=acts, idx=idx, continuous=c.cont)
            else:
                loss, lp = _restated(c, lg, v, ls, acts, idx, dt, t)
            if lg.shape[0]:
                loss.backward()
        except (RuntimeError, ValueError) as e:
            return type(e)
        return [x.detach().cpu().numpy() for x in
                (loss, lp, lg.grad if lg.grad is not None else lg.detach() * 0,
                 v.grad if v.grad is not None else v.detach() * 0)]

    def both(c, dt, m=None):
        got, want = one(c, dt, m, True), one(c, dt, m, False)
        if isinstance(want, type):
            assert got is want
            return
        for a, b_ in zip(got, want):
            assert a.dtype == b_.dtype and a.tobytes() == b_.tobytes()

    both(C.make_case(m=33, A=CAP + 1, cont=cont, seed=41), torch.float32)   # A above the cap
    small = C.make_case(m=33, A=4, cont=cont, seed=42)
    both(small, torch.float64)                               # a dtype other than float32
    both(small, torch.float32, m=0)                          # an empty minibatch
