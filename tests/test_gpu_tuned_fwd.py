"""GPU checks of the tuned class's two forward kernels (csrc/mlp.hip eval_kernel and act_kernel)
over shapes, sizes and alignments, against the float64 oracle.

A. heads: dppo_actor_forward_f32 against P.forward in float64, per element within
   2e-5 max(1, |f64|) + 4 |oracle32 - f64| (gpu_helpers._within, the near rule of
   tests/test_gpu_regimes.py); also at every first-layer width D = 1 .. 32.
B. dppo_old_policy_f32 called directly (no rollout, no reuse): log-probs, values and next values
   against the float64 restatement of tuned_fwd_cases.oracle_eval, with the bound of A.
C. draws: dppo_act_f32's categorical draws against the inverse CDF of the float64 softmax on the
   samples farther than 1e-4 from every CDF boundary (at most max(1, ceil(n / 100)) samples are
   not: tests/test_tuned_fwd_cpu.py), its Gaussian draws against oracle_gaussian_draws at
   rtol = atol = 1e-4; dppo_act_squash_f32 returns the same u bit for bit and the squashed actions
   of tests/test_gpu_wide_act.py's bounds; the same call twice gives the same bits, counter + 1
   other draws.
D. alignment: B and C again with obs (and next_obs) 4 bytes past a 16-byte boundary -- the
   per-feature loads of a D that is a multiple of 4 -- equal to the aligned run bit for bit.
E. guards, in every call of A to D and H: every output buffer is prefilled with one NaN bit pattern
   and has 64 guard elements on either side of the part the kernel owns (afterwards the owned part
   is finite and the guards hold the pattern), every input buffer lies in a NaN-filled allocation
   with at least 32 NaN floats before row 0 and after row n - 1 (a feature or an action read past
   a row's end or a row >= n that reaches a stored result makes it NaN).
F. n = 0: DPPO_OK, outputs untouched.
G. the reuse path of dppo_prepare_f32 (the LDS ring, the pooled remainder, the next_values[ip] = v
   shortcut) on chained rollouts: log-probs, values, next values with the bound of A, returns ==
   values + gae(values) bit for bit, advantages within 2e-6; the same bits with obs at a 4-byte
   offset.
H. three wide shapes through B at sizes off a multiple of 32 (csrc/mbwide.hip wide_eval_kernel sits
   behind the same entry point).

Shapes, sizes and seeds: tests/tuned_fwd_cases.py.  Measured figures: DESIGN.md §4.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from diamond import _native as N
from oracle import ppo_np as P

import tuned_fwd_cases as C
from gpu_helpers import _within, dev, hparams, stream
from test_gpu_rollout_ckpt import oracle_gaussian_draws, philox4x32_10, u01
from wide_act_cases import categorical_oracle

NAN_BITS = 0x7FC0DEAD  # a quiet NaN with a payload no arithmetic produces
GUARD = 64             # guard elements on either side of an output
PAD = 32               # NaN floats before and after an input (128 bytes: keeps 16-byte alignment)
_KEYS = ("log_probs", "values", "next_values", "advantages", "returns")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _params(cases):
    return [pytest.param(c, id=C.case_id(c)) for c in cases]


def _resolve(case):
    """The case with its size spelled out (BIG needs the device's CU count)."""
    return (*case[:4], C.real_n(case[4], _cus()))


@functools.lru_cache(maxsize=None)
def _case(Hd, D, A, cont, n):
    """One case's inputs and oracles, computed once and shared (read-only) by the tests."""
    params, flat, obs, nobs, act = C.inputs(Hd, D, A, cont, n)
    ref = C.oracle_eval(params, obs, act, nobs, cont)
    for a in (flat, obs, nobs, act, *(x for pair in ref.values() for x in pair)):
        a.setflags(write=False)
    return params, flat, obs, nobs, act, ref


@functools.lru_cache(maxsize=None)
def _handle(Hd, D, A, cont):
    return N.Handle(0, C.dims(Hd, D, A, cont))


# ---- E: guarded buffers -----------------------------------------------------------------------
class _In:
    """A host array on the device inside a NaN-filled allocation: PAD + offset NaN floats before
    its first element, PAD after its last."""

    def __init__(self, x, offset=0):
        raw = np.ascontiguousarray(x).ravel().view(np.uint8)  # (the done flags are bytes)
        pre = 4 * (PAD + offset)
        host = np.full((pre + raw.size + 3) // 4 + PAD, NAN_BITS, np.uint32).view(np.uint8)
        host[pre:pre + raw.size] = raw
        self.buf = torch.from_numpy(host).to(dev())
        self.ptr = self.buf.data_ptr() + pre
        assert self.ptr % 16 == 4 * offset  # the alignment the case asks for


class _Out:
    """count elements the kernel owns between two guards, all prefilled with NAN_BITS."""

    def __init__(self, count, dtype=np.float32):
        self.count, self.dtype = count, dtype
        self.buf = torch.full((GUARD + count + GUARD,), NAN_BITS, dtype=torch.int32, device=dev())
        self.ptr = self.buf.data_ptr() + 4 * GUARD

    def bits(self):
        return self.buf.cpu().numpy().view(np.uint32)

    def untouched(self):
        return bool((self.bits() == NAN_BITS).all())

    def get(self, what):
        """The owned part, after checking it and the guards."""
        raw = self.bits()
        assert (raw[:GUARD] == NAN_BITS).all(), f"{what}: the guard before the output was written"
        assert (raw[GUARD + self.count:] == NAN_BITS).all(), \
            f"{what}: the guard after the output was written"
        own = raw[GUARD:GUARD + self.count].view(self.dtype).copy()
        if self.dtype == np.float32:
            assert np.isfinite(own).all(), f"{what}: {int((~np.isfinite(own)).sum())} not finite"
        else:
            assert (own.view(np.uint32) != NAN_BITS).all(), f"{what}: elements left unwritten"
        return own


# ---- the calls ---------------------------------------------------------------------------------
def _run_heads(case, offset=0):
    Hd, D, A, cont, n = case
    _, flat, obs, *_ = _case(*case)
    h, pd, od, out = _handle(Hd, D, A, cont), _In(flat), _In(obs, offset), _Out(n * A)
    rc = h.lib.dppo_actor_forward_f32(h.h, pd.ptr, od.ptr, n, out.ptr, stream())
    torch.cuda.synchronize()
    N.check(rc)
    return out.get("heads").reshape(n, A)


def _run_eval(case, offset=0):
    Hd, D, A, cont, n = case
    _, flat, obs, nobs, act, _ = _case(*case)
    h, pd = _handle(Hd, D, A, cont), _In(flat)
    od, nd, ad = _In(obs, offset), _In(nobs, offset), _In(act)
    outs = {k: _Out(n) for k in _KEYS[:3]}
    rc = h.lib.dppo_old_policy_f32(h.h, pd.ptr, od.ptr, ad.ptr, nd.ptr, outs["log_probs"].ptr,
                                   outs["values"].ptr, outs["next_values"].ptr, n, stream())
    torch.cuda.synchronize()
    N.check(rc)
    return {k: o.get(k) for k, o in outs.items()}


def _run_act(case, counter, offset=0):
    Hd, D, A, cont, n = case
    _, flat, obs, *_ = _case(*case)
    h, pd, od = _handle(Hd, D, A, cont), _In(flat), _In(obs, offset)
    out = _Out(n * A) if cont else _Out(n, np.int32)
    rc = h.lib.dppo_act_f32(h.h, pd.ptr, od.ptr, n, C.SEED, counter, out.ptr, stream())
    torch.cuda.synchronize()
    N.check(rc)
    got = out.get("actions")
    return got.reshape(n, A) if cont else got


def _run_act_squash(case, counter, lo, hi, offset=0):
    Hd, D, A, cont, n = case
    _, flat, obs, *_ = _case(*case)
    h, pd, od = _handle(Hd, D, A, cont), _In(flat), _In(obs, offset)
    u, env = _Out(n * A), _Out(n * A)
    rc = h.lib.dppo_act_squash_f32(h.h, pd.ptr, od.ptr, n, C.SEED, counter,
                                   None if lo is None else lo.ctypes.data,
                                   None if hi is None else hi.ctypes.data, u.ptr, env.ptr, stream())
    torch.cuda.synchronize()
    N.check(rc)
    return u.get("u").reshape(n, A), env.get("env actions").reshape(n, A)


# ---- the comparisons ---------------------------------------------------------------------------
def _check_heads(case, got):
    x64, x32 = _case(*case)[5]["heads"]
    d, d32 = _within(got, x64, x32, "heads")
    print(f"TUNED heads {C.case_id(case)}: max |kernel - f64| {d:.3g}, |oracle32 - f64| {d32:.3g}")


def _check_eval(case, got, tag="eval"):
    ref = _case(*case)[5]
    figs = {k: _within(got[k], *ref[k], k) for k in _KEYS[:3]}
    print(f"TUNED {tag} {C.case_id(case)}: max |kernel - f64| / |oracle32 - f64| " + " ".join(
        f"{k} {a:.3g} / {b:.3g}" for k, (a, b) in figs.items()))


def _bounds(A):
    return (np.linspace(-2.0, -0.25, A).astype(np.float32),
            np.linspace(0.5, 3.0, A).astype(np.float32))


def _check_draws(case, offset=0):
    """C on one case; returns what the calls gave, for D's comparison of bits."""
    Hd, D, A, cont, n = case
    params, *_, ref = _case(*case)
    out64 = ref["heads"][0]
    got = _run_act(case, C.COUNTER, offset)
    assert np.array_equal(got.view(np.uint32),
                          _run_act(case, C.COUNTER, offset).view(np.uint32))  # the same call twice
    # (a single categorical draw may well repeat under another counter; from n = 31 up the oracle's
    # own draws differ, tests/test_tuned_fwd_cpu.py)
    if cont or n >= 31:
        assert not np.array_equal(got, _run_act(case, C.COUNTER + 1, offset))
    if not cont:
        want, clear = categorical_oracle(out64, C.SEED, C.COUNTER, philox4x32_10, u01)
        unclear = int((~clear).sum())
        print(f"TUNED draws {C.case_id(case)}: {unclear} of {n} samples unclear "
              f"(share {unclear / n:.4f}), equal on clear {np.mean(got[clear] == want[clear]):.4f}")
        assert unclear <= C.max_unclear(n), (unclear, n)
        assert got.min() >= 0 and got.max() < A
        assert np.array_equal(got[clear], want[clear])
        return (got,)
    want = oracle_gaussian_draws(out64, params["actor_log_std"], C.SEED, C.COUNTER)
    print(f"TUNED draws {C.case_id(case)}: max |u - oracle| {np.abs(got - want).max():.3g}")
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4)
    lo, hi = _bounds(A)
    envs = []
    for bounded in (False, True):
        u2, env = _run_act_squash(case, C.COUNTER, lo if bounded else None,
                                  hi if bounded else None, offset)
        assert np.array_equal(u2.view(np.uint32), got.view(np.uint32))  # the plain call's draws
        if bounded:
            env_own = P.squash_action(u2, lo.astype(np.float64), hi.astype(np.float64))
            assert np.all(env >= lo) and np.all(env <= hi)
            atol = float(4e-7 * (1 + np.abs(lo).max()))
        else:
            env_own = np.tanh(u2.astype(np.float64))
            assert np.all(np.abs(env) <= 1.0)
            atol = 4e-7
        print(f"  bounded={bounded}: max |env - squash(u)| {np.abs(env - env_own).max():.3g}")
        np.testing.assert_allclose(env, env_own, rtol=0, atol=atol)
        envs.append(env)
    return (got, *envs)


# ---- A: heads ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _params(C.cases()))
def test_tuned_actor_heads_vs_float64(case):
    case = _resolve(case)
    _check_heads(case, _run_heads(case))


@pytest.mark.parametrize("case", _params(C.sweep_cases()))
def test_tuned_actor_heads_at_every_obs_dim(case):
    _check_heads(case, _run_heads(case))


# ---- B: dppo_old_policy_f32 -------------------------------------------------------------------
@pytest.mark.parametrize("case", _params(C.cases()))
def test_tuned_old_policy_direct_vs_float64(case):
    case = _resolve(case)
    _check_eval(case, _run_eval(case))


# ---- C: draws ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", _params(C.cases()))
def test_tuned_draws_are_the_documented_philox_stream(case):
    _check_draws(_resolve(case))


# ---- D: alignment -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", _params(C.align_cases()))
def test_tuned_forward_with_obs_at_a_4_byte_offset(case):
    """(_In asserts the offset from the 16-byte boundary.)"""
    aligned, shifted = _run_eval(case), _run_eval(case, offset=1)
    _check_eval(case, shifted, "eval at +4 B")
    for k in aligned:
        assert np.array_equal(aligned[k].view(np.uint32), shifted[k].view(np.uint32)), k
    heads = _run_heads(case, offset=1)
    _check_heads(case, heads)
    assert np.array_equal(_run_heads(case).view(np.uint32), heads.view(np.uint32))
    for a, b in zip(_check_draws(case), _check_draws(case, offset=1)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- F: n = 0 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(C.H, 8, 4, False), (C.H, 17, 6, True)],
                         ids=lambda s: C.case_id((*s, 0)))
def test_tuned_forward_of_no_samples_writes_nothing(shape):
    Hd, D, A, cont = shape
    _, flat, obs, nobs, act, _ = _case(*shape, 33)
    h, pd, od, nd, ad = _handle(*shape), _In(flat), _In(obs), _In(nobs), _In(act)
    outs = [_Out(33 * A) for _ in range(3)]
    assert h.lib.dppo_old_policy_f32(h.h, pd.ptr, od.ptr, ad.ptr, nd.ptr, outs[0].ptr,
                                     outs[1].ptr, outs[2].ptr, 0, stream()) == N.DPPO_OK
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)
    assert h.lib.dppo_act_f32(h.h, pd.ptr, od.ptr, 0, C.SEED, C.COUNTER, outs[0].ptr,
                              stream()) == N.DPPO_OK
    assert h.lib.dppo_actor_forward_f32(h.h, pd.ptr, od.ptr, 0, outs[1].ptr,
                                        stream()) == N.DPPO_OK
    torch.cuda.synchronize()
    assert all(o.untouched() for o in outs)


# ---- G: the reuse path ------------------------------------------------------------------------
def _prepare(h, flat, host, offset):
    B = host[3].size
    ins = [_In(host[0], offset), _In(host[1], offset)] + [_In(x) for x in host[2:]]
    pd = _In(flat)
    outs = {k: _Out(B) for k in _KEYS}
    ro = N.Rollout(*[x.ptr for x in ins])
    lo = N.LearnOutputs(*[outs[k].ptr for k in _KEYS])
    hp = hparams()
    rc = h.lib.dppo_prepare_f32(h.h, ctypes.byref(ro), pd.ptr, ctypes.byref(hp), ctypes.byref(lo),
                                stream())
    torch.cuda.synchronize()
    N.check(rc)
    return {k: o.get(k) for k, o in outs.items()}


@pytest.mark.parametrize("case", C.REUSE_CASES, ids=C.reuse_id)
def test_tuned_reuse_path_on_chained_rollouts_vs_float64(case):
    T, Nn, D, A, cont = case
    params, flat, host, _ = C.chained_rollout(*case)
    obs, nobs, act, rew, te, tr = host
    h = N.Handle(0, N.Dims(T, Nn, D, A, int(cont), C.H, 1, 1, 1, 0))
    assert h.fused_plan(T * Nn)["shape_class"] == "tuned"
    o = _prepare(h, flat, host, 0)
    ref = C.oracle_eval(params, obs, act, nobs, cont)
    figs = {k: _within(o[k], ref[k][0].ravel(), ref[k][1].ravel(), k) for k in _KEYS[:3]}
    print(f"TUNED reuse {C.reuse_id(case)}: max |kernel - f64| / |oracle32 - f64| " + " ".join(
        f"{k} {a:.3g} / {b:.3g}" for k, (a, b) in figs.items()))
    vals, nvals = o["values"].reshape(T, Nn), o["next_values"].reshape(T, Nn)
    raw = P.gae(rew, te, tr, vals, nvals)
    assert np.array_equal(o["returns"].reshape(T, Nn), vals + raw)
    np.testing.assert_allclose(o["advantages"], P.normalize_adv(raw).ravel(), rtol=0, atol=2e-6)
    shifted = _prepare(h, flat, host, 1)
    for k in _KEYS:
        assert np.array_equal(o[k].view(np.uint32), shifted[k].view(np.uint32)), k
    h.close()


# ---- H: wide shapes through dppo_old_policy_f32 -----------------------------------------------
@pytest.mark.parametrize("case", _params(C.wide_cases()))
def test_wide_old_policy_direct_at_ragged_sizes_vs_float64(case):
    Hd, D, A, cont, n = case
    assert _handle(Hd, D, A, cont).fused_plan(n)["shape_class"] == "wide"
    _check_eval(case, _run_eval(case), "wide eval")
