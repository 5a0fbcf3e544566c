"""The opt-in GRU scan path without a GPU: the host-only plan of the scan kernels
(dppo_gru_scan_plan), the flags' defaults, and the fallback -- on a CPU module, a float64 module
and a hidden size outside 16 / 32 / 64, ``GRUCore.forward`` with ``fused_scan`` set returns exactly
what it returns with it unset, and no kernel call is counted."""
import ctypes

import pytest
import torch

import diamond
from diamond import _native as N
from diamond import recurrent_ppo as R
from diamond.recurrent_ppo import GRUCore


@pytest.mark.parametrize("G,envs", [(16, 16), (32, 8), (64, 4)])
def test_plan_geometry_and_sizes(G, envs):
    for T, Nn in ((1, 1), (7, envs - 1), (7, envs), (7, envs + 1), (7, 2 * envs + 1), (32, 8192),
                  (3, 2 ** 31)):
        got = N.gru_scan_plan(G, T, Nn)
        assert got == (envs, -(-Nn // envs), T * Nn * 4 * G, T * Nn * 3 * G, T * Nn * 3 * G)


def test_plan_output_may_be_null():
    assert N.load().dppo_gru_scan_plan(16, 1, 1, None) == N.DPPO_OK


@pytest.mark.parametrize("G", [0, 8, 17, 48, 128])
def test_plan_refuses_other_widths(G):
    out = (ctypes.c_int64 * 5)(*([-7] * 5))
    assert N.load().dppo_gru_scan_plan(G, 4, 4, out) != N.DPPO_OK
    assert list(out) == [-7] * 5
    with pytest.raises(Exception):
        N.gru_scan_plan(G, 4, 4)


@pytest.mark.parametrize("T,Nn", [(0, 4), (4, 0), (-1, 4), (4, -1), (0, 0)])
def test_plan_refuses_empty_sequences(T, Nn):
    for G in (16, 32, 64):
        assert N.load().dppo_gru_scan_plan(G, T, Nn, None) == N.DPPO_EINVAL


def test_scan_entry_points_are_exported():
    lib = N.load()
    for name in ("dppo_gru_scan_plan", "dppo_gru_scan_fwd_f32", "dppo_gru_scan_bwd_f32"):
        assert name in N.EXPORTED and hasattr(lib, name)


def test_flags_default_off():
    assert GRUCore(8, 16).fused_scan is False
    assert diamond.RecurrentPPO.fused_core is False
    assert isinstance(R.CORE_SCAN_CALLS[0], int)


def test_rollout_case_has_wide_action_margins():
    """The peaked rollout case of tests/test_gpu_gru_core_learn.py: in the float64 CPU module every
    sample's arg-max action leads by PEAK_MARGIN (far above the 1e-3 the comparison of actions
    needs), so sampling returns it whatever the generator draws."""
    import gru_core_cases as C
    cfg = C.config(C.ROLLOUT_SHAPE, rollout_steps=C.ROLLOUT_T)
    net = C.initial_network(C.ROLLOUT_SHAPE, cfg)
    plain, _ = C.replica_logits(net, C.ROLLOUT_SHAPE)
    C.peak_(net)
    peaked, hxs = C.replica_logits(net, C.ROLLOUT_SHAPE)
    assert C.action_margins(peaked).min() >= C.PEAK_MARGIN > 1e-3
    assert torch.equal(peaked.argmax(-1), plain.argmax(-1))
    assert peaked.shape == (C.ROLLOUT_T, C.NENVS, C.ROLLOUT_SHAPE[3])
    assert len(set(peaked.argmax(-1).reshape(-1).tolist())) > 1


def _inputs(I, G, dtype, T=5, Nn=3):
    g = torch.Generator().manual_seed(I * 100 + G)
    x = torch.randn(T, Nn, I, generator=g, dtype=dtype)
    hx = torch.randn(1, Nn, G, generator=g, dtype=dtype) * 0.5
    dones = torch.rand(T, Nn, generator=g) < 0.3
    return x, hx, dones


def _both(core, x, hx, dones):
    """(out, hx, gradients) of one forward + backward with fused_scan unset and set."""
    res = []
    for flag in (False, True):
        core.fused_scan = flag
        core.zero_grad()
        xi = x.clone().requires_grad_(True)
        out, h = core(xi, hx, dones)
        (out.sum() + 2.0 * h.sum()).backward()
        res.append([out.detach(), h.detach(), xi.grad] + [p.grad.clone()
                                                           for p in core.parameters()])
    return res


@pytest.mark.parametrize("case", ["cpu-f32-16", "cpu-f32-64", "cpu-f64-32", "cpu-f32-48"])
def test_fallback_is_the_step_loop(case):
    _, dt, G = case.split("-")
    dtype, G = {"f32": torch.float32, "f64": torch.float64}[dt], int(G)
    torch.manual_seed(3)
    core = GRUCore(6, G).to(dtype)
    x, hx, dones = _inputs(6, G, dtype)
    calls0 = R.CORE_SCAN_CALLS[0]
    for args in ((x, hx, dones), (x, None, None), (x, hx, None), (x, None, dones)):
        off, on = _both(core, *args)
        for a, b in zip(off, on):
            assert torch.equal(a, b)
        with torch.no_grad():
            core.fused_scan = True
            assert torch.equal(core(*args)[0], off[0])
    assert R.CORE_SCAN_CALLS[0] == calls0      # no kernel served any of these forwards
