"""GRUCore on the GRU scan kernels (``fused_scan``, csrc/gruseq.hip) against GRUCore itself, flag
off, in float64 on the CPU under autograd -- the existing module, the project's intended semantics
of recurrent_ppo.py:41-91.

Compared per case: ``out``, the final ``hx``, and the gradients of one fixed random linear
functional of both with respect to x, hx, weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0.

* Bound, per tensor: max|diff| <= 2e-5 * max|ref| (tests/test_gpu_gru.py's, which the same
  recurrence arithmetic meets in grugrad.hip at these three widths).
* 4x rule, per tensor (tests/test_gpu_production.py's): the fused result is no further from float64
  than 4x the float32 flag-off module's own distance on the same inputs and device, + 1e-6 *
  max|ref|.
* A reference tensor that is identically zero must come back exactly zero.
* The saturated case (weight_hh x 8): where it misses the 2e-5 bound and the float32 step loop
  misses it too, it stands under the 4x rule alone.

Measured on an MI355X, largest max|diff| / max|ref| over the tensors of every case but the
saturated one, scan / float32 step loop: 4.7e-7 / 4.7e-7 at G = 16, 4.4e-7 / 5.0e-7 at 32,
5.8e-7 / 5.3e-7 at 64; the saturated case 7.6e-7 / 1.1e-6, 9.3e-7 / 1.4e-6, 7.6e-7 / 5.5e-7: it
meets the 2e-5 bound on both paths, so its exemption does not come into play.

Then the C ABI called directly: every output between NaN guard regions that must stay untouched, a
repeat call bit-identical, a NULL ``saved`` the same ``out`` bits, and refusals without a launch.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from diamond import _native as N
from diamond import recurrent_ppo as R
from diamond.recurrent_ppo import GRUCore

WIDTHS = (16, 32, 64)
PATTERNS = ("none", "first", "env_always", "last", "random")


def _cases(G):
    """name -> (T, N, input width, dones pattern or None, hx given, weight_hh scale)"""
    E = 256 // G
    c = {"T1": (1, 3, 8, "random", True, 1.0),
         "T40": (40, 5, 8, "random", True, 1.0),
         "wide-input": (7, E + 1, 128, "random", True, 1.0),
         "no-hx-no-dones": (7, E + 1, 8, None, False, 1.0),
         "no-hx": (7, 3, 8, "random", False, 1.0),
         # the one env is done at every step: dWhh and dhx are identically zero
         "always-done": (7, 1, 8, "env_always", True, 1.0),
         "saturated": (7, E + 1, 8, "random", True, 8.0)}
    for n in (1, E - 1, E, E + 1, 2 * E + 1):
        c[f"N{n}"] = (7, n, 8, "random", True, 1.0)
    for p in PATTERNS:
        c[f"dones-{p}"] = (7, E + 1, 8, p, True, 1.0)
    return c


ALL = [(G, name) for G in WIDTHS for name in _cases(G)]
GRAD_NAMES = ("x", "hx", "weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def _dones(pattern, T, Nn, g):
    d = torch.zeros(T, Nn, dtype=torch.bool)
    if pattern == "first":
        d[0] = True
    elif pattern == "env_always":
        d[:, 0] = True
    elif pattern == "last":
        d[T - 1] = True
    elif pattern == "random":
        d = torch.rand(T, Nn, generator=g) < 0.3
    return d


@functools.lru_cache(maxsize=None)
def _inputs(G, name):
    T, Nn, I, pattern, with_hx, whh = _cases(G)[name]
    g = torch.Generator().manual_seed(1000 * G + 7 * T + Nn + I)
    torch.manual_seed(G + I)
    core = GRUCore(I, G).double()
    with torch.no_grad():
        core.weight_hh_l0.mul_(whh)
    x = torch.randn(T, Nn, I, generator=g, dtype=torch.float64)
    hx = torch.randn(1, Nn, G, generator=g, dtype=torch.float64) * 0.5 if with_hx else None
    dones = _dones(pattern, T, Nn, g) if pattern is not None else None
    w_out = torch.randn(T, Nn, G, generator=g, dtype=torch.float64)
    w_h = torch.randn(1, Nn, G, generator=g, dtype=torch.float64)
    return core, x, hx, dones, w_out, w_h


def _evaluate(G, name, dtype, device, fused):
    """out, final hx and the functional's gradients, as float64 CPU tensors."""
    core64, x, hx, dones, w_out, w_h = _inputs(G, name)
    core = GRUCore(core64.input_size, G).to(dtype)
    core.load_state_dict(core64.state_dict())
    core = core.to(device)
    core.fused_scan = fused
    to = lambda t: None if t is None else t.detach().clone().to(device=device, dtype=dtype)
    xi = to(x).requires_grad_(True)
    hi = to(hx).requires_grad_(True) if hx is not None else None
    di = dones.to(device) if dones is not None else None
    calls0 = R.CORE_SCAN_CALLS[0]
    out, h = core(xi, hi, di)
    assert R.CORE_SCAN_CALLS[0] - calls0 == (1 if fused else 0)
    assert out.shape == x.shape[:2] + (G,) and h.shape == (1, x.shape[1], G)
    ((out * to(w_out)).sum() + (h * to(w_h)).sum()).backward()
    res = {"out": out, "hx_final": h, "x": xi.grad, "hx": hi.grad if hi is not None else None}
    for n in GRAD_NAMES[2:]:
        res[n] = getattr(core, n).grad
    return {k: v.detach().double().cpu() for k, v in res.items() if v is not None}


@functools.lru_cache(maxsize=None)
def _reference(G, name):
    return _evaluate(G, name, torch.float64, "cpu", False)


@pytest.mark.parametrize("G,name", ALL, ids=[f"G{G}-{n}" for G, n in ALL])
def test_scan_matches_float64_module(G, name):
    ref = _reference(G, name)
    loop32 = _evaluate(G, name, torch.float32, "cuda", False)
    fused = _evaluate(G, name, torch.float32, "cuda", True)
    assert set(fused) == set(ref) == set(loop32)
    if name == "always-done":
        assert not ref["weight_hh_l0"].any() and not ref["hx"].any()
    if name == "dones-first":
        assert not ref["hx"].any()
    for k, r in ref.items():
        s = float(r.abs().max())
        if s == 0.0:
            assert not fused[k].any(), (k, float(fused[k].abs().max()))
            continue
        d_f = float((fused[k] - r).abs().max()) / s
        d_l = float((loop32[k] - r).abs().max()) / s
        print(f"G{G} {name} {k}: fused {d_f:.2e}, float32 loop {d_l:.2e} (of max|ref| {s:.2e})")
        assert torch.isfinite(fused[k]).all(), k
        if not (name == "saturated" and d_l > 2e-5):
            assert d_f <= 2e-5, (k, d_f, d_l)
        assert d_f <= 4 * d_l + 1e-6, (k, d_f, d_l)


class _Recorder:
    """libdppo with the scan forward's arguments recorded."""

    def __init__(self, lib):
        self._lib, self.fwd_args = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "dppo_gru_scan_fwd_f32":
            return fn

        def wrapped(*args):
            self.fwd_args.append(args)
            return fn(*args)
        return wrapped


@pytest.mark.parametrize("G", WIDTHS)
def test_inference_saves_nothing_and_gives_the_same_bits(G, monkeypatch):
    core64, x, hx, dones, _, _ = _inputs(G, f"N{256 // G + 1}")
    core = GRUCore(core64.input_size, G)
    core.load_state_dict(core64.state_dict())
    core = core.cuda()
    core.fused_scan = True
    rec = _Recorder(N.load())
    monkeypatch.setattr(N, "load", lambda: rec)
    xc, hc, dc = x.float().cuda(), hx.float().cuda(), dones.cuda()
    out, h = core(xc, hc, dc)
    assert out.requires_grad and rec.fwd_args[-1][6] is not None      # saved
    with torch.no_grad():
        out_ng, h_ng = core(xc, hc, dc)
    assert rec.fwd_args[-1][6] is None
    with torch.inference_mode():
        out_im, h_im = core(xc, hc, dc)
    assert rec.fwd_args[-1][6] is None
    for a, b in ((out_ng, h_ng), (out_im, h_im)):
        assert torch.equal(a, out) and torch.equal(b, h) and not a.requires_grad
    assert torch.equal(h, out[-1:])
    # non-contiguous operands are made contiguous: the same bits
    x_nc = xc.transpose(0, 1).contiguous().transpose(0, 1)
    d_nc = dc.t().contiguous().t()
    h_nc = hc.repeat_interleave(2, dim=2)[:, :, ::2]
    assert not x_nc.is_contiguous() and not d_nc.is_contiguous() and not h_nc.is_contiguous()
    out_nc, _ = core(x_nc, h_nc, d_nc)
    assert torch.equal(out_nc, out)
    # dones of another dtype keep their meaning: non-zero = done
    out_f, _ = core(xc, hc, dc.to(torch.float32) * 3.0)
    assert torch.equal(out_f, out)


def test_other_inputs_fall_back_on_the_gpu():
    """float64 on the GPU and a hidden size of 48 run the step loop: no kernel call."""
    torch.manual_seed(0)
    for I, G, dt in ((8, 32, torch.float64), (8, 48, torch.float32)):
        core = GRUCore(I, G).to(dt).cuda()
        x = torch.randn(4, 3, I, dtype=dt, device="cuda")
        core.fused_scan = False
        want = core(x)[0]
        core.fused_scan = True
        calls0 = R.CORE_SCAN_CALLS[0]
        assert torch.equal(core(x)[0], want)
        assert R.CORE_SCAN_CALLS[0] == calls0


# ---- the C ABI, called directly

GUARD = 64  # floats on either side of every output


class _Guarded:
    """``n`` floats between two NaN guard regions; the payload starts 16-byte aligned and is
    itself filled with NaN, so an element the kernel skipped shows."""

    def __init__(self, n):
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), device="cuda")
        self.n = n

    @property
    def payload(self):
        return self.buf[GUARD:GUARD + self.n]

    def ptr(self):
        return self.payload.data_ptr()

    def check(self, what):
        assert torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[GUARD + self.n:]).all(), what
        assert not torch.isnan(self.payload).any(), what


def _abi_operands(G, T, Nn, seed=0):
    g = torch.Generator().manual_seed(seed + G)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    return dict(gi=r(T, Nn, 3 * G), hx0=r(Nn, G) * 0.5, whh=r(3 * G, G) / G ** 0.5, bhh=r(3 * G),
                dones=(torch.rand(T, Nn, generator=g) < 0.3).to(torch.uint8).cuda(),
                dout=r(T, Nn, G), dhT=r(Nn, G))


def _fwd(lib, o, out, saved, T, Nn, G, whh=None, dones=True):
    return lib.dppo_gru_scan_fwd_f32(
        o["gi"].data_ptr(), o["hx0"].data_ptr(), o["dones"].data_ptr() if dones else None,
        whh if whh is not None else o["whh"].data_ptr(), o["bhh"].data_ptr(), out, saved, T, Nn,
        G, torch.cuda.current_stream().cuda_stream)


def _bwd(lib, o, saved, out, dgi, dgh, dh0, T, Nn, G, whh=None, dhT=True):
    return lib.dppo_gru_scan_bwd_f32(
        o["dout"].data_ptr(), o["dhT"].data_ptr() if dhT else None, saved, out,
        o["hx0"].data_ptr(), o["dones"].data_ptr(), whh if whh is not None else o["whh"].data_ptr(),
        dgi, dgh, dh0, T, Nn, G, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("G", WIDTHS)
def test_abi_writes_exactly_its_outputs_and_repeats_bit_for_bit(G):
    lib = N.load()
    T, Nn = 5, 2 * (256 // G) + 1        # three workgroups, the last with one env
    envs, grid, n_saved, n_dgi, n_dgh = N.gru_scan_plan(G, T, Nn)
    assert grid == 3
    o = _abi_operands(G, T, Nn)
    runs = []
    for _ in range(2):
        out, saved = _Guarded(T * Nn * G), _Guarded(n_saved)
        dgi, dgh, dh0 = _Guarded(n_dgi), _Guarded(n_dgh), _Guarded(Nn * G)
        assert _fwd(lib, o, out.ptr(), saved.ptr(), T, Nn, G) == N.DPPO_OK
        assert _bwd(lib, o, saved.ptr(), out.ptr(), dgi.ptr(), dgh.ptr(), dh0.ptr(), T, Nn,
                    G) == N.DPPO_OK
        torch.cuda.synchronize()
        for name, b in (("out", out), ("saved", saved), ("dgi", dgi), ("dgh", dgh), ("dh0", dh0)):
            b.check(name)
        runs.append([b.payload.clone() for b in (out, saved, dgi, dgh, dh0)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    # a NULL saved: the same out bits; NULL dones = no reset, NULL dh_T = zeros
    out2 = _Guarded(T * Nn * G)
    assert _fwd(lib, o, out2.ptr(), None, T, Nn, G) == N.DPPO_OK
    torch.cuda.synchronize()
    out2.check("out, saved NULL")
    assert torch.equal(out2.payload, runs[0][0])
    o0 = dict(o, dones=torch.zeros_like(o["dones"]), dhT=torch.zeros_like(o["dhT"]))
    res = []
    for null in (False, True):
        out, saved = _Guarded(T * Nn * G), _Guarded(n_saved)
        dgi, dgh, dh0 = _Guarded(n_dgi), _Guarded(n_dgh), _Guarded(Nn * G)
        assert _fwd(lib, o0, out.ptr(), saved.ptr(), T, Nn, G, dones=not null) == N.DPPO_OK
        assert lib.dppo_gru_scan_bwd_f32(
            o0["dout"].data_ptr(), None if null else o0["dhT"].data_ptr(), saved.ptr(), out.ptr(),
            o0["hx0"].data_ptr(), None if null else o0["dones"].data_ptr(), o0["whh"].data_ptr(),
            dgi.ptr(), dgh.ptr(), dh0.ptr(), T, Nn, G,
            torch.cuda.current_stream().cuda_stream) == N.DPPO_OK
        torch.cuda.synchronize()
        res.append([b.payload.clone() for b in (out, saved, dgi, dgh, dh0)])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_abi_refuses_without_a_launch():
    lib = N.load()
    G, T, Nn = 16, 3, 5
    o = _abi_operands(G, T, Nn)
    n_saved = N.gru_scan_plan(G, T, Nn)[2]
    bufs = [_Guarded(T * Nn * G), _Guarded(n_saved), _Guarded(T * Nn * 3 * G),
            _Guarded(T * Nn * 3 * G), _Guarded(Nn * G)]
    out, saved, dgi, dgh, dh0 = (b.ptr() for b in bufs)
    # Whh off the 16-byte grid (staged with 16-byte loads), and a float array off the 4-byte grid
    w = torch.zeros(3 * G * G + 4, device="cuda")
    w[1:1 + 3 * G * G] = o["whh"].reshape(-1)
    bad_whh = w.data_ptr() + 4
    stream = torch.cuda.current_stream().cuda_stream
    rcs = [
        _fwd(lib, o, out, saved, T, Nn, G, whh=bad_whh),
        _bwd(lib, o, saved, out, dgi, dgh, dh0, T, Nn, G, whh=bad_whh),
        _fwd(lib, o, out + 2, saved, T, Nn, G),
        _bwd(lib, o, saved, out, dgi + 2, dgh, dh0, T, Nn, G),
        _fwd(lib, o, None, saved, T, Nn, G),
        _bwd(lib, o, saved, out, dgi, None, dh0, T, Nn, G),
        _fwd(lib, o, out, saved, 0, Nn, G), _fwd(lib, o, out, saved, T, 0, G),
        _bwd(lib, o, saved, out, dgi, dgh, dh0, 0, Nn, G),
        _bwd(lib, o, saved, out, dgi, dgh, dh0, T, 0, G),
    ]
    assert rcs == [N.DPPO_EINVAL] * len(rcs)
    for bad_g in (0, 8, 17, 48, 128):
        assert _fwd(lib, o, out, saved, T, Nn, bad_g) == N.DPPO_EUNSUPPORTED
        assert _bwd(lib, o, saved, out, dgi, dgh, dh0, T, Nn, bad_g) == N.DPPO_EUNSUPPORTED
    assert stream == torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    for b in bufs:      # nothing ran: every output is as it was allocated
        assert torch.isnan(b.buf).all()
    with pytest.raises(Exception):
        N.check(_fwd(lib, o, out, saved, T, Nn, 48), "dppo_gru_scan_fwd_f32")
