"""GPU checks of the wide family's launch configurations (csrc/mbwide.hip wide_mb_kernel,
wide_eval_kernel, wide_pack_kernel; csrc/optim.hip slab_reduce_kernel) that
tests/test_gpu_wide.py does not reach.  Cases, inputs and bounds: tests/wide_mb_cases.py;
tests/test_wide_mb_cpu.py asserts the tables' coverage, the sizes' conditions and that the float32
oracle meets the same bounds on the same inputs.

The yardstick is oracle/ppo_np.py in float64 (minibatch_loss_grads(dt=np.float64),
tuned_fwd_cases.oracle_eval).  Bounds are test_gpu_wide._check's (overall 2e-5 max|g|, each tensor
1e-4 of its own scale floored at 1e-3 max|g|, loss and entropy 2e-5 max(1, |x|)); the capped-grid
gradient takes test_full_minibatch_gradient_vs_oracle's (also 4 x the float32 oracle's distance
+ 1e-6 max|g|, all four loss terms).

A  every reachable wide_mb_kernel<H, CONT, NB1> at m = 379 (12 tiles, 6 workgroups); the same ten
   run off-policy in tests/test_gpu_offpolicy.py through gpu_helpers.OFFPOLICY_SHAPES
B  first-layer widths D = 16k - 1, 16k, 16k + 1 at hidden 128 and (D >= 33) 64
C  action counts 1..16, categorical and Gaussian
D  3, 5 and 7 tiles: one workgroup with three tiles, or workgroups with two and three
E  m = 32 (2 CUs + 1) + 7: grid == CUs, two and three tiles per workgroup, slab_sum's batched
   loop; prepare() with more than 32 CUs samples (wide_eval_kernel's second tile); then m = 7 and
   m = 379 on the same handle (a smaller grid ignores the larger grid's slabs)
F  B = 28,800 records of 148 floats: wide_pack_kernel's second grid-stride pass
G  learn() with B = 105 and m = 35

Measured on an MI355X (largest overall error / max|g| and largest per-tensor error / own scale
over the group's cases; every case is printed by its test):

    group                     overall  worst tensor
    A  on-policy              1.3e-6   2.0e-5  (H64 D57 A11 Gaussian, actor_log_std)
    A  off-policy (24 cases)  3.3e-6   5.2e-6
    B                         3.0e-7   1.2e-6
    C                         3.3e-6   7.2e-5  (H128 D8 A1 Gaussian, output bias)
    D                         3.7e-7   4.1e-6
    E  m = 16,423             3.3e-7   5.8e-5  (H64 D105 A8 Gaussian, actor_log_std)
    E  then m = 7, 379        3.2e-6   5.4e-6  (with another index draw of the same sizes)
    F                         8.1e-7   4.5e-6

E's kernel error beside the float32 oracle's own, overall / max|g|: 2.6e-8 | 9.7e-7 (H128 D8 A4
categorical), 7.6e-8 | 6.6e-7 (H128 D17 A6 Gaussian), 3.3e-7 | 8.9e-7 (H64 D105 A8 Gaussian).
The three per-tensor figures above 1e-5 are Gaussian-head tensors on-policy whose policy term
nearly cancels over the minibatch, measured against the 1e-3 max|g| floor; the float32 oracle is
at 1.7e-5, 2.8e-5 and 2.1e-5 on the same three.  Nothing missed a bound, so nothing in
mbwide.hip or optim.hip changed.

Sensitivity: the hand mutations of the kernel source (the W1 slab guard one column short, the Wo
slab guard one action short, slab_reduce skipping a slab at G == CUs) were NOT run.  In their
place tests/test_wide_mb_cpu.py applies the same three omissions to the float32 oracle's gradient
and asserts that these bounds turn each one down at every case of B, C and E.  Without a
restriction to the widths and action counts that are new here, the first two omissions are wrong
at every shape, so the earlier gradient tests would see them as well; the third needs G == CUs,
which only group E reaches among the wide tests (the largest grid before was 24).
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import diamond
from diamond import _native as N
from oracle import ppo_np as P

import tuned_fwd_cases as TF
import wide_mb_cases as C
from gpu_helpers import SpecEnvs, dev, hparams, stream, synth, to_device

_KEYS = ("log_probs", "values", "next_values", "advantages", "returns")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _prepare(h, flat, host):
    """dppo_prepare_f32 on the rollout: (device parameters, hyper-parameters, the five outputs)"""
    B = h.dims.rollout_steps * h.dims.num_envs
    ro = to_device(host)
    pd = torch.from_numpy(flat).to(dev())
    outs = {k: torch.empty(B, device=dev()) for k in _KEYS}
    lo = N.LearnOutputs(*[outs[k].data_ptr() for k in _KEYS])
    hp = hparams()
    N.check(h.lib.dppo_prepare_f32(h.h, ctypes.byref(ro.as_struct()), pd.data_ptr(),
                                   ctypes.byref(hp), ctypes.byref(lo), stream()))
    torch.cuda.synchronize()
    return pd, hp, {k: v.cpu().numpy() for k, v in outs.items()}


def _gradient(h, pd, hp, idx):
    idx_d = torch.from_numpy(idx).to(dev())
    g = torch.zeros(h.layout.total, device=dev())
    loss4 = (ctypes.c_float * 4)()
    N.check(h.lib.dppo_minibatch_grad_f32(h.h, pd.data_ptr(), idx_d.data_ptr(), idx.size, idx.size,
                                          ctypes.byref(hp), g.data_ptr(), loss4, stream()))
    torch.cuda.synchronize()
    return g.cpu().numpy(), tuple(loss4)


def _plan(h, mb):
    p = h.fused_plan(mb)
    assert p["shape_class"] == "wide"
    return p["tile"], p["grid"]


def _check_records(o, params, host, cont):
    """test_wide_old_policy_and_records_vs_oracle's assertions, the oracle in float64"""
    obs, nobs, act, rew, te, tr = host
    T, Nn, D = obs.shape
    B = T * Nn
    act_f = act.reshape(B, -1) if cont else act.reshape(B)
    ref = TF.oracle_eval(params, obs.reshape(B, D), act_f, nobs.reshape(B, D), cont)
    for k in ("log_probs", "values", "next_values"):
        np.testing.assert_allclose(o[k], ref[k][0], rtol=2e-5, atol=2e-5, err_msg=k)
    vals = o["values"].reshape(T, Nn)
    adv = P.gae(rew, te, tr, vals, o["next_values"].reshape(T, Nn))
    assert np.array_equal(o["returns"].reshape(T, Nn), vals + adv)
    np.testing.assert_allclose(o["advantages"], P.normalize_adv(adv).ravel(), rtol=0, atol=2e-6)


def _check_minibatch(h, case, pd, hp, o, idx, production=False):
    """One minibatch gradient of the handle against the float64 oracle on the kernel's own
    records (wide_mb_cases.check_gradient)."""
    _grp, seed, Hd, D, A, cont, T, Nn, M, _mb = case
    L, names, params, _flat, host = C.inputs(seed, Hd, D, A, cont, T, Nn, M)
    got, loss4 = _gradient(h, pd, hp, idx)
    ref64 = C.oracle_gradient(params, host, cont, o, idx, np.float64)
    ref32 = C.oracle_gradient(params, host, cont, o, idx, np.float32) if production else None
    return C.check_gradient(L, names, got, loss4, ref64, f"{C.case_id(case)} m={idx.size}", ref32)


def _run_small(case):
    _grp, seed, Hd, D, A, cont, T, Nn, M, mb = case
    h = N.Handle(0, C.dims(Hd, D, A, cont, T, Nn, M))
    tile, grid = _plan(h, mb)
    _L, _names, _params, flat, host = C.inputs(seed, Hd, D, A, cont, T, Nn, M)
    pd, hp, o = _prepare(h, flat, host)
    _check_minibatch(h, case, pd, hp, o, C.minibatch_idx(seed, T * Nn, mb))
    return tile, grid


def _ids(cases):
    return [C.case_id(c) for c in cases]


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.cases_of("A"), ids=_ids(C.cases_of("A")))
def test_every_instantiation_on_policy(case):
    """One shape per reachable wide_mb_kernel<H, CONT, NB1> (NB1 is wide_mb_cases.nb1: not visible
    through the ABI); twelve tiles on six workgroups, the last tile partial."""
    tile, grid = _run_small(case)
    assert (tile, grid) == (C.S, 6)
    assert C.tiles_per_group(case[9], tile, grid) == (2, 2) and case[9] % tile != 0


@pytest.mark.parametrize("case", C.cases_of("B"), ids=_ids(C.cases_of("B")))
def test_first_layer_width_edges(case):
    """D around every multiple of 16: the record's D8, the image's D16 and the slab write's
    `k < D` differ; every dW1 block count 1..8, the part-used sets of NB1 = 4 and 8 included."""
    assert _run_small(case) == (C.S, 1)


@pytest.mark.parametrize("case", C.cases_of("C"), ids=_ids(C.cases_of("C")))
def test_action_counts(case):
    """A = 1..16: the `4 g + v < A` and `r < A` guards of the slab write and the `c < A` head
    loops."""
    assert _run_small(case) == (C.S, 1)


@pytest.mark.parametrize("case", C.cases_of("D"), ids=_ids(C.cases_of("D")))
def test_unequal_tile_counts(case):
    """3, 5 and 7 tiles: the library's own plan gives one workgroup three tiles, or some
    workgroup more tiles than another."""
    tile, grid = _run_small(case)
    lo, hi = C.tiles_per_group(case[9], tile, grid)
    assert hi > lo or (grid == 1 and hi == 3), (grid, lo, hi)
    assert case[9] % tile != 0


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", range(len(C.CAPPED_SHAPES)),
                         ids=[C.shape_id(s) for s in C.CAPPED_SHAPES])
def test_capped_grid(j):
    """The smallest minibatch at which wide_grid's cap binds, sized from the device's CU count
    and the library's plan: every workgroup strides by gridDim.x over two or three tiles, the
    last tile is partial, and slab_reduce sums CUs slabs.  The same prepare() runs
    wide_eval_kernel over more than one tile per workgroup with a partial last tile.  Then, on
    the same handle and records, m = 7 (one workgroup) and m = 379 (six): their gradients are
    right only if the reduction leaves the larger grid's slabs out."""
    cus = _cus()
    case = C.capped_case(j, cus)
    _grp, seed, Hd, D, A, cont, T, Nn, M, mb = case
    B = T * Nn
    h = N.Handle(0, C.dims(Hd, D, A, cont, T, Nn, M))
    tile, grid = _plan(h, mb)
    assert tile == C.S and grid == cus
    assert C.tiles_per_group(mb, tile, grid) == (2, 3) and mb % tile != 0
    assert mb < B and B % tile != 0 and B > tile * cus
    _L, _names, params, flat, host = C.inputs(seed, Hd, D, A, cont, T, Nn, M)
    pd, hp, o = _prepare(h, flat, host)
    _check_records(o, params, host, cont)
    _check_minibatch(h, case, pd, hp, o, C.minibatch_idx(seed, B, mb), production=True)
    for small in C.CAPPED_AFTER:
        assert _plan(h, small)[1] == C.wide_grid(small, cus) < grid
        _check_minibatch(h, case, pd, hp, o, C.minibatch_idx(seed, B, small))


def test_pack_second_pass():
    """B * R / 4 16-byte record pieces exceed launch_wide_pack's 4,096 blocks of 256 threads, so
    the samples from 28,339 on are packed in the second grid-stride pass.  The minibatch holds
    every one of them and as many of the others.  Each sample adds a term of about 1 / m of the
    gradient (m = 922) that depends on every field of its record -- the observation through all
    five weight gradients, the action, old log-prob and advantage through the policy delta, the
    return through the value delta -- so a record written to the wrong place, from the wrong
    sample or not at all moves the gradient by about 1e-3 max|g|, fifty times the bound."""
    Hd, D, A, cont = C.PACK_SHAPE
    T, Nn, M, seed = C.PACK_T, C.PACK_N, 1, 600
    B = T * Nn
    R = C.record_floats(D, A, cont)
    first = C.pack_first_second_pass_sample()
    assert B * (R // 4) > C.PACK_BLOCKS * C.PACK_THREADS >= first * (R // 4)
    idx = C.pack_idx(seed, B, first)
    h = N.Handle(0, C.dims(Hd, D, A, cont, T, Nn, M))
    _plan(h, idx.size)
    _L, _names, params, flat, host = C.inputs(seed, Hd, D, A, cont, T, Nn, M)
    pd, hp, o = _prepare(h, flat, host)
    _check_records(o, params, host, cont)
    _check_minibatch(h, ("F", seed, Hd, D, A, cont, T, Nn, M, idx.size), pd, hp, o, idx)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hd,D,A,cont", C.LEARN_SHAPES,
                         ids=[C.shape_id(s) for s in C.LEARN_SHAPES])
def test_ragged_learn_vs_oracle(Hd, D, A, cont):
    """test_wide_learn_vs_oracle with B = 105 and m = 35, neither a multiple of the tile: 12 Adam
    steps of one workgroup on a full and a 3-sample tile."""
    T, Nn, M = C.LEARN_T, C.LEARN_N, C.LEARN_M
    Cfg = diamond.ContinuousPPOConfig if cont else diamond.PPOConfig
    Agent = diamond.ContinuousPPO if cont else diamond.PPO
    cfg = Cfg(network_hidden_dim=Hd, rollout_steps=T, num_envs=Nn, num_minibatches=M,
              verbose=False)
    agent = Agent(None, cfg, envs=SpecEnvs(D, A, cont))
    assert agent._learner.fused and agent._learner.shape_class == "wide"
    names = [n for n, _ in agent.network.named_parameters()]
    params = {n: p.detach().cpu().numpy().copy() for n, p in agent.network.named_parameters()}
    seed = 700 + Hd + D
    ro, host = synth(T, Nn, D, A, cont, seed)
    np.random.seed(seed)
    st = np.random.get_state()
    agent.learn_device(ro)
    tr = agent.learn_trace()
    torch.cuda.synchronize()
    np.random.set_state(st)
    adam = P.new_adam_state(params, names)
    ref = P.learn(params, adam, list(host), P.Hyper(num_minibatches=M), cfg.lr, cont,
                  rng=np.random)
    assert len(ref["loss"]) == 4 * M == tr.shape[0]
    np.testing.assert_allclose(tr[:, 0], ref["loss"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(tr[:, 4], ref["norm"], rtol=1e-4, atol=1e-5)
    for n, p in agent.network.named_parameters():
        np.testing.assert_allclose(p.detach().cpu().numpy(), params[n], rtol=0, atol=2e-5,
                                   err_msg=n)
