"""The inputs of tests/test_gpu_tuned_fwd.py, examined without a GPU.

For the same cases, seeds and sizes (tests/tuned_fwd_cases.py; the compute-unit count that sizes
the largest case taken as the MI355X's 256), from the oracle and the NumPy Philox restatement
alone:

1. the categorical draw check leaves out the samples whose uniform lies within 1e-4 of a CDF
   boundary; at most max(1, ceil(n / 100)) samples of a case are that unclear (the GPU test asserts
   the same cap before it compares), and the oracle's draws at counter and counter + 1 differ
   wherever the GPU test asserts that they do (n >= 31);
2. the float32 oracle stays within 2e-5 max(1, |f64|) of the float64 one on heads, log-probs,
   values and next values, so the 4 |oracle32 - f64| term of the element bound is a small
   correction, not the bound itself;
3. every rollout of the reuse check is chained as described: rows that take the next_values[ip] = v
   shortcut, rows that are queued, and -- except with one env and two steps -- an episode end in a
   step before the last.
"""
import numpy as np
import pytest

from oracle import ppo_np as P

import tuned_fwd_cases as C
from test_gpu_rollout_ckpt import philox4x32_10, u01
from wide_act_cases import categorical_oracle

DRAW_CASES = C.draw_cases(cont=False)
EVAL_CASES = C.cases() + [c for c in C.align_cases() if c not in C.cases()] + C.wide_cases()


def _resolve(case):
    return (*case[:4], C.real_n(case[4], C.MI355X_CUS))


@pytest.mark.parametrize("case", DRAW_CASES, ids=C.case_id)
def test_categorical_draw_inputs_are_clear_of_cdf_boundaries(case):
    Hd, D, A, cont, n = _resolve(case)
    params, _, obs, _, _ = C.inputs(Hd, D, A, cont, n)
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    logits = P.forward(p64, obs, False, np.float64)["out"]
    want, clear = categorical_oracle(logits, C.SEED, C.COUNTER, philox4x32_10, u01)
    unclear = int((~clear).sum())
    print(f"{C.case_id(case)}: {unclear} of {n} samples unclear (cap {C.max_unclear(n)})")
    assert want.min() >= 0 and want.max() < A
    assert unclear <= C.max_unclear(n), (unclear, n)
    if n >= 31:
        other, _ = categorical_oracle(logits, C.SEED, C.COUNTER + 1, philox4x32_10, u01)
        assert not np.array_equal(want, other)


@pytest.mark.parametrize("case", EVAL_CASES + C.sweep_cases(), ids=C.case_id)
def test_float32_oracle_is_close_to_the_float64_one(case):
    Hd, D, A, cont, n = _resolve(case)
    params, _, obs, nobs, act = C.inputs(Hd, D, A, cont, n)
    worst = {}
    for k, (x64, x32) in C.oracle_eval(params, obs, act, nobs, cont).items():
        d = np.abs(x32.astype(np.float64) - x64)
        worst[k] = float(d.max())
        assert np.all(d <= 2e-5 * np.maximum(1.0, np.abs(x64))), (k, worst[k])
    print(f"{C.case_id(case)}: max |oracle32 - f64| " +
          " ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("case", C.REUSE_CASES, ids=C.reuse_id)
def test_reuse_rollouts_are_chained(case):
    T, Nn, D, A, cont = case
    _, _, (obs, nobs, *_), keep = C.chained_rollout(*case)
    same = (nobs[:-1].view(np.uint32) == obs[1:].view(np.uint32)).all(-1)  # [T - 1][N]
    print(f"{C.reuse_id(case)}: {int(same.sum())} rows take the shortcut, {int((~same).sum())} "
          f"episode ends before the last step, {Nn} rows of the last step")
    assert np.array_equal(same, ~keep)
    assert same.any()                          # the shortcut is taken
    assert T * Nn - int(same.sum()) >= Nn >= 1  # the last step's rows are queued
    if (T, Nn) != (2, 1):
        assert keep.any()                      # and so is a predecessor row
