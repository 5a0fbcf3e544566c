"""The inputs of tests/test_gpu_wide_act.py's discrete-draw check, examined without a GPU.

That check compares dppo_act_f32 at wide shapes with the inverse CDF of the oracle's softmax on
the samples whose uniform lies farther than 1e-4 from every CDF boundary, on condition that at
least 99 % of the samples are that clear.  Here the clear share is computed from the oracle and
the NumPy Philox restatement alone, for the same shapes, sizes, seed and counter (the compute-unit
count that sizes the largest case taken as the MI355X's 256): the inputs themselves keep the
condition, so a GPU run that misses it has drawn from other logits or another stream.
"""
import pytest

from oracle import ppo_np as P

import wide_act_cases as W
from test_gpu_rollout_ckpt import philox4x32_10, u01

CASES = W.cases(cont=False)


@pytest.mark.parametrize("case", CASES, ids=[W.case_id(c) for c in CASES])
def test_discrete_draw_inputs_are_clear_of_cdf_boundaries(case):
    Hd, D, A, cont, n = case
    n = W.real_n(n, W.MI355X_CUS)
    params, _, obs = W.inputs(Hd, D, A, cont, n)
    logits = P.forward(params, obs, False)["out"]
    want, clear = W.categorical_oracle(logits, W.SEED, W.COUNTER, philox4x32_10, u01)
    print(f"{W.case_id(case)}: clear share {clear.mean():.4f}")
    assert want.min() >= 0 and want.max() < A
    assert clear.mean() >= W.MIN_CLEAR, clear.mean()
