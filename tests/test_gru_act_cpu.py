"""Host-side surface of RecurrentPPO's fused rollout step (csrc/gruact.hip; include/dppo.h
dppo_gru_act_f32 / dppo_gru_value_f32): the symbols exist, reject bad arguments before any HIP
call, and the Python switch is off by default.  The kernels themselves: tests/test_gpu_gru_act.py."""
import pytest

import diamond
from diamond import _native as N

SYMBOLS = ["dppo_gru_act_f32", "dppo_gru_value_f32"]


def test_rollout_symbols_are_exported():
    lib = N.load()
    for s in SYMBOLS:
        assert s in N.EXPORTED
        assert hasattr(lib, s), s


def test_null_handle_is_einval_without_a_device():
    lib = N.load()
    with pytest.raises(ValueError, match="dppo_gru_act_f32"):
        N.check(lib.dppo_gru_act_f32(None, None, None, 4, 1, 0, None), "dppo_gru_act_f32")
    with pytest.raises(ValueError, match="dppo_gru_value_f32"):
        N.check(lib.dppo_gru_value_f32(None, None, None, None, None, 4, None, None),
                "dppo_gru_value_f32")
    with pytest.raises(ValueError):
        N.check(lib.dppo_gru_set_timing(None, 1))
    with pytest.raises(ValueError):
        N.check(lib.dppo_gru_get_timing(None, None, None))


def test_step_struct_matches_the_header_field_order():
    assert [f[0] for f in N.GruStep._fields_] == ["obs", "prev_dones", "hx", "hx_out", "actions",
                                                  "log_probs", "values", "logits"]


def test_fused_rollout_is_off_by_default():
    assert diamond.RecurrentPPO.fused_rollout is False
    assert diamond.RecurrentPPO.fused_gru is True
