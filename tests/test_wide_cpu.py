"""The shape-class predicate of the fused path (diamond/engine.py fused_shape_class; the same
predicate as dppo_create's in csrc/capi.cpp).  No GPU needed."""
import pytest

from diamond.engine import fused_shape_class

TUNED = [(64, 32, 16, 1)]
WIDE = [(128, 1, 2, 1), (128, 128, 16, 1), (64, 33, 2, 1), (64, 128, 16, 1)]
NONE = [(128, 129, 2, 1), (256, 8, 4, 1), (96, 8, 4, 1), (128, 8, 17, 1), (128, 8, 4, 2)]


def test_shape_classes(monkeypatch):
    monkeypatch.delenv("DPPO_WIDE", raising=False)
    for s in TUNED:
        assert fused_shape_class(*s) == "tuned", s
    for s in WIDE:
        assert fused_shape_class(*s) == "wide", s
    for s in NONE:
        assert fused_shape_class(*s) is None, s


def test_tuned_class_keeps_its_ranks(monkeypatch):
    """Only the wide class is single-rank: a tuned shape stays fused at any world size."""
    monkeypatch.delenv("DPPO_WIDE", raising=False)
    assert fused_shape_class(64, 8, 4, 8) == "tuned"
    assert fused_shape_class(64, 33, 4, 2) is None


@pytest.mark.parametrize("value", ["0"])
def test_dppo_wide_0_turns_the_wide_class_off(monkeypatch, value):
    monkeypatch.setenv("DPPO_WIDE", value)
    for s in WIDE:
        assert fused_shape_class(*s) is None, s
    for s in TUNED:
        assert fused_shape_class(*s) == "tuned", s
    for s in NONE:
        assert fused_shape_class(*s) is None, s
