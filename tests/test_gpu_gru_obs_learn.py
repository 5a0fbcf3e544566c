"""RecurrentPPO.learn() at observations of 33 to 128 floats (RecurrentPPOConfig.wide_observations)
against oracle/gru_torch.py's learn(): tests/test_gpu_gru_wide_learn.py's procedure (_oracle, _run)
and bounds on (T, N, D, A) = (8, 20, 100, 6) with 2 epochs x 2 minibatches at gru_hidden_dim 16,
32 and 64, and at 64 on (72, 5, 128, 3) -- full workgroups of 288 samples, more than one pass of
the gradient kernel's 256 threads, and a 1-env last workgroup -- with 2 epochs x 3 minibatches;
two learn() calls under a decaying LR.  Both of the agent's paths -- the fused kernel
(fused_gru=True, csrc/grugrad.hip's wide-observation form) and torch autograd (fused_gru=False) --
are compared with the oracle, then with each other.

Bounds, unchanged: parameters, the fused path within max(2e-5, 2 x the torch path's deviation),
the torch path within 2e-5 grown in proportion to steps x lr (4e-5 at 8 steps, 6e-5 at 12); Adam
m and v relative to their largest entry, floors 1e-3 and 2e-3; the two paths within 2e-5 of each
other.

Measured on an MI355X, max|param - oracle| (parameters moved by 2.0e-3 / 3.1e-3), torch path then
fused path: (8, 20, 100, 6) G 16 3.0e-8 / 3.0e-8, G 32 6.0e-8 / 3.0e-8, G 64 3.0e-8 / 3.1e-8;
(72, 5, 128, 3) G 64 3.0e-8 / 3.0e-8.  m 0.6e-7 .. 2.1e-7 and v 1.3e-5 of their largest entry on
either path, every shape; normalised advantages equal to the oracle's bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import diamond
import gru_obs_cases as O

import test_gpu_gru_wide_learn as base

SHAPE = (8, 20, 100, 6)
LONG_SHAPE = (72, 5, 128, 3)
CASES = [(G, SHAPE) for G in O.WIDTHS] + [(64, LONG_SHAPE)]


def _kw(shape):
    return dict(num_epochs=2, num_minibatches=2 if shape == SHAPE else 3, decay_lr=True,
                total_steps=3 * shape[0] * shape[1])


def _config(G, shape):
    return diamond.RecurrentPPOConfig(rollout_steps=shape[0], num_envs=shape[1], verbose=False,
                                      gru_hidden_dim=G, wide_observations=True, **_kw(shape))


@pytest.fixture(autouse=True)
def _wide_observation_configs(monkeypatch):
    """base._oracle and base._run build their configs through the module's _config / _kw: here
    they get this module's, with the flag on.  Their caches are keyed by (G, shape), and no shape
    of this module is one of base's."""
    assert not {s for _, s in CASES} & {s for _, s in base.CASES}
    monkeypatch.setattr(base, "_config", _config)
    monkeypatch.setattr(base, "_kw", _kw)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "torch"])
@pytest.mark.parametrize("case", CASES, ids=base._id)
def test_obs_recurrent_learn_matches_oracle(case, fused):
    G, shape = case
    KW = _kw(shape)
    torch_dev = base._run(G, shape, False)[0]
    dev = base._run(G, shape, fused)[0]
    if fused:
        bound = dict(p=max(2e-5, 2 * torch_dev["p"]), m=max(1e-3, 2 * torch_dev["m"]),
                     v=max(2e-3, 2 * torch_dev["v"]))
    else:
        steps = KW["num_epochs"] * KW["num_minibatches"] * len(base.SEEDS)
        bound = dict(p=2e-5 * max(1.0, steps * 3e-4 / (4 * 3e-4)), m=1e-3, v=2e-3)
    for k in ("p", "m", "v"):
        assert dev[k] <= bound[k], (k, dev[k], bound[k], torch_dev[k])


@pytest.mark.parametrize("case", CASES, ids=base._id)
def test_obs_recurrent_learn_fused_matches_torch_path(case):
    _, p1, m1 = base._run(*case, True)
    _, p2, m2 = base._run(*case, False)
    assert np.abs(p1 - p2).max() <= 2e-5
    np.testing.assert_allclose(m1, m2, rtol=1e-3, atol=1e-7)
