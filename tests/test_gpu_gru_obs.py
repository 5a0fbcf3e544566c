"""The fused RecurrentPPO minibatch kernel at observations of 33 to 128 floats
(csrc/grugrad.hip's gru_grad_kernel<G, true> behind dppo_gru_minibatch_grad_f32, asked for with
RecurrentPPOConfig.wide_observations) against the float64 autograd oracle (oracle/gru_torch.py) on
the cases of tests/gru_obs_cases.py, under tests/test_gpu_gru_wide.py's checks (_check_case) and
the project's bound for this kernel: per tensor max|diff| <= 2e-5 x max|g|, loss sums rtol 1e-5 and
atol 1e-5 m, a repeat call bit for bit, m = 0 exact zeros, and the agent on the fused path at the
case's obs_dim.  Without the flag such an agent stays on the torch path; at obs_dim <= 32 the flag
changes no bit.

Measured on an MI355X: max|diff| / max|g| over the 66 cases 1.7e-7 .. 1.1e-6 (largest per G:
7.0e-7, 8.5e-7, 1.1e-6 at (3, 5, 65, 4) share 0.4; obs_scale 0.25: 1.7e-7 .. 6.1e-7); on the 12
long cases the kernel 2.1e-7 .. 4.3e-7, the float32 oracle 3.2e-7 .. 6.4e-7."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import gru_obs_cases as O
import gru_wide_cases as W
import regime_cases as R

import test_gpu_gru_wide as base
from test_gpu_gru import _kernel_grad


def _check_case(case):
    """base._check_case on an agent built with the flag (base._case_agent builds its own without
    it, which at these widths has no fused path: the shared dict is filled first)."""
    key = (case.G, case.shape)
    if key not in base._case_agents:
        base._case_agents[key] = base._agent(*case.shape, case.G, wide_observations=True)
    agent = base._case_agents[key]
    assert agent.gru is not None, "obs_dim %d did not take the fused path" % case.shape[2]
    assert agent.gru.dims.obs_dim == case.shape[2] > 32 and agent.gru.dims.wide_obs == 1
    return base._check_case(case)


@pytest.mark.parametrize("case", O.CASES, ids=str)
def test_obs_gru_minibatch_gradient(case):
    _check_case(case)


@pytest.mark.parametrize("case", O.LONG_CASES, ids=str)
def test_obs_gru_minibatch_gradient_long(case):
    """More than one pass of the 256 threads per workgroup at D = 128."""
    params, x, mb_idx, m_total, g, ref, worst = _check_case(case)
    _, err32 = R.gru_oracle_pair(case, params, x, mb_idx, m_total)
    print(f"{case}: err_kernel {worst:.2e} err_oracle32 {err32:.2e} m {len(mb_idx)}")


def test_without_the_flag_the_agent_stays_on_torch():
    agent = base._agent(4, 5, 64, 3, 16)
    assert agent.gru is None
    assert base._agent(4, 5, 64, 3, 16, wide_observations=True).gru is not None


@pytest.mark.parametrize("G", O.WIDTHS)
def test_flag_changes_no_bit_at_narrow_observations(G):
    case = W.Case("flag-7x17x8x3", (7, 17, 8, 3), G=G)
    params, x, mb_idx, m_total = W.build(case)
    grads = []
    for flag in (False, True):
        agent = base._agent(*case.shape, G, wide_observations=flag)
        assert agent.gru is not None and agent.gru.dims.wide_obs == int(flag)
        with torch.no_grad():
            for n, p in agent.network.named_parameters():
                p.copy_(torch.from_numpy(params[n]))
        grads.append(_kernel_grad(agent, x, mb_idx, m_total, case.clip, case.vf, case.ent))
    assert torch.count_nonzero(grads[0]).item() > agent.gru.layout.total // 2
    assert torch.equal(grads[0], grads[1])
    assert np.isfinite(grads[0].cpu().numpy()).all()
