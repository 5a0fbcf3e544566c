"""Inputs of the GRU kernels' wide-observation cases (33 <= obs_dim <= 128 under
RecurrentPPOConfig.wide_observations; csrc/grugrad.hip's gru_grad_kernel<G, true>):
tests/gru_wide_cases.py's recipe, Case and guards at the observation widths where the kernel's
phase A and F take another path.  Test infrastructure only.

Per G, with E = the gradient kernel's envs per workgroup:
  (5, 3, 33, 2)       one column past the first block of 32
  (7, E + 1, 64, 3)   two full blocks, a 1-env last workgroup
  (3, 5, 65, 4)       one column past the second block
  (6, 2E + 1, 100, 6) D16 = 112: the last 16-column tile of the Wb gradient is part used
  (4, 9, 127, 16)     one column short of the full width
  (9, 18, 128, 16)    the full width with all 16 actions
each off-policy at frac 1.0 and 0.4, two of them on-policy.  The default recipe (observations
N(0, 1), orthogonal Wb + 0.3 N(0, 1)) puts about 47 % of the base units past |tanh| 0.99 at
D = 128; ``obs_scale=0.25`` (about 1 %) checks the Wb gradient in the linear range as well.
LONG_CASES: per G one shape at D = 128 whose full workgroups hold more samples than one pass of
the kernel's 256 threads, also with the dones patterns that reset the BPTT carry.

Every case has seed_shift 0: tests/test_gru_obs_cpu.py is the proof that the clip-regime guards
(gru_cases.guards) hold there on the float64 oracle alone."""
from gru_wide_cases import ENVS_PER_WG, Case, build, guards, workgroups  # noqa: F401

WIDTHS = (16, 32, 64)
_x = lambda s: "x".join(map(str, s))


def shapes(G):
    E = ENVS_PER_WG[G]
    return [(5, 3, 33, 2), (7, E + 1, 64, 3), (3, 5, 65, 4), (6, 2 * E + 1, 100, 6),
            (4, 9, 127, 16), (9, 18, 128, 16)]


def on_policy_shapes(G):
    return [(7, ENVS_PER_WG[G] + 1, 64, 3), (9, 18, 128, 16)]


def _cases(G):
    return ([Case(f"obs-{_x(s)}-{f}", s, frac=f, G=G) for s in shapes(G) for f in (1.0, 0.4)]
            + [Case(f"obs-onpolicy-{_x(s)}", s, on_policy=True, G=G) for s in on_policy_shapes(G)]
            + [Case(f"obs-linear-{_x(s)}-{f}", s, frac=f, obs_scale=0.25, G=G)
               for s in reversed(on_policy_shapes(G)) for f in (1.0, 0.4)])


CASES = [c for G in WIDTHS for c in _cases(G)]

# a full workgroup of 320 / 320 / 288 samples, and a partial one
LONG_SHAPE = {16: (20, 29, 128, 3), 32: (40, 15, 128, 3), 64: (72, 7, 128, 3)}
LONG_CASES = [c for G in WIDTHS for c in (
    [Case(f"obs-long-{_x(LONG_SHAPE[G])}-{f}", LONG_SHAPE[G], frac=f, G=G) for f in (1.0, 0.4)]
    + [Case(f"obs-long-dones-{d}-{_x(LONG_SHAPE[G])}", LONG_SHAPE[G], dones=d, G=G)
       for d in ("env_always", "last")])]
