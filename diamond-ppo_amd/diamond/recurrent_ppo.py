"""RecurrentPPO (GRU core) -- API-compatible with reference ``diamond/recurrent_ppo.py``.

The reference cannot run: ``GRUCore.forward`` evaluates ``hx or torch.zeros(...)`` and
``dones or ...`` on multi-element tensors (recurrent_ppo.py:78-79), so both ``rollout()`` and
``learn()`` raise ``RuntimeError``.  This module implements the intended
semantics: per-timestep GRU with the hidden state reset where ``dones[t]`` (:82-87), old
log-probs / values / next-values cached during rollout (:219-243), and ``learn`` recomputing the
full [T, N] sequence from the stored initial ``hx`` for every minibatch (:337-341).  The network
runs under torch autograd on the GPU; GAE, advantage normalisation and clip + Adam run in the
gfx950 kernels.  No oracle pins this path beyond the shared GAE (reference broken).  For the
default network, learn()'s minibatches (``fused_gru``) and, when switched on, rollout()'s env steps
(``fused_rollout``) run as fused HIP kernels instead.

Data parallelism (torchrun, one process per GPU): each rank owns its own envs (seeded
``seed + rank * num_envs``) and permutes its own samples (``np.random`` seeded ``seed + rank``);
global minibatch j is the union of the ranks' local minibatches j.  The advantage statistics are
global (the ranks' {sum, sum^2} all-reduced, ppo.py:243 over the global batch), each rank's loss
is its local mean scaled by 1/world, and the flat gradient is all-reduced (SUM, RCCL under the
"nccl" backend) before the replicated clip + Adam -- so every rank takes the identical step.
"""
from __future__ import annotations

import ctypes
import os
import time
from dataclasses import dataclass
from math import sqrt
from typing import Any, Callable

import numpy as np
import torch
import torch.nn as nn

from . import _native as N
from ._spaces import is_box, is_discrete, make_vector_env
from .engine import FlatParams, bind_adam_state, adam_step_count, advance_adam_steps, \
    broadcast_flat, clip_adam, dist_world, fused_ppo_loss, hparams, require_gpu, \
    torch_ppo_terms, LOSS_KERNEL_CALLS
from .utils import Checkpointer, Logger, Ticker, Timer


@dataclass
class RecurrentPPOConfig:
    total_steps: int = 1_000_000
    rollout_steps: int = 32
    num_envs: int = 32
    lr: float = 3e-4
    adam_eps: float = 1e-5
    decay_lr: bool = False
    gamma: float = 0.99
    gae_lambda: float = 0.95
    num_epochs: int = 10
    num_minibatches: int = 1
    ppo_clip: float = 0.15
    value_loss_weight: float = 1.0
    entropy_beta: float = 0.01
    advantage_norm: bool = True
    grad_norm_clip: float = 0.5
    network_hidden_dim: int = 64
    gru_hidden_dim: int = 16
    cuda: bool = False
    seed: int | None = 42
    checkpoint: bool = False
    save_interval: float = 600
    verbose: bool = True
    device_index: int = 0
    gae_bitexact: bool = True   # False: the chunked affine-scan GAE kernel (PPOConfig)
    # True: the fused kernels (fused_gru, fused_rollout) also serve observations of 33 to 128
    # floats (fused_gru_shape's wide_obs); up to 32 nothing changes, bits included
    wide_observations: bool = False


CORE_SCAN_CALLS = [0]  # GRUCore forwards of this process that the scan kernels served
_SCAN_WIDTHS = (16, 32, 64)


class _FusedGRUScan(torch.autograd.Function):
    """The GRU recurrence with per-step resets as an autograd node on the scan kernels
    (csrc/gruseq.hip): forward = the input projection as one GEMM over [T N, I] and one
    dppo_gru_scan_fwd_f32 launch; backward = one dppo_gru_scan_bwd_f32 launch and the five sums
    over samples (dx, dWih, db_ih, dWhh, db_hh) as torch GEMMs / reductions.  Everything runs on
    the current stream without a host synchronisation.  ``save`` False (inference): no per-sample
    activations are kept."""

    @staticmethod
    def forward(ctx, x, hx0, dones, w_ih, w_hh, b_ih, b_hh, save):
        T, Nn, I = x.shape
        G = w_hh.shape[1]
        dev = x.device
        x2 = x.detach().reshape(T * Nn, I)
        w_ih, w_hh, b_ih, b_hh = (t.detach().contiguous() for t in (w_ih, w_hh, b_ih, b_hh))
        hx0 = hx0.detach().contiguous()
        gi = torch.addmm(b_ih, x2, w_ih.t())
        out = torch.empty((T, Nn, G), dtype=torch.float32, device=dev)
        saved = torch.empty((T, Nn, 4 * G), dtype=torch.float32, device=dev) if save else None
        N.check(N.load().dppo_gru_scan_fwd_f32(
            gi.data_ptr(), hx0.data_ptr(), dones.data_ptr() if dones is not None else None,
            w_hh.data_ptr(), b_hh.data_ptr(), out.data_ptr(),
            saved.data_ptr() if save else None, T, Nn, G,
            torch.cuda.current_stream(dev).cuda_stream), "dppo_gru_scan_fwd_f32")
        CORE_SCAN_CALLS[0] += 1
        if save:
            ctx.save_for_backward(x2, hx0, w_ih, w_hh, saved, out)
            ctx.dones = dones
        ctx.set_materialize_grads(False)
        # the final hidden state as a tensor of its own: a view of `out` could not carry the graph
        return out, out[T - 1].unsqueeze(0).clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, d_hT):
        x2, hx0, w_ih, w_hh, saved, out = ctx.saved_tensors
        dones = ctx.dones
        T, Nn, G = out.shape
        dev = out.device
        d_out = torch.zeros_like(out) if d_out is None else d_out.contiguous()
        if d_hT is not None:
            d_hT = d_hT.reshape(Nn, G).contiguous()
        dgi = torch.empty((T * Nn, 3 * G), dtype=torch.float32, device=dev)
        dgh = torch.empty((T * Nn, 3 * G), dtype=torch.float32, device=dev)
        dh0 = torch.empty((Nn, G), dtype=torch.float32, device=dev)
        N.check(N.load().dppo_gru_scan_bwd_f32(
            d_out.data_ptr(), d_hT.data_ptr() if d_hT is not None else None, saved.data_ptr(),
            out.data_ptr(), hx0.data_ptr(), dones.data_ptr() if dones is not None else None,
            w_hh.data_ptr(), dgi.data_ptr(), dgh.data_ptr(), dh0.data_ptr(), T, Nn, G,
            torch.cuda.current_stream(dev).cuda_stream), "dppo_gru_scan_bwd_f32")
        need = ctx.needs_input_grad
        dx = (dgi @ w_ih).reshape(T, Nn, -1) if need[0] else None
        d_wih = dgi.t() @ x2 if need[3] else None
        d_whh = None
        if need[4]:
            # the hidden state every step started from, after the reset: hp = h_prev * keep
            hp = torch.cat([hx0.unsqueeze(0), out[:T - 1]], dim=0)
            if dones is not None:
                hp = hp * (dones == 0).to(torch.float32).unsqueeze(-1)
            d_whh = dgh.t() @ hp.reshape(T * Nn, G)
        return (dx, dh0 if need[1] else None, None, d_wih, d_whh,
                dgi.sum(0) if need[5] else None, dgh.sum(0) if need[6] else None, None)


class GRUCore(nn.GRU):
    """GRU with per-timestep hidden resets (intended semantics of recurrent_ppo.py:41-91)."""

    def __init__(self, input_dim: int, hidden_dim: int) -> None:
        super().__init__(input_dim, hidden_dim)
        # True: forward() runs the recurrence on the scan kernels (csrc/gruseq.hip) where
        # _scan_serves admits the call; the step loop below otherwise.  Off by default: the bits
        # then differ from the loop's
        self.fused_scan = False

    def _scan_serves(self, x, hx, dones) -> bool:
        """float32 CUDA input [T >= 1, N >= 1, I], hidden 16 / 32 / 64, and the module as
        __init__ builds it: one layer, unidirectional, biases, no projection."""
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3
                and x.shape[0] >= 1 and x.shape[1] >= 1 and x.shape[2] == self.input_size):
            return False
        if not (self.hidden_size in _SCAN_WIDTHS and self.num_layers == 1
                and not self.bidirectional and self.bias and not self.batch_first
                and getattr(self, "proj_size", 0) == 0):
            return False
        w = self.weight_hh_l0
        if w.dtype != torch.float32 or w.device != x.device:
            return False
        if hx is not None and not (hx.dtype == torch.float32 and hx.device == x.device
                                   and hx.numel() == x.shape[1] * self.hidden_size):
            return False
        return dones is None or (dones.device == x.device and dones.dim() == 2
                                 and tuple(dones.shape) == tuple(x.shape[:2]))

    def _forward_scan(self, x, hx, dones):
        T, Nn = x.shape[:2]
        G = self.hidden_size
        if hx is None:
            hx0 = torch.zeros(Nn, G, dtype=x.dtype, device=x.device)
        else:
            hx0 = hx.reshape(Nn, G)
        if dones is not None:
            dones = (dones if dones.dtype == torch.bool else dones.bool()).contiguous()
            dones = dones.view(torch.uint8)
        params = (self.weight_ih_l0, self.weight_hh_l0, self.bias_ih_l0, self.bias_hh_l0)
        save = torch.is_grad_enabled() and any(t.requires_grad for t in (x, hx0) + params)
        return _FusedGRUScan.apply(x.contiguous(), hx0, dones, *params, save)

    def forward(self, x, hx=None, dones=None):
        if getattr(self, "fused_scan", False) and self._scan_serves(x, hx, dones):
            return self._forward_scan(x, hx, dones)
        seq_length, batch_size = x.shape[:2]
        if hx is None:
            hx = torch.zeros(1, batch_size, self.hidden_size, dtype=x.dtype, device=x.device)
        if dones is None:
            dones = torch.zeros(seq_length, batch_size, dtype=torch.bool, device=x.device)
        outputs = []
        for t in range(seq_length):
            keep = (~dones[t].bool()).to(hx.dtype)[None, :, None]
            hx = hx * keep                                 # hx[:, dones[t]] = 0 (:84)
            out, hx = super().forward(x[t:t + 1], hx)
            outputs.append(out)
        return torch.cat(outputs, dim=0), hx


class RecurrentActorCriticNetwork(nn.Module):
    def __init__(self, observation_space, action_space, cfg: RecurrentPPOConfig) -> None:
        super().__init__()
        assert is_box(observation_space), "Only Box obs spaces are supported."
        assert is_discrete(action_space), "Only Discrete action spaces are supported."
        hd, gd = cfg.network_hidden_dim, cfg.gru_hidden_dim
        self.base = nn.Sequential(nn.Linear(int(np.prod(observation_space.shape)), hd), nn.Tanh())
        self.gru = GRUCore(hd, gd)
        self.actor_head = nn.Sequential(nn.Linear(gd, hd), nn.Tanh(),
                                        nn.Linear(hd, int(action_space.n)))
        self.actor_out_layer = self.actor_head[-1]
        self.critic_head = nn.Sequential(nn.Linear(gd, hd), nn.Tanh(), nn.Linear(hd, 1))

    def get_values(self, observations, hx, dones):
        x = self.base(observations)
        x, hx = self.gru.forward(x, hx, dones)
        return self.critic_head(x).squeeze(-1)

    def get_logits_values_and_hx(self, observations, hx, dones):
        x = self.base(observations)
        x, hx = self.gru.forward(x, hx, dones)
        return self.actor_head(x), self.critic_head(x).squeeze(-1), hx


def network_parameter_init_(network: nn.Module, gain: float = 1.0) -> None:
    with torch.no_grad():
        for m in network.modules():
            if isinstance(m, nn.Linear):
                nn.init.orthogonal_(m.weight, gain=gain)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
        if hasattr(network, "actor_out_layer"):
            nn.init.orthogonal_(network.actor_out_layer.weight, gain=0.01)


def fused_gru_shape(hidden: int, gru_hidden: int, obs_dim: int, act_dim: int,
                    wide_obs: bool = False) -> bool:
    """Whether the fused GRU kernels (``fused_gru``, ``fused_rollout``) serve the default network
    at this shape: hidden 64, gru_hidden 16, 32 or 64, act_dim <= 16 and obs_dim <= 32, or
    <= 128 with ``wide_obs`` (``RecurrentPPOConfig.wide_observations``, ``dppo_gru_dims.wide_obs``).
    The same predicate as ``gru_validate`` (csrc/gru.hip).  ``DPPO_GRU_WIDE=0`` turns gru_hidden
    32 and 64 off (A/B runs against the torch path); 16 is not affected."""
    if not (hidden == 64 and 1 <= obs_dim <= (128 if wide_obs else 32) and 1 <= act_dim <= 16):
        return False
    if gru_hidden == 16:
        return True
    return gru_hidden in (32, 64) and os.environ.get("DPPO_GRU_WIDE", "1") != "0"


class RecurrentPPO:
    # learn() runs each minibatch's sequence recompute, loss and BPTT as one fused HIP launch
    # (dppo_gru_minibatch_grad_f32) for the default network at supported shapes; False (or any
    # other network_cls) runs the network under torch autograd on the GPU
    fused_gru = True
    # rollout() runs each env step's policy forward, Categorical draw and log-prob as one fused HIP
    # launch (dppo_gru_act_f32) and V(next_obs) as another (dppo_gru_value_f32), under the same
    # conditions as fused_gru.  Off by default: the actions then come from torch's generator, as
    # before; the fused path draws from its own Philox stream (same distribution, other draws)
    fused_rollout = False
    # the torch learn loop (custom network_cls or fused_gru = False) takes each minibatch's loss
    # and its backward from the loss-head kernel (engine.fused_ppo_loss, csrc/losshead.hip)
    # instead of the torch op chain; the network stays under autograd.  Off by default
    fused_loss = False
    # the torch learn loop and the torch rollout run every GRUCore of the network on the GRU scan
    # kernels (GRUCore.fused_scan, csrc/gruseq.hip): one launch for the whole forward sequence and
    # one for the BPTT instead of T cell launches each way; the rest of the network stays under
    # autograd.  Where fused_gru / fused_rollout serve the agent they win as before.  Off by
    # default: the bits then differ from nn.GRU's
    fused_core = False
    # the head, for the subclass with the Gaussian one (RecurrentContinuousPPO): which loss the
    # torch loop evaluates, and the fused minibatch launch with its batch struct and action type
    continuous = False
    _grad_entry = "dppo_gru_minibatch_grad_f32"
    _batch_struct = N.GruBatch
    _action_dtype = torch.int32

    def __init__(self, env_fn: Callable[[], Any], cfg: RecurrentPPOConfig = RecurrentPPOConfig(),
                 network_cls: Any = RecurrentActorCriticNetwork, envs=None) -> None:
        self.device = require_gpu(cfg.device_index)
        world, rank = dist_world()
        if cfg.seed is not None:
            np.random.seed(cfg.seed + rank)
            torch.manual_seed(cfg.seed)   # same initial weights on every rank
        self.envs = envs if envs is not None else make_vector_env(env_fn, cfg.num_envs)
        obs_space, act_space = self.envs.single_observation_space, self.envs.single_action_space
        self.network = network_cls(obs_space, act_space, cfg=cfg)
        network_parameter_init_(self.network, gain=sqrt(2.0))
        self.optimizer = torch.optim.Adam(self.network.parameters(), lr=cfg.lr, eps=cfg.adam_eps)
        self.flat = FlatParams(self.network, self.device)
        self.flat.bind_grads()
        self.m, self.v = bind_adam_state(self.optimizer, self.flat)
        self.optimizer._opt_called = True
        self.lr_scheduler = torch.optim.lr_scheduler.LinearLR(
            self.optimizer, start_factor=1.0, end_factor=0.05 if cfg.decay_lr else 1.0,
            total_iters=cfg.total_steps // (cfg.num_envs * cfg.rollout_steps))
        dims = N.Dims(rollout_steps=cfg.rollout_steps, num_envs=cfg.num_envs, obs_dim=1,
                      act_dim=1, continuous=0, hidden=cfg.network_hidden_dim,
                      num_epochs=cfg.num_epochs, num_minibatches=cfg.num_minibatches,
                      world_size=1, rank=0)
        self.handle = N.Handle(self.device.index or 0, dims)
        self.gru = None
        obs_dim = int(np.prod(obs_space.shape))
        wide_obs = bool(getattr(cfg, "wide_observations", False))
        if (type(self.network) is RecurrentActorCriticNetwork
                and fused_gru_shape(cfg.network_hidden_dim, cfg.gru_hidden_dim, obs_dim,
                                    int(act_space.n), wide_obs)):
            gd = N.GruDims(rollout_steps=cfg.rollout_steps, num_envs=cfg.num_envs,
                           obs_dim=obs_dim, act_dim=int(act_space.n), hidden=64,
                           gru_hidden=cfg.gru_hidden_dim, wide_obs=int(wide_obs))
            self.gru = N.GruHandle(self.device.index or 0, gd)
            L = self.gru.layout
            if L.total != self.flat.total or any(L.offset[i] != o for i, o in
                                                  enumerate(self.flat.offsets)):
                raise RuntimeError("RecurrentActorCriticNetwork layout differs from libdppo's")
        self.last_losses = None
        self.loss_head_calls = 0  # minibatches whose loss the loss-head kernel computed (fused_loss)
        self.core_scan_calls = 0  # GRUCore forwards the scan kernels served (fused_core)
        # the fused rollout's Philox key (mixed as _AgentBase._act_seed) and call counter
        base_seed = cfg.seed if cfg.seed is not None else torch.initial_seed()
        self._act_seed = (int(base_seed) * 0x9E3779B97F4A7C15 + rank) & (2 ** 64 - 1)
        self._act_counter = 0
        self._rollout_staging = None
        if not getattr(cfg, "gae_bitexact", True):
            self.handle.set_gae_mode(N.GAE_AFFINE)
        if world > 1:
            broadcast_flat(self.flat)
        self.logger, self.timer = Logger(), Timer()
        self.checkpointer = Checkpointer(folder="models", run_name="default")
        self.ticker = Ticker(cfg.total_steps, cfg.num_envs, cfg.rollout_steps, verbose=cfg.verbose)
        self.cfg = cfg

    def _set_core_scan(self) -> bool:
        """Hand ``fused_core`` to every GRUCore of the network (before a torch-path use)."""
        on = bool(self.fused_core)
        for m in self.network.modules():
            if isinstance(m, GRUCore):
                m.fused_scan = on
        return on

    def _policy_terms(self, observations, hx, prev_dones):
        """(actor output [T, N, A], log_std or None, values [T, N]) over the whole rollout, under
        autograd: what the torch learn loop differentiates."""
        nl, nv, _ = self.network.get_logits_values_and_hx(observations, hx, prev_dones)
        return nl, None, nv

    def rollout(self):
        """recurrent_ppo.py:205-263 with tensor-safe hidden-state handling."""
        if self.fused_rollout and self.gru is not None:
            return self._rollout_fused()
        self._set_core_scan()
        scans0 = CORE_SCAN_CALLS[0]
        experience = []
        observations, hx, prev_dones = self.current_observations, self.current_hx, self.prev_dones
        for _ in range(self.cfg.rollout_steps):
            obs_t = torch.as_tensor(observations[None, ...], dtype=torch.float32, device=self.device)
            pd_t = torch.as_tensor(prev_dones[None, ...], dtype=torch.bool, device=self.device)
            with torch.inference_mode():
                logits, values, new_hx = self.network.get_logits_values_and_hx(obs_t, hx, pd_t)
            dist = torch.distributions.Categorical(logits=logits.squeeze(0))
            actions = dist.sample()
            log_probs = dist.log_prob(actions)
            next_observations, rewards, terms, truncs, infos = self.envs.step(actions.cpu().numpy())
            nobs_t = torch.as_tensor(next_observations[None, ...], dtype=torch.float32,
                                     device=self.device)
            with torch.inference_mode():
                next_values = self.network.get_values(nobs_t, new_hx, None)
            experience.append([obs_t.squeeze(0), actions, rewards, terms, truncs, pd_t.squeeze(0),
                               log_probs, values.squeeze(0), next_values.squeeze(0), hx])
            dones = np.logical_or(terms, truncs)
            observations, infos = (self.envs.reset(options={"reset_mask": dones})
                                   if np.any(dones) else (next_observations, infos))
            hx, prev_dones = new_hx, dones
            if self.ticker is not None:
                self.ticker.tick(rewards, dones)
        self.current_observations, self.current_hx, self.prev_dones = observations, hx, prev_dones
        self.core_scan_calls += CORE_SCAN_CALLS[0] - scans0
        return experience

    def _rollout_fused(self):
        """rollout() on the fused kernels.  Per env step: the observations and prev_dones go up
        through pinned staging, one dppo_gru_act_f32 launch (recurrent_ppo.py:214-224), the int32
        actions come down (the step's only synchronisation), the envs step, next_observations go
        up and one dppo_gru_value_f32 launch follows from the step's new hidden state (:226-232)
        without a synchronisation.  Everything lands in device buffers allocated per call, so a
        returned experience outlives the next rollout; its rows are views of them, in the torch
        path's layout."""
        cfg, dev, lib = self.cfg, self.device, self.gru.lib
        T, Nn, G = cfg.rollout_steps, cfg.num_envs, cfg.gru_hidden_dim
        D, A = self.gru.dims.obs_dim, self.gru.dims.act_dim
        st = self._rollout_staging
        if st is None:
            pin = lambda shape, dt: torch.empty(shape, dtype=dt).pin_memory()
            st = self._rollout_staging = {
                "obs": pin((Nn, D), torch.float32), "dones": pin((Nn,), torch.bool),
                "nobs": pin((Nn, D), torch.float32), "act": pin((Nn,), torch.int32),
                "nobs_d": torch.empty((Nn, D), dtype=torch.float32, device=dev)}
            for k in ("obs", "dones", "nobs", "act"):
                st[k + "_np"] = st[k].numpy()
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        obs_d, hx_d = f32(T, Nn, D), f32(T + 1, 1, Nn, G)
        lp_d, v_d, nv_d = f32(T, Nn), f32(T, Nn), f32(T, Nn)
        pd_d = torch.empty((T, Nn), dtype=torch.bool, device=dev)
        act_d = torch.empty((T, Nn), dtype=torch.int32, device=dev)
        hx_d[0].copy_(self.current_hx.reshape(1, Nn, G))
        stream = torch.cuda.current_stream(dev)
        params = self.flat.flat.data_ptr()
        host = []
        observations, prev_dones = self.current_observations, self.prev_dones
        for t in range(T):
            st["obs_np"][...] = np.asarray(observations, dtype=np.float32).reshape(Nn, D)
            st["dones_np"][...] = prev_dones
            obs_d[t].copy_(st["obs"], non_blocking=True)
            pd_d[t].copy_(st["dones"], non_blocking=True)
            step = N.GruStep(obs_d[t].data_ptr(), pd_d[t].data_ptr(), hx_d[t].data_ptr(),
                             hx_d[t + 1].data_ptr(), act_d[t].data_ptr(), lp_d[t].data_ptr(),
                             v_d[t].data_ptr(), None)
            N.check(lib.dppo_gru_act_f32(self.gru.h, params, ctypes.byref(step), Nn,
                                         self._act_seed, self._act_counter, stream.cuda_stream),
                    "dppo_gru_act_f32")
            self._act_counter += 1
            st["act"].copy_(act_d[t], non_blocking=True)
            stream.synchronize()
            next_observations, rewards, terms, truncs, infos = self.envs.step(
                st["act_np"].astype(np.int64))
            st["nobs_np"][...] = np.asarray(next_observations, dtype=np.float32).reshape(Nn, D)
            st["nobs_d"].copy_(st["nobs"], non_blocking=True)
            N.check(lib.dppo_gru_value_f32(self.gru.h, params, st["nobs_d"].data_ptr(),
                                           hx_d[t + 1].data_ptr(), None, Nn, nv_d[t].data_ptr(),
                                           stream.cuda_stream), "dppo_gru_value_f32")
            host.append((rewards, terms, truncs))
            dones = np.logical_or(terms, truncs)
            observations, infos = (self.envs.reset(options={"reset_mask": dones})
                                   if np.any(dones) else (next_observations, infos))
            prev_dones = dones
            if self.ticker is not None:
                self.ticker.tick(rewards, dones)
        act64 = act_d.to(torch.int64)
        self.current_observations, self.prev_dones = observations, prev_dones
        self.current_hx = hx_d[T]
        return [[obs_d[t], act64[t], *host[t], pd_d[t], lp_d[t], v_d[t], nv_d[t], hx_d[t]]
                for t in range(T)]

    def calculate_advantage(self, rewards, terminations, truncations, values, next_values):
        """Shared GAE (recurrent_ppo.py:265-299) on the gfx950 kernel."""
        dev = self.device
        f = lambda x: torch.as_tensor(x, device=dev).to(torch.float32).contiguous()
        u8 = lambda x: (torch.as_tensor(x, device=dev) != 0).to(torch.uint8).contiguous()
        # every operand bound to a name until the launch is enqueued: a temporary's block would go
        # back to the caching allocator at once and could be handed to the next operand's copy
        r, v, nv = f(rewards), f(values), f(next_values)
        te, tr = u8(terminations), u8(truncations)
        adv, ret = torch.empty_like(r), torch.empty_like(r)
        stream = torch.cuda.current_stream(dev).cuda_stream
        N.check(self.handle.lib.dppo_gae_f32(
            self.handle.h, r.data_ptr(), te.data_ptr(), tr.data_ptr(),
            v.data_ptr(), nv.data_ptr(), adv.data_ptr(), ret.data_ptr(), float(self.cfg.gamma),
            float(self.cfg.gae_lambda), stream), "dppo_gae_f32")
        return adv

    def learn(self, experience) -> None:
        """recurrent_ppo.py:301-367 (intended semantics)."""
        cfg, lib, h = self.cfg, self.handle.lib, self.handle.h
        (observations, actions, rewards, terms, truncs, prev_dones, log_probs, values,
         next_values, hx) = zip(*experience)
        observations = torch.stack(observations)
        actions = torch.stack(actions)
        prev_dones = torch.stack(prev_dones)
        log_probs, values = torch.stack(log_probs), torch.stack(values)
        next_values = torch.stack(next_values)
        hx = hx[0].clone()
        advantages = self.calculate_advantage(np.asarray(rewards), np.asarray(terms),
                                              np.asarray(truncs), values, next_values)
        returns = values + advantages
        stream = torch.cuda.current_stream(self.device).cuda_stream
        world, _ = dist_world()
        if cfg.advantage_norm:
            ms = torch.empty(4, dtype=torch.float32, device=self.device)
            if world > 1:
                # global statistics: this rank's {sum, sum^2}, all-reduced, then finalised
                sums = torch.empty(2, dtype=torch.float64, device=self.device)
                N.check(lib.dppo_adv_sums(h, sums.data_ptr(), stream), "dppo_adv_sums")
                torch.distributed.all_reduce(sums)
                n_total = float(cfg.rollout_steps * cfg.num_envs * world)
                N.check(lib.dppo_adv_stats_from_sums(sums.data_ptr(), n_total, ms.data_ptr(),
                                                     stream), "dppo_adv_stats_from_sums")
            else:
                N.check(lib.dppo_adv_stats(h, ms.data_ptr(), stream), "dppo_adv_stats")
            advantages = advantages.contiguous()
            N.check(lib.dppo_adv_normalize_f32(advantages.data_ptr(), ms.data_ptr(),
                                               advantages.numel(), stream), "normalize")
        flatten = lambda x: x.reshape(-1, *x.shape[2:])
        log_probs, actions, advantages, returns = [flatten(x) for x in
                                                   (log_probs, actions, advantages, returns)]
        B = cfg.rollout_steps * cfg.num_envs
        mb = B // cfg.num_minibatches
        perms = np.empty(cfg.num_epochs * B, np.int32)
        N.numpy_rng_permutations(B, cfg.num_epochs, perms)
        idx = torch.from_numpy(perms.astype(np.int64)).to(self.device).view(
            cfg.num_epochs, cfg.num_minibatches, mb)
        step = adam_step_count(self.optimizer, self.flat)
        lr = self.optimizer.param_groups[0]["lr"]
        if self.fused_gru and self.gru is not None:
            self._learn_fused(observations, actions, log_probs, advantages, returns, prev_dones,
                              hx, idx, step, lr, world, stream)
            advance_adam_steps(self.optimizer, self.flat, cfg.num_epochs * cfg.num_minibatches)
            self.lr_scheduler.step()
            return
        fused_loss = bool(self.fused_loss)
        # with fused_core the loop records {loss, policy, value, entropy} per minibatch (this
        # rank's means), as the fused learn does
        record = [] if self._set_core_scan() else None
        scans0 = CORE_SCAN_CALLS[0]
        if fused_loss:
            act32 = actions.to(self._action_dtype).contiguous()
            old_lp, adv_c, ret_c = (x.float().contiguous() for x in
                                    (log_probs, advantages, returns))
        for b_idx in idx:
            for mb_idx in b_idx:
                self.flat.grad.zero_()
                nl, ls, nv = self._policy_terms(observations, hx, prev_dones)
                nl, nv = flatten(nl)[mb_idx], flatten(nv)[mb_idx]
                if ls is not None:
                    ls = flatten(ls)[mb_idx]
                if fused_loss:
                    calls0 = LOSS_KERNEL_CALLS[0]
                    loss, terms = fused_ppo_loss(
                        nl, nv, ls, actions=act32, old_log_probs=old_lp, advantages=adv_c,
                        returns=ret_c, idx=mb_idx, clip=cfg.ppo_clip,
                        value_loss_weight=cfg.value_loss_weight, entropy_beta=cfg.entropy_beta,
                        scale=1.0 / world if world > 1 else 1.0, continuous=self.continuous)
                    self.loss_head_calls += LOSS_KERNEL_CALLS[0] - calls0
                    if record is not None:
                        record.append(terms[:4].clone())
                else:
                    loss, l_pi, l_v, ent, _ = torch_ppo_terms(
                        nl, nv, ls, actions[mb_idx], log_probs[mb_idx], advantages[mb_idx],
                        returns[mb_idx], cfg.ppo_clip, cfg.value_loss_weight, cfg.entropy_beta,
                        self.continuous)
                    if record is not None:
                        record.append(torch.stack([loss, l_pi, l_v, ent]).detach())
                    if world > 1:
                        # local mean x 1/world, summed over the ranks = the union minibatch's mean
                        loss = loss * (1.0 / world)
                loss.backward()
                if world > 1:
                    torch.distributed.all_reduce(self.flat.grad)
                step += 1
                clip_adam(self.flat, self.m, self.v, cfg, lr, step, stream)
        self.core_scan_calls += CORE_SCAN_CALLS[0] - scans0
        if record is not None:
            self.last_losses = torch.stack(record)
            if fused_loss and world > 1:   # the kernel's loss carries the rank's 1 / world share
                self.last_losses[:, 0] *= float(world)
        advance_adam_steps(self.optimizer, self.flat, cfg.num_epochs * cfg.num_minibatches)
        self.lr_scheduler.step()

    def _learn_fused(self, observations, actions, log_probs, advantages, returns, prev_dones,
                     hx, idx, step, lr, world, stream):
        """Every minibatch: one dppo_gru_minibatch_grad_f32 launch (sequence recompute from hx,
        loss on the minibatch, BPTT; recurrent_ppo.py:335-360) -> [all-reduce] -> clip + Adam."""
        cfg, lib = self.cfg, self.gru.lib
        f32 = lambda x: x.to(torch.float32).contiguous()
        obs = f32(observations)
        act = actions.to(self._action_dtype).contiguous()
        old_lp, adv, ret = f32(log_probs), f32(advantages), f32(returns)
        dones = prev_dones.to(torch.uint8).contiguous()
        hx0 = f32(hx.reshape(cfg.num_envs, cfg.gru_hidden_dim))
        batch = self._batch_struct(obs.data_ptr(), act.data_ptr(), old_lp.data_ptr(),
                                   adv.data_ptr(),
                                   ret.data_ptr(), dones.data_ptr(), hx0.data_ptr())
        grad_fn = getattr(lib, self._grad_entry)
        hp = hparams(cfg, lr, step)
        idx32 = idx.to(torch.int32).contiguous()
        mb = idx32.shape[-1]
        m_total = mb * world          # the union minibatch's size under data parallelism
        total = self.flat.total
        losses = []
        for e in range(idx32.shape[0]):
            for j in range(idx32.shape[1]):
                mb_idx = idx32[e, j]
                N.check(grad_fn(
                    self.gru.h, self.flat.flat.data_ptr(), ctypes.byref(batch), mb_idx.data_ptr(),
                    mb, m_total, ctypes.byref(hp), self.flat.grad.data_ptr(), stream),
                    self._grad_entry)
                if world > 1:
                    torch.distributed.all_reduce(self.flat.grad)
                losses.append(self.flat.grad[total:total + 3].clone())
                step += 1
                clip_adam(self.flat, self.m, self.v, cfg, lr, step, stream)
        # {loss, policy, value, entropy} per minibatch (reference never logs these; for tests)
        sums = torch.stack(losses) / float(m_total)
        self.last_losses = torch.stack([sums[:, 0] + cfg.value_loss_weight * sums[:, 1]
                                        - cfg.entropy_beta * sums[:, 2], sums[:, 0], sums[:, 1],
                                        sums[:, 2]], dim=1)

    def train(self) -> None:
        world, rank = dist_world()   # per-rank env seeds, rank-0 checkpoints (as PPO.train)
        seed = self.cfg.seed
        if seed is not None and world > 1:
            seed = seed + rank * self.cfg.num_envs
        self.current_observations, _ = self.envs.reset(seed=seed)
        self.prev_dones = np.zeros(self.cfg.num_envs, dtype=bool)
        self.current_hx = torch.zeros(1, self.cfg.num_envs, self.cfg.gru_hidden_dim,
                                      device=self.device)
        last = time.time()
        total = self.cfg.total_steps // (self.cfg.rollout_steps * self.cfg.num_envs)
        env_steps = 0
        for i in range(total):
            self.learn(self.rollout())
            env_steps = (i + 1) * self.cfg.rollout_steps * self.cfg.num_envs
            if self.cfg.checkpoint and rank == 0 and time.time() - last >= self.cfg.save_interval:
                self.checkpointer.save(env_steps, self.network, self.optimizer)
                last = time.time()
        if self.cfg.checkpoint and rank == 0:
            self.checkpointer.save(env_steps, self.network, self.optimizer)
        self.envs.close()
