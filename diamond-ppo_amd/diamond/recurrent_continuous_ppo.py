"""RecurrentContinuousPPO -- RecurrentPPO's GRU agent with ContinuousPPO's Gaussian policy.

The reference has no recurrent Gaussian agent.  This one puts the head of reference
``diamond/continuous_ppo.py`` (``JointNormal`` :40-47, a mean head and a state-independent
``actor_log_std`` parameter :50-111, init without the 0.01 output scaling :114-121, the loss of
:276-292) on the recurrent network of ``diamond/recurrent_ppo.py`` (:94-149, intended semantics as
``diamond/recurrent_ppo.py`` here restates them).  Everything but the head is ``RecurrentPPO``'s:
the rollout's experience rows, GAE, advantage normalisation, the minibatch split, the data-parallel
semantics and the four class flags.  For the default network at a shape ``fused_gru_shape``
admits (``act_dim`` = action dimensions), learn()'s minibatches run as one
``dppo_gru_gauss_minibatch_grad_f32`` launch each and, with ``fused_rollout``, every env step as
one ``dppo_gru_gauss_act_f32`` and one ``dppo_gru_value_f32`` launch; otherwise the network runs
under torch autograd with ``torch_ppo_terms(..., continuous=True)``.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Any, Callable

import numpy as np
import torch
import torch.nn as nn

from . import _native as N
from ._spaces import is_box
from .continuous_ppo import JointNormal
from .recurrent_ppo import CORE_SCAN_CALLS, GRUCore, RecurrentPPO, RecurrentPPOConfig, \
    fused_gru_shape


@dataclass
class RecurrentContinuousPPOConfig(RecurrentPPOConfig):
    """RecurrentPPOConfig's fields, order and defaults."""


class RecurrentContinuousActorCriticNetwork(nn.Module):
    def __init__(self, observation_space, action_space, cfg: RecurrentPPOConfig) -> None:
        super().__init__()
        assert is_box(observation_space), "Only Box obs spaces are supported."
        assert is_box(action_space), "Only Box action spaces are supported."
        hd, gd = cfg.network_hidden_dim, cfg.gru_hidden_dim
        act_dim = int(np.prod(action_space.shape))
        # a direct parameter, registered first: the first entry of named_parameters()
        # (continuous_ppo.py:95) and tensor 0 of the flat layout
        self.actor_log_std = nn.Parameter(torch.zeros(1, act_dim))
        self.base = nn.Sequential(nn.Linear(int(np.prod(observation_space.shape)), hd), nn.Tanh())
        self.gru = GRUCore(hd, gd)
        self.actor_mean_head = nn.Sequential(nn.Linear(gd, hd), nn.Tanh(), nn.Linear(hd, act_dim))
        self.critic_head = nn.Sequential(nn.Linear(gd, hd), nn.Tanh(), nn.Linear(hd, 1))

    def get_values(self, observations, hx, dones):
        x = self.base(observations)
        x, hx = self.gru.forward(x, hx, dones)
        return self.critic_head(x).squeeze(-1)

    def get_means_log_stds_values_and_hx(self, observations, hx, dones):
        x = self.base(observations)
        x, hx = self.gru.forward(x, hx, dones)
        mean = self.actor_mean_head(x)
        log_std = torch.broadcast_to(self.actor_log_std, mean.shape)
        return mean, log_std, self.critic_head(x).squeeze(-1), hx


class RecurrentContinuousPPO(RecurrentPPO):
    # fused_gru, fused_rollout, fused_loss and fused_core: RecurrentPPO's, with the Gaussian
    # kernels (dppo_gru_gauss_minibatch_grad_f32, dppo_gru_gauss_act_f32) behind the first two
    continuous = True
    _grad_entry = "dppo_gru_gauss_minibatch_grad_f32"
    _batch_struct = N.GruGaussBatch
    _action_dtype = torch.float32

    def __init__(self, env_fn: Callable[[], Any],
                 cfg: RecurrentPPOConfig = RecurrentContinuousPPOConfig(),
                 network_cls: Any = RecurrentContinuousActorCriticNetwork, envs=None) -> None:
        # RecurrentPPO builds everything but the fused workspace: its own is for the categorical
        # network alone.  Its init is continuous_ppo.network_parameter_init_ for a network
        # without an actor_out_layer: orthogonal sqrt(2), zero biases, no 0.01 output scaling
        super().__init__(env_fn, cfg, network_cls, envs)
        obs_space, act_space = self.envs.single_observation_space, self.envs.single_action_space
        assert is_box(act_space), "Only Box action spaces are supported."
        obs_dim = int(np.prod(obs_space.shape))
        self.act_dim = int(np.prod(act_space.shape))
        wide_obs = bool(getattr(cfg, "wide_observations", False))
        if (type(self.network) is RecurrentContinuousActorCriticNetwork
                and fused_gru_shape(cfg.network_hidden_dim, cfg.gru_hidden_dim, obs_dim,
                                    self.act_dim, wide_obs)):
            gd = N.GruDims(rollout_steps=cfg.rollout_steps, num_envs=cfg.num_envs,
                           obs_dim=obs_dim, act_dim=self.act_dim, hidden=64,
                           gru_hidden=cfg.gru_hidden_dim, wide_obs=int(wide_obs))
            self.gru = N.GruHandle(self.device.index or 0, gd, gauss=True)
            L = self.gru.layout
            if L.total != self.flat.total or any(L.offset[i] != o for i, o in
                                                  enumerate(self.flat.offsets)):
                raise RuntimeError(
                    "RecurrentContinuousActorCriticNetwork layout differs from libdppo's")

    def _policy_terms(self, observations, hx, prev_dones):
        mean, log_std, nv, _ = self.network.get_means_log_stds_values_and_hx(observations, hx,
                                                                              prev_dones)
        return mean, log_std, nv

    def rollout(self):
        """RecurrentPPO.rollout with a JointNormal draw (continuous_ppo.py:100-105); the envs
        receive the float32 actions."""
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
                mean, log_std, values, new_hx = self.network.get_means_log_stds_values_and_hx(
                    obs_t, hx, pd_t)
                # inside the mode: log_std is a view of the parameter and would carry a graph
                dist = JointNormal(loc=mean.squeeze(0), scale=log_std.squeeze(0).exp())
                actions = dist.sample()
                log_probs = dist.log_prob(actions)
            next_observations, rewards, terms, truncs, infos = self.envs.step(
                actions.cpu().numpy().astype(np.float32, copy=False))
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
        """RecurrentPPO._rollout_fused with dppo_gru_gauss_act_f32 as the policy step: the same
        staging, Philox key and counter scheme; the float32 actions [N, A] come down."""
        cfg, dev, lib = self.cfg, self.device, self.gru.lib
        T, Nn, G = cfg.rollout_steps, cfg.num_envs, cfg.gru_hidden_dim
        D, A = self.gru.dims.obs_dim, self.gru.dims.act_dim
        st = self._rollout_staging
        if st is None:
            pin = lambda shape, dt: torch.empty(shape, dtype=dt).pin_memory()
            st = self._rollout_staging = {
                "obs": pin((Nn, D), torch.float32), "dones": pin((Nn,), torch.bool),
                "nobs": pin((Nn, D), torch.float32), "act": pin((Nn, A), torch.float32),
                "nobs_d": torch.empty((Nn, D), dtype=torch.float32, device=dev)}
            for k in ("obs", "dones", "nobs", "act"):
                st[k + "_np"] = st[k].numpy()
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        obs_d, hx_d = f32(T, Nn, D), f32(T + 1, 1, Nn, G)
        lp_d, v_d, nv_d = f32(T, Nn), f32(T, Nn), f32(T, Nn)
        pd_d = torch.empty((T, Nn), dtype=torch.bool, device=dev)
        act_d = f32(T, Nn, A)
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
            step = N.GruGaussStep(obs_d[t].data_ptr(), pd_d[t].data_ptr(), hx_d[t].data_ptr(),
                                  hx_d[t + 1].data_ptr(), act_d[t].data_ptr(),
                                  lp_d[t].data_ptr(), v_d[t].data_ptr(), None)
            N.check(lib.dppo_gru_gauss_act_f32(self.gru.h, params, ctypes.byref(step), Nn,
                                               self._act_seed, self._act_counter,
                                               stream.cuda_stream), "dppo_gru_gauss_act_f32")
            self._act_counter += 1
            st["act"].copy_(act_d[t], non_blocking=True)
            stream.synchronize()
            next_observations, rewards, terms, truncs, infos = self.envs.step(
                st["act_np"].copy())
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
        self.current_observations, self.prev_dones = observations, prev_dones
        self.current_hx = hx_d[T]
        return [[obs_d[t], act_d[t], *host[t], pd_d[t], lp_d[t], v_d[t], nv_d[t], hx_d[t]]
                for t in range(T)]
