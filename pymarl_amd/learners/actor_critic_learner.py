"""ActorCriticLearner: epymarl's actor_critic_learner (configs maa2c.yaml / ia2c.yaml), MI355X-native, opt-in through
`learner: actor_critic_learner`. DESIGN.md §3k holds the specification it implements.

The critic is a V network (`critic_type`: `cv_critic` on the state, `ac_critic` on the agent's own obs) trained in ONE
optimiser step over every t against n-step returns of the target critic (`q_nstep`, `add_value_last_step`); the actor
is the GRU agent with a softmax policy (`agent_output_type: pi_logits`, `action_selector: soft_policies`, no epsilon
floor), trained with the advantage td = (return - V) mask and an entropy bonus (`entropy_coef`). All of train() is one
launch sequence of hand-written HIP kernels (include/ma_a2c.h, pymarl_amd/csrc/a2c_kernels.hpp); torch only owns the
buffers. There is no CPU path. One synchronisation per train(): the stats read-back that says whether the batch had a
live transition (an empty one changes nothing and counts nothing).

Keys: `lr` (both optimisers), `optimizer` (absent or `adam`: torch.optim.Adam with torch's defaults, read through
keys.optimizer_config; `rmsprop`: the reference's RMSprop), `grad_norm_clip`, `target_update_interval_or_tau`
(keys.target_update_config's rules counted in critic training steps; absent: a hard update every
`target_update_interval`, default 200, critic training steps), `standardise_rewards` (keys.reward_norm_config),
`hidden_dim` (the critic's width, 64 or 128), `mask_before_softmax` (default True). Refused with ValueError:
`use_rnn: False`, `learner_dp`, `standardise_returns: True`, `obs_individual_obs: True`, a critic_type other than the
two, and a PrioritizedReplayBuffer batch.
"""
from __future__ import annotations

import copy
import ctypes
from types import SimpleNamespace

import numpy as np
import torch as th
from torch.optim import Adam, RMSprop

from .. import _lib
from ..components.episode_buffer import is_per_batch, is_replay_view, replay_view
from ..modules.agents.rnn_agent import obs_dim, use_rnn_config
from ..modules.critics import REGISTRY as critic_REGISTRY
from ..modules.flat import link, load_state, pack, rebind, state_buffers, state_dict_own_steps, to_current_device
from .keys import (REW_MS_INIT, hard_target_update, load_rew_ms, optimizer_config, reward_norm_config, reward_stats,
                   save_rew_ms, target_update_config)

CRITIC_TYPES = ("cv_critic", "ac_critic")
A2C_STATS = list(_lib.A2C_STATS)


def gamma_table(gamma, q_nstep):
    """g[k] = float32(gamma ** k), k = 0 .. q_nstep + 1: the Python-float powers the n-step return multiplies with,
    each rounded to fp32 once."""
    return np.array([float(gamma) ** k for k in range(int(q_nstep) + 2)], dtype=np.float32)


def a2c_config(args):
    """The learner's own keys, checked: a namespace of critic_type, q_nstep, add_value_last_step, entropy_coef,
    mask_before_softmax, optimizer (name, Adam kwargs or None), target (mode, value), standardise_rewards."""
    ct = getattr(args, "critic_type", None)
    if ct not in CRITIC_TYPES:
        raise ValueError("critic_type {!r} not recognised (one of {}).".format(ct, ", ".join(CRITIC_TYPES)))
    if not use_rnn_config(args):
        raise ValueError("ActorCriticLearner does not support use_rnn: False (the feed-forward agent): its actor is "
                         "the GRU agent.")
    if getattr(args, "learner_dp", False):
        raise ValueError("learner_dp is not supported by ActorCriticLearner.")
    if getattr(args, "standardise_returns", False):
        raise ValueError("standardise_returns: True is not supported by ActorCriticLearner.")
    if getattr(args, "obs_individual_obs", False):
        raise ValueError("obs_individual_obs: True is not supported by ActorCriticLearner.")
    if getattr(args, "agent_output_type", "pi_logits") != "pi_logits":
        raise ValueError("ActorCriticLearner needs agent_output_type: pi_logits, got {!r}.".format(
            args.agent_output_type))
    n = getattr(args, "q_nstep", 5)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError("q_nstep must be an int >= 1, got {!r}.".format(n))
    ec = getattr(args, "entropy_coef", 0.01)
    if isinstance(ec, bool) or not isinstance(ec, (int, float, np.floating)) or not float(ec) >= 0.0:
        raise ValueError("entropy_coef must be a number >= 0, got {!r}.".format(ec))
    name = getattr(args, "optimizer", None)
    if name is None:   # epymarl's learner steps Adam: the absent key is adam here, not the Q learner's rmsprop
        name, kw = optimizer_config(SimpleNamespace(**dict(vars(args), optimizer="adam")))
    else:
        name, kw = optimizer_config(args)
    return SimpleNamespace(critic_type=ct, q_nstep=int(n),
                           add_value_last_step=bool(getattr(args, "add_value_last_step", True)),
                           entropy_coef=float(ec),
                           mask_before_softmax=bool(getattr(args, "mask_before_softmax", True)),
                           optimizer=(name, kw), target=target_update_config(args),
                           standardise_rewards=reward_norm_config(args))


def make_a2c_config(args, ac, input_dim, critic, max_batch, max_seq, gpow):
    cfg = _lib.MAConfig()
    cfg.n_agents = args.n_agents
    cfg.n_actions = args.n_actions
    cfg.obs_dim = obs_dim(args, input_dim)
    cfg.state_dim = critic.state_dim
    cfg.rnn_hidden_dim = 64
    cfg.critic_hidden = critic.hidden_dim
    cfg.critic_type = critic.KIND
    cfg.obs_last_action = int(bool(args.obs_last_action))
    cfg.obs_agent_id = int(bool(args.obs_agent_id))
    cfg.mask_before_softmax = int(ac.mask_before_softmax)
    cfg.q_nstep = ac.q_nstep
    cfg.add_value_last_step = int(ac.add_value_last_step)
    cfg.entropy_coef = ac.entropy_coef
    cfg.lr = args.lr
    cfg.optim_alpha = getattr(args, "optim_alpha", 0.99)
    cfg.optim_eps = getattr(args, "optim_eps", 1e-5)
    cfg.grad_norm_clip = args.grad_norm_clip
    cfg.gamma_pow = gpow.ctypes.data
    cfg.max_batch = int(max_batch)
    cfg.max_seq = int(max_seq)
    return cfg


class ActorCriticLearner:
    def __init__(self, mac, scheme, logger, args):
        self.args = args
        self.cfg = a2c_config(args)
        self.n_agents = args.n_agents
        self.n_actions = args.n_actions
        self.mac = mac
        self.logger = logger
        self.last_target_update_step = 0
        self.critic_training_steps = 0
        self.log_stats_t = -self.args.learner_log_interval - 1
        self.critic = critic_REGISTRY[self.cfg.critic_type](scheme, args)
        self.target_critic = copy.deepcopy(self.critic)
        self.agent_params = list(mac.parameters())
        self.critic_params = list(self.critic.parameters())
        self.params = self.agent_params + self.critic_params
        self.optim_name, adam_kw = self.cfg.optimizer
        if adam_kw is None:
            mk = lambda ps: RMSprop(params=ps, lr=args.lr, alpha=getattr(args, "optim_alpha", 0.99),   # noqa: E731
                                    eps=getattr(args, "optim_eps", 1e-5))
        else:
            mk = lambda ps: Adam(params=ps, **adam_kw)   # noqa: E731
        self.agent_optimiser = mk(self.agent_params)
        self.critic_optimiser = mk(self.critic_params)
        self.target_mode, self.target_value = self.cfg.target
        self.standardise_rewards = self.cfg.standardise_rewards
        self._gpow = gamma_table(args.gamma, self.cfg.q_nstep)
        dev = self.mac.agent.fc1.weight.device
        self._agent, self.n_agent_params = pack([self.mac.agent], device=dev)
        self._critic, self.n_critic_params = pack([self.critic], device=dev)
        self._tcritic, _ = pack([self.target_critic], device=dev)
        self.rew_ms = th.tensor(REW_MS_INIT, dtype=th.float64, device=dev) if self.standardise_rewards else None
        self._opt_steps = 0
        self._alloc_state(dev)
        self._handle = None
        self._handle_key = None
        self._last = None

    # -- buffers ---------------------------------------------------------------------------------------------
    def _alloc_state(self, dev):
        Pa, Pc = self.n_agent_params, self.n_critic_params
        z = lambda n: th.zeros(n, dtype=th.float32, device=dev)   # noqa: E731
        self._agrad, self._asq = z(Pa + _lib.NSUMS), z(Pa)
        self._cgrad, self._csq = z(Pc + _lib.MA_NTAIL), z(Pc)
        adam = self.optim_name == "adam"
        self._am, self._cm = (z(Pa), z(Pc)) if adam else (None, None)   # Adam's exp_avg; exp_avg_sq lives in _asq / _csq
        self._stats = z(_lib.MA_NSTATS)
        self._relink()

    def _relink(self):
        """Point module params, .grad and both optimisers' state at the flat buffers."""
        rebind([self.mac.agent], self._agent)
        rebind([self.critic], self._critic)
        rebind([self.target_critic], self._tcritic)
        self.mac.agent._flat = self._agent
        self.critic._flat = self._critic
        self.target_critic._flat = self._tcritic
        self._step_t = th.tensor(float(self._opt_steps))   # one counter shared by every parameter of both optimisers
        for params, grad, sq, m, opt in ((self.agent_params, self._agrad, self._asq, self._am, self.agent_optimiser),
                                         (self.critic_params, self._cgrad, self._csq, self._cm, self.critic_optimiser)):
            link(params, opt, grad, dict(step=self._step_t, **state_buffers(self.optim_name, sq, m)))
        self._handle = None

    def _get_handle(self, batch):
        T = batch.source.max_seq_length if is_replay_view(batch) else batch.max_seq_length
        need_b = max(batch.batch_size, getattr(self.args, "batch_size", 1))
        if self._handle is None or self._handle_key[0] < need_b or self._handle_key[1] < T:
            cfg = make_a2c_config(self.args, self.cfg, self.mac.agent.input_dim, self.critic, need_b, T, self._gpow)
            h = _lib.A2CHandle(cfg)
            if h.agent_offsets[-1] != self.n_agent_params or h.critic_offsets[-1] != self.n_critic_params:
                raise _lib.MQError("parameter layout mismatch: library ({}, {}) vs modules ({}, {})".format(
                    h.agent_offsets[-1], h.critic_offsets[-1], self.n_agent_params, self.n_critic_params))
            P = _lib.ptr
            _lib.check(h.lib.ma_bind(h.h, P(self._agent), P(self._agrad), P(self._asq), P(self._critic),
                                     P(self._tcritic), P(self._cgrad), P(self._csq), P(self._stats)))
            if self.optim_name == "adam":
                g = self.agent_optimiser.param_groups[0]
                ad = _lib.MAAdam(agent_exp_avg=self._am.data_ptr(), critic_exp_avg=self._cm.data_ptr(),
                                 beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], weight_decay=g["weight_decay"])
                _lib.check(h.lib.ma_set_adam(h.h, ctypes.byref(ad)))
            if self.rew_ms is not None:
                _lib.check(h.lib.ma_set_reward_norm(h.h, _lib.ptr(self.rew_ms)))
            self._handle, self._handle_key = h, (need_b, T)
        return self._handle

    # -- reference API ---------------------------------------------------------------------------------------
    def train(self, batch, t_env: int, episode_num: int):
        if is_per_batch(batch):
            raise ValueError("ActorCriticLearner is on-policy and does not take a PrioritizedReplayBuffer batch: its "
                             "loss carries no importance weights and it writes no priorities back")
        _lib.require_gpu(self._agent)
        h = self._get_handle(batch)
        rep, keep = replay_view(batch)
        _lib.check(h.lib.ma_train_step(h.h, ctypes.byref(rep), self._opt_steps + 1, _lib.stream_ptr()))
        del keep
        st = self._stats.tolist()   # the one synchronisation per train()
        self._last_batch = (batch.batch_size, rep.t_len)
        self._last = {k: st[i] for k, i in _lib.A2C_STATS.items()}
        self._last["mask_elems"] = st[_lib.A2C_MASK_ELEMS]
        if not st[_lib.A2C_MASK_ELEMS] > 0.0:
            return   # an empty batch: nothing was applied, nothing is counted
        self._opt_steps += 1
        self._step_t += 1
        self.critic_training_steps += 1
        self._target_schedule()

        if t_env - self.log_stats_t >= self.args.learner_log_interval:
            for key in A2C_STATS:
                self.logger.log_stat(key, self._last[key], t_env)
            self.log_stats_t = t_env

    def _target_schedule(self):
        """After both optimiser steps: soft, or hard when due, counted in critic training steps."""
        if self.target_mode == "soft":
            self._update_targets_soft(self.target_value)
            return
        every = self.target_value if self.target_mode == "hard" else getattr(self.args, "target_update_interval", 200)
        if (self.critic_training_steps - self.last_target_update_step) / every >= 1.0:
            self._update_targets()
            self.last_target_update_step = self.critic_training_steps

    def _update_targets_soft(self, tau):
        """target = target (1 - tau) + critic tau (soft_update_kernel; tau = 1 is the copy)."""
        _lib.check(self._handle.lib.ma_update_targets(self._handle.h, float(tau), _lib.stream_ptr()))

    def _update_targets(self):
        hard_target_update(self._handle, "ma_update_targets", self._tcritic, self._critic, self.logger, 0.0)

    def cuda(self):
        to_current_device(self, ("_agent", "_critic", "_tcritic", "_agrad", "_asq", "_cgrad", "_csq", "_am", "_cm",
                                 "_stats", "rew_ms"))
        self._relink()

    def reward_stats(self):
        """The running reward statistics as a dict of Python floats: mean, var, count (synchronises)."""
        return reward_stats(self.rew_ms)

    def save_models(self, path):
        self.mac.save_models(path)
        th.save(self.critic.state_dict(), "{}/critic.th".format(path))
        for fname, opt in (("agent_opt.th", self.agent_optimiser), ("critic_opt.th", self.critic_optimiser)):
            th.save(state_dict_own_steps(opt), "{}/{}".format(path, fname))
        save_rew_ms(self.rew_ms, path)

    def load_models(self, path):
        ml = lambda s, loc: s  # noqa: E731
        self.mac.load_models(path)
        self.critic.load_state_dict(th.load("{}/critic.th".format(path), map_location=ml, weights_only=True))
        # the target critic is not saved (as the COMA learner): it restarts from the critic
        self.target_critic.load_state_dict(self.critic.state_dict())
        steps = []
        for fname, opt, params, sq, m in (("agent_opt.th", self.agent_optimiser, self.agent_params, self._asq, self._am),
                                          ("critic_opt.th", self.critic_optimiser, self.critic_params, self._csq,
                                           self._cm)):
            sd = th.load("{}/{}".format(path, fname), map_location=ml, weights_only=True)
            steps.append(load_state(opt, sd, params, state_buffers(self.optim_name, sq, m), expect=self.optim_name,
                                    what="{}/{}".format(path, fname)))
        self._opt_steps = next((n for n in steps if n is not None), 0)
        load_rew_ms(self.rew_ms, path, self.logger)
        self._relink()

    # -- extras (parity / diagnostics) -----------------------------------------------------------------------
    def last_stats(self):
        return dict(self._last)

    def last_plan(self):
        """What the last train() launched (ma_last_plan): rows, k / kp, split-K slices, blocks per launch."""
        pl = _lib.MAPlan()
        _lib.check(self._handle.lib.ma_last_plan(self._handle.h, ctypes.byref(pl)))
        return pl.as_dict()

    def last_intermediate(self, which):
        """0: V' (B, T+1, n); 1: V (B, T, n); 2: the n-step returns (B, T, n); 3: pi (B, T, n, A); 4: dLoss/dlogits
        before the 1 / M scale, (B, T, n, A)."""
        B, Tp = self._last_batch
        T, n, A = Tp - 1, self.n_agents, self.n_actions
        out = self._handle.copy_intermediate(which, self._agent.device)
        if which == 0:
            return out.view(Tp, B, n).permute(1, 0, 2)
        if which in (1, 2):
            return out.view(T, B, n).permute(1, 0, 2)
        if which == 3:
            return out.view(T, B, n, A).permute(1, 0, 2, 3)
        return out.view(T, B, n, -1)[..., :A].permute(1, 0, 2, 3)
