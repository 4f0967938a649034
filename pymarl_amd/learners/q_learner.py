"""QLearner: QMIX / VDN / IQL learner (reference: src/learners/q_learner.py:9-143), MI355X-native.

Same constructor, `train(batch, t_env, episode_num)`, `_update_targets`, `cuda`, `save_models`, `load_models`,
the five logged stats and the episode-counted hard target update. The whole of train() — replay gather,
both GRU unrolls, double-Q selection, mixer, masked L2 TD loss, BPTT, clip_grad_norm_, RMSprop — is one
launch sequence of hand-written HIP kernels in libmq_learner.so (include/mq_learner.h); torch only owns the
device buffers. There is no CPU path: a learner that is not on a HIP device raises.

Opt-in `optimizer: adam` (pymarl2's key; `weight_decay`, `adam_betas`, `adam_eps`): the step's last launch is then
torch.optim.Adam's update (apply_adam_kernel, mq_set_adam) and `self.optimiser` a real torch.optim.Adam whose exp_avg /
exp_avg_sq are views into two flat buffers, so opt.th has torch's format both ways. Without the key nothing changes.

Opt-in epymarl keys (target_update_config, reward_norm_config): `target_update_interval_or_tau` above 1 is a hard target
update counted in training steps, at most 1 a Polyak update after every step (soft_update_kernel, mq_set_soft_target:
the step's last launch); `standardise_rewards: True` standardises the rewards with running statistics kept on the
device (`self.rew_ms`, reward_norm_kernel, mq_set_reward_norm) before the target is formed. Without the keys nothing
changes.

Opt-in `use_rnn: False` (epymarl's key, modules/agents/rnn_agent.py): the agent's `rnn` is a Linear + ReLU, and the
step runs the feed-forward agent's GEMM chain in the recurrence's place (ffn_kernels.hpp, mq_config.agent);
`last_agent()` says which agent the last step ran. Without the key nothing changes.

Data parallel: with `args.learner_dp = True` and torch.distributed initialised (RCCL, one process
per GPU), every rank calls train() with the SAME GLOBAL sample, as run.py:207-219 does unchanged (ranks share the
seed, so the sampled ids agree; ids and contents checked on a call-count schedule, `args.learner_dp_check`); the
learner trains its own contiguous shard
of the episodes (dp.local_shard), the unnormalised gradient buffer (+ the loss/mask sums in its tail) is summed with
ONE all_reduce, and every rank then applies the identical normalised update. Under an RCCL process group the learner
borrows the process's library communicator (dp.SharedComm: mq_comm_create once, mq_comm_use per handle): the
all-reduce is then issued inside mq_forward_backward, in stream order, and a train step makes no Python call between
its kernels. Other backends (gloo) all-reduce from Python (dp.py).
"""
from __future__ import annotations

import copy
import ctypes
import os

import torch as th
from torch.optim import Adam, RMSprop

from .. import _lib
from ..components.episode_buffer import (_FIELDS, PrioritizedBatch, _field_view, is_per_batch,  # noqa: F401
                                         is_replay_view, replay_view)
from ..modules.agents.rnn_agent import Q_TARGETS, make_config  # noqa: F401
from ..modules.flat import link, load_state, pack, rebind, state_buffers, state_dict_own_steps, to_current_device
from .dp import (DPCheck, SharedComm, allreduce_grad_buffer, dp_active, dp_collective, dp_world, local_shard,
                 native_comm_wanted)
from .keys import (OPTIMIZERS, REW_MS_INIT, hard_target_update, load_rew_ms, optimizer_config,  # noqa: F401
                   reward_norm_config, reward_stats, save_rew_ms, target_update_config)
from ..modules.mixers.qmix import QMixer
from ..modules.mixers.vdn import VDNMixer

MIXER_IDS = {None: _lib.MIXER_NONE, "vdn": _lib.MIXER_VDN, "qmix": _lib.MIXER_QMIX}


class QLearner:
    def __init__(self, mac, scheme, logger, args):
        self.args = args
        self.mac = mac
        self.logger = logger
        self.params = list(mac.parameters())
        self.last_target_update_episode = 0
        # epymarl's keys, both opt-ins: the target schedule in training steps (or soft), and reward standardisation
        self.target_mode, self.target_value = target_update_config(args)
        self.standardise_rewards = reward_norm_config(args)
        self.training_steps = 0
        self.last_target_update_step = 0
        self.mixer = None
        if args.mixer is not None:
            if args.mixer == "vdn":
                self.mixer = VDNMixer()
            elif args.mixer == "qmix":
                self.mixer = QMixer(args)
            else:
                raise ValueError("Mixer {} not recognised.".format(args.mixer))
            self.params += list(self.mixer.parameters())
            self.target_mixer = copy.deepcopy(self.mixer)
        # optimizer: adam is an opt-in (optimizer_config); without the key this is the reference's line
        self.optim_name, adam_kw = optimizer_config(args)
        if adam_kw is None:
            self.optimiser = RMSprop(params=self.params, lr=args.lr, alpha=args.optim_alpha, eps=args.optim_eps)
        else:
            self.optimiser = Adam(params=self.params, **adam_kw)
        self.target_mac = copy.deepcopy(mac)
        self.log_stats_t = -self.args.learner_log_interval - 1
        self.dp = bool(getattr(args, "learner_dp", False))
        # when to check that the ranks passed the same global sample (ids AND contents): a call-count schedule, the
        # same on every rank (dp.DPCheck: "first", "always", "off" or every N calls, default 100)
        self.dp_check = DPCheck(getattr(args, "learner_dp_check", None))
        # the mixer's double-Q selection reads the replay buffer's avail bitmask (False: the int32 avail_actions rows;
        # bitwise the same result, test_avail_bits_bitwise)
        self.use_avail_bits = bool(getattr(args, "learner_avail_bits", True))

        # flat device buffers: [agent params | mixer params] for online and target nets (MQ_P_* order)
        self._mods = [m for m in (self.mac.agent, self.mixer) if m is not None and len(list(m.parameters()))]
        self._tmods = [m for m in (self.target_mac.agent, getattr(self, "target_mixer", None))
                       if m is not None and len(list(m.parameters()))]
        dev = self.mac.agent.fc1.weight.device
        self._online, self.n_params = pack(self._mods, device=dev)
        self._target, _ = pack(self._tmods, device=dev)
        # the running reward statistics [mean, var, count]: float64 on the device, never read by a step
        self.rew_ms = th.tensor(REW_MS_INIT, dtype=th.float64, device=dev) if self.standardise_rewards else None
        self._alloc_state(dev)
        self._handle = None
        self._handle_key = None
        self._opt_steps = 0

    # -- buffers ---------------------------------------------------------------------------------------------
    def _alloc_state(self, dev):
        P = self.n_params
        self._grad = th.zeros(P + _lib.NSUMS, dtype=th.float32, device=dev)
        self._sq = th.zeros(P, dtype=th.float32, device=dev)
        # Adam's first moment (exp_avg); its second (exp_avg_sq) lives in _sq, where RMSprop's square_avg does
        self._m = th.zeros(P, dtype=th.float32, device=dev) if self.optim_name == "adam" else None
        self._stats = th.zeros(_lib.NSTATS, dtype=th.float32, device=dev)
        self._curmax = None
        self._relink()

    def _relink(self):
        """Point module params, .grad and the optimiser's square_avg (Adam: exp_avg, exp_avg_sq) at the flat buffers."""
        Pa = sum(p.numel() for p in self.mac.agent.parameters())
        rebind(self._mods, self._online)
        rebind(self._tmods, self._target)
        self.mac.agent._flat = self._online[:Pa]
        self.target_mac.agent._flat = self._target[:Pa]
        if self.mixer is not None and hasattr(self.mixer, "_flat"):
            self.mixer._flat = self._online[Pa:self.n_params]
            self.target_mixer._flat = self._target[Pa:self.n_params]
        # one shared step counter: train() increments it once, not once per parameter
        self._step_t = th.tensor(float(getattr(self, "_opt_steps", 0)))
        bufs = state_buffers(self.optim_name, self._sq, self._m)
        # where each optimiser's state has had its step here: Adam's first (torch's order), RMSprop's last
        link(self.params, self.optimiser, self._grad,
             dict(step=self._step_t, **bufs) if self.optim_name == "adam" else dict(bufs, step=self._step_t))
        self._handle = None

    _dp_active, collective = dp_active, dp_collective

    def _local_batch(self, batch):
        """Data parallel: this rank's shard of the global sample (dp.local_shard), the ranks' agreement checked per
        `self.dp_check`."""
        rank, world = dp_world()
        check = self.dp_check.due()
        out = local_shard(batch, rank, world, check=check, device=self._online.device)
        self.dp_check.done += int(check)
        return out

    def _get_handle(self, batch):
        T = batch.source.max_seq_length if is_replay_view(batch) else batch.max_seq_length
        world = dp_world()[1] if self._dp_active() else 1
        need_b = max(batch.batch_size, -(-getattr(self.args, "batch_size", 1) // world))
        key = (need_b, T)
        if SharedComm.stale(self._handle):
            self._handle = None   # its communicator was freed (SharedComm.free detached it): rebuild and re-attach
        if self._handle is None or self._handle_key[0] < need_b or self._handle_key[1] < T:
            cfg = make_config(self.args, MIXER_IDS[self.args.mixer], input_dim=self.mac.agent.input_dim,
                              max_batch=need_b, max_seq=T)
            h = _lib.Handle(cfg)
            Tmax = T
            self._curmax = th.zeros(Tmax * need_b * self.args.n_agents, dtype=th.int32, device=self._online.device)
            _lib.check(h.lib.mq_bind(h.h, _lib.ptr(self._online), _lib.ptr(self._target), _lib.ptr(self._grad),
                                     _lib.ptr(self._sq), _lib.ptr(self._stats), _lib.ptr(self._curmax)))
            if getattr(self, "optim_name", "rmsprop") == "adam":
                # with the CURRENT step count: a handle rebuilt for a larger batch must not restart the bias correction
                g = self.optimiser.param_groups[0]
                ad = _lib.MQAdam(exp_avg=self._m.data_ptr(), beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"],
                                 weight_decay=g["weight_decay"], step=self._opt_steps)
                _lib.check(h.lib.mq_set_adam(h.h, ctypes.byref(ad)))
            # sticky per handle, so a handle rebuilt for a larger batch gets them again (the statistics are the
            # learner's tensor: they carry over)
            if getattr(self, "target_mode", None) == "soft":
                _lib.check(h.lib.mq_set_soft_target(h.h, self.target_value))
            if getattr(self, "rew_ms", None) is not None:
                _lib.check(h.lib.mq_set_reward_norm(h.h, _lib.ptr(self.rew_ms)))
            h.dp_on = False
            h.native = False
            if self._dp_active() and native_comm_wanted(self._online.device):
                # the process's communicator, created once (a handle rebuilt later needs no collective to attach)
                SharedComm.lend(h, "mq_comm_use", "mq_comm_detach", self._online.device)
            if h.n_params != self.n_params:
                raise _lib.MQError("parameter layout mismatch: library {} vs modules {}".format(h.n_params,
                                                                                              self.n_params))
            self._handle, self._handle_key = h, key
        return self._handle

    # -- reference API ---------------------------------------------------------------------------------------
    def train(self, batch, t_env: int, episode_num: int):
        _lib.require_gpu(self._online)
        # decided per call: torch.distributed may be initialised after the handle was created; mq_apply must then
        # recompute the gradient norm from the all-reduced buffer
        dp = self._dp_active()
        per = is_per_batch(batch)
        if per and (self.dp or getattr(self, "force_dp_norm", False)):
            raise ValueError("learner_dp is not supported with a PrioritizedReplayBuffer batch: the priorities and "
                             "importance weights belong to one device's buffer")
        if getattr(self, "rew_ms", None) is not None and (self.dp or getattr(self, "force_dp_norm", False)):
            raise ValueError("learner_dp is not supported with standardise_rewards: the running reward statistics "
                             "belong to one device's batches, and each rank would see only its shard")
        if dp:
            batch = self._local_batch(batch)
        h = self._get_handle(batch)
        want = dp or getattr(self, "force_dp_norm", False)
        if want != h.dp_on:
            _lib.check(h.lib.mq_set_data_parallel(h.h, int(want)))
            h.dp_on = want
        rep, keep = replay_view(batch, self.use_avail_bits)
        lib, s = h.lib, _lib.stream_ptr()
        if per:
            # weighted loss, then the new priorities into the buffer: armed for this step only (mq_set_per)
            src = batch.source
            pr = _lib.MQPer(weights=batch.weights.data_ptr(), prio=src.prio.data_ptr(),
                            prio_max=src.prio_max.data_ptr(), n_prio=src.prio.numel(), eps=src.eps)
            keep.append(batch.weights)
            _lib.check(lib.mq_set_per(h.h, ctypes.byref(pr)))
        if dp and not h.native:
            _lib.check(lib.mq_forward_backward(h.h, ctypes.byref(rep), s))
            allreduce_grad_buffer(self._grad)
            _lib.check(lib.mq_apply(h.h, s))
        else:
            # one call: mq_forward_backward (+ the native all-reduce when attached) and mq_apply
            _lib.check(lib.mq_train_step(h.h, ctypes.byref(rep), s))
        self._opt_steps += 1
        self._step_t += 1   # every parameter's optimiser state holds this tensor (see save_models)
        self._last_batch = (batch.batch_size, rep.t_len)
        del keep

        self._target_schedule(episode_num)

        if t_env - self.log_stats_t >= self.args.learner_log_interval:
            st = self._stats.tolist()
            self.logger.log_stat("loss", st[0], t_env)
            self.logger.log_stat("grad_norm", st[1], t_env)
            self.logger.log_stat("td_error_abs", st[2], t_env)
            self.logger.log_stat("q_taken_mean", st[3], t_env)
            self.logger.log_stat("target_mean", st[4], t_env)
            self.log_stats_t = t_env

    def _target_schedule(self, episode_num):
        """After the optimiser step of every train(): count it, then the hard target update when it is due."""
        self.training_steps += 1
        if self.target_mode is None:
            if (episode_num - self.last_target_update_episode) / self.args.target_update_interval >= 1.0:
                self._update_targets()
                self.last_target_update_episode = episode_num
        elif self.target_mode == "hard":
            # epymarl's schedule: counted in training steps; target_update_interval is ignored
            if (self.training_steps - self.last_target_update_step) / self.target_value >= 1.0:
                self._update_targets()
                self.last_target_update_step = self.training_steps
        # "soft": the step's last launch already moved the targets (mq_set_soft_target); nothing to do or to print

    def _update_targets(self):
        hard_target_update(self._handle, "mq_update_targets", self._target, self._online, self.logger)

    def cuda(self):
        to_current_device(self, ("_online", "_target", "_grad", "_sq", "_m", "_stats", "rew_ms"))
        self._relink()

    def reward_stats(self):
        """The running reward statistics as a dict of Python floats: mean, var, count (synchronises)."""
        return reward_stats(self.rew_ms)

    def save_models(self, path):
        self.mac.save_models(path)
        if self.mixer is not None:
            th.save(self.mixer.state_dict(), "{}/mixer.th".format(path))
        th.save(state_dict_own_steps(self.optimiser), "{}/opt.th".format(path))
        # the epymarl keys' state, as plain dicts of Python numbers: the running reward statistics, and the counters
        # of the step-counted target schedule
        save_rew_ms(self.rew_ms, path)
        if self.target_mode is not None:
            th.save(dict(training_steps=int(self.training_steps),
                         last_target_update_step=int(self.last_target_update_step)),
                    "{}/target_update.th".format(path))

    def load_models(self, path):
        self.mac.load_models(path)
        # Not quite right but I don't want to save target networks (reference comment, q_learner.py:139)
        self.target_mac.load_models(path)
        ml = lambda s, loc: s  # noqa: E731
        if self.mixer is not None:
            self.mixer.load_state_dict(th.load("{}/mixer.th".format(path), map_location=ml, weights_only=True))
        sd = th.load("{}/opt.th".format(path), map_location=ml, weights_only=True)
        # load_state_dict replaces the state tensors: copied back into the flat buffers, and re-linked below
        self._opt_steps = load_state(self.optimiser, sd, self.params, state_buffers(self.optim_name, self._sq, self._m),
                                     expect=self.optim_name, what="{}/opt.th".format(path),
                                     names={"adam": "Adam", "rmsprop": "RMSprop"}.get) or 0
        load_rew_ms(self.rew_ms, path, self.logger)
        if self.target_mode is not None:
            f = "{}/target_update.th".format(path)
            if os.path.exists(f):
                tu = th.load(f, map_location=ml, weights_only=True)
                self.training_steps = int(tu["training_steps"])
                self.last_target_update_step = int(tu["last_target_update_step"])
        self._relink()

    # -- extras (parity / diagnostics) -----------------------------------------------------------------------
    def last_stats(self):
        """dict of the last step's stats (loss, grad_norm, td_error_abs, q_taken_mean, target_mean, mask_sum)."""
        st = self._stats.tolist()
        return dict(loss=st[0], grad_norm=st[1], td_error_abs=st[2], q_taken_mean=st[3], target_mean=st[4],
                    mask_sum=st[5])

    def last_plan(self):
        """Kernel variants the last train() launched (mq_last_plan): rows, fused_fwd, rw_fwd, fused_bwd, rw_bwd,
        inline_ids, hyper, mix, tiles, dwh (where QMIX's dW_hyper ran: "red1" or "bptt_grid"), td_lambda (1: the
        mixer tail ran as the TD(lambda) passes), bwd_lean (1: the fused BPTT ran its lean per-step path), per (1: a
        prioritized-replay step: weighted loss, then the priority write-back), hyper_layers (2: the two-layer QMIX
        hypernet ran as launches of its own, 1: the one-layer hypernet, 0: no QMIX mixer), reward_norm (1: the step
        standardised its rewards, standardise_rewards), soft_target (1: the step ended with the soft target update)."""
        pl = _lib.MQPlan()
        _lib.check(self._handle.lib.mq_last_plan(self._handle.h, ctypes.byref(pl)))
        d = pl.as_dict()
        d["hyper_layers"] = int(self._handle.lib.mq_last_hyper_layers(self._handle.h))   # an entry of its own
        d["reward_norm"] = int(self._handle.lib.mq_last_reward_norm(self._handle.h))
        d["soft_target"] = int(self._handle.lib.mq_last_soft_target(self._handle.h))
        d["hyper"] = _lib.HYP_NAMES[d["hyper"]]
        d["mix"] = _lib.MIX_NAMES[d["mix"]]
        d["dwh"] = ("red1", "bptt_grid")[d["dwh"]]
        return d

    def last_agent(self):
        """mq_last_agent of the last train(): 0 when the GRU agent ran; otherwise a bit set, bit 0 = the feed-forward
        agent (use_rnn: False) ran, bits 1 / 2 = its forward / backward was a fused kernel (never set: the step runs
        the GEMM chain)."""
        return int(self._handle.lib.mq_last_agent(self._handle.h))

    def last_cur_max_actions(self):
        """Double-Q greedy actions of the last step as (B, T, n) int64 (q_learner.py:75)."""
        B, Tp = self._last_batch
        n = self.args.n_agents
        a = self._curmax[:(Tp - 1) * B * n].view(Tp - 1, B, n)
        return a.permute(1, 0, 2).long()

    def last_intermediate(self, which):
        """0 / 1: online / target mac_out as (B, T+1, n, A); 2: dLoss_num/dchosen as (B, T, n);
        3: online relu(fc1(inputs)) as (B, T+1, n, 64). After a TD(lambda) step (last_plan()["td_lambda"] == 1):
        4: y', the target network's mixed value at step t + 1, as (B, T, 1), or (B, T, n) without a mixer;
        5: the lambda targets in the same shape. After a prioritized-replay step (last_plan()["per"] == 1): 6: the
        unweighted |td * mask| the priority write-back summed, as (B, T, 1) (no mixer: summed over the agents).
        After a step of the two-layer hypernet (last_plan()["hyper_layers"] == 2): 7: the online net's layer-1
        pre-activations [hyper_w_1.0 | hyper_w_final.0] as (B, T, 2 * hypernet_embed). After a step that standardised
        its rewards (last_plan()["reward_norm"] == 1): 8: the standardised rewards the step read, as (B, T, 1). After
        a step of the feed-forward agent (last_agent() & 1): 9: the online net's h = relu(rnn(x1)) as
        (B, T+1, n, 64)."""
        B, Tp = self._last_batch
        n, A = self.args.n_agents, self.args.n_actions
        out = self._handle.copy_intermediate(which, self._online.device)
        if which in (0, 1):
            return out.view(Tp, B, n, A).permute(1, 0, 2, 3)
        if which in (3, 9):
            return out.view(Tp, B, n, -1).permute(1, 0, 2, 3)
        if which in (4, 5, 6, 7, 8):
            return out.view(Tp - 1, B, -1).permute(1, 0, 2)
        return out.view(Tp - 1, B, n).permute(1, 0, 2)

    def set_timing(self, slots=1, phases=None):
        """Record HIP events around the named phases (None = all) for the next `slots` steps (0 = off)."""
        h = self._handle
        names = h.lib.mq_phase_names().decode().split(";")
        mask = 0xFFFFFFFF if phases is None else sum(1 << names.index(p) for p in phases)
        _lib.check(h.lib.mq_set_timing(h.h, int(slots), mask))

    def phase_times(self):
        h = self._handle
        ms = (ctypes.c_float * 32)()
        n = ctypes.c_int32()
        _lib.check(h.lib.mq_phase_times(h.h, ms, 32, ctypes.byref(n)))
        names = h.lib.mq_phase_names().decode().split(";")
        return {names[i]: ms[i] for i in range(n.value)}

    def phase_names(self):
        return _lib.load().mq_phase_names().decode().split(";")
