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
import numbers
import os

import numpy as np

import torch as th
from torch.optim import Adam, RMSprop

from .. import _lib
from ..components.episode_buffer import PrioritizedBatch, is_replay_view
from ..modules.agents.rnn_agent import agent_kind, hidden_dim
from ..modules.flat import pack, rebind
from .dp import DPCheck, SharedComm, allreduce_grad_buffer, dp_world, local_shard, native_comm_wanted
from ..modules.mixers.qmix import QMixer, hypernet_config
from ..modules.mixers.vdn import VDNMixer

MIXER_IDS = {None: _lib.MIXER_NONE, "vdn": _lib.MIXER_VDN, "qmix": _lib.MIXER_QMIX}
Q_TARGETS = ("one_step", "td_lambda")
OPTIMIZERS = ("rmsprop", "adam")
_FIELDS = [("obs", th.float32), ("state", th.float32), ("actions", th.int64), ("avail_actions", th.int32),
           ("reward", th.float32), ("terminated", th.uint8), ("filled", th.int64)]


def make_config(args, mixer, input_dim=None, max_batch=1, max_seq=2):
    cfg = _lib.MQConfig()
    cfg.n_agents = args.n_agents
    cfg.n_actions = args.n_actions
    obs = getattr(args, "obs_shape", None)
    if obs is None and input_dim is not None:
        obs = input_dim - (args.n_actions if args.obs_last_action else 0) - (args.n_agents if args.obs_agent_id else 0)
    cfg.obs_dim = int(obs)
    st = getattr(args, "state_shape", 1)
    cfg.state_dim = int(st if isinstance(st, int) else th.Size(st).numel())
    cfg.rnn_hidden_dim = hidden_dim(args)   # epymarl's hidden_dim when rnn_hidden_dim is absent
    # epymarl's use_rnn: False selects the feed-forward agent (rnn = Linear + ReLU); absent or True: the GRU
    cfg.agent = agent_kind(args)
    cfg.mixing_embed_dim = getattr(args, "mixing_embed_dim", 32)
    cfg.mixer = mixer
    cfg.double_q = int(bool(getattr(args, "double_q", True)))
    cfg.obs_last_action = int(bool(args.obs_last_action))
    cfg.obs_agent_id = int(bool(args.obs_agent_id))
    cfg.gamma = getattr(args, "gamma", 0.99)
    cfg.lr = getattr(args, "lr", 5e-4)
    cfg.optim_alpha = getattr(args, "optim_alpha", 0.99)
    cfg.optim_eps = getattr(args, "optim_eps", 1e-5)
    cfg.grad_norm_clip = getattr(args, "grad_norm_clip", 10.0)
    cfg.max_batch = int(max_batch)
    cfg.max_seq = int(max_seq)
    # opt-in masked Huber TD loss (north_star; the reference has L2 only, q_learner.py:96-97): td_loss: huber,
    # huber_delta (default 1.0); anything else keeps L2
    cfg.huber_delta = float(getattr(args, "huber_delta", 1.0)) if getattr(args, "td_loss", "l2") == "huber" else 0.0
    # opt-in TD(lambda) targets (the reference's Q learner has the one-step target only, q_learner.py:86; the
    # function is its rl_utils.build_td_lambda_targets): q_targets: td_lambda selects them with args.td_lambda.
    # Without it args.td_lambda is ignored: COMA-style configs carry td_lambda: 0.8 globally
    q_targets = getattr(args, "q_targets", "one_step")
    if q_targets not in Q_TARGETS:
        raise ValueError("q_targets {} not recognised (one of {}).".format(q_targets, ", ".join(Q_TARGETS)))
    cfg.td_lambda = float(args.td_lambda) if q_targets == "td_lambda" else 0.0
    # upstream PyMARL's two-layer QMIX hypernetwork (hypernet_layers: 2, hypernet_embed); VDN / IQL ignore the keys
    if mixer == _lib.MIXER_QMIX:
        cfg.hypernet_layers, cfg.hypernet_embed = hypernet_config(args)
    return cfg


def optimizer_config(args):
    """The optimiser keys, named as pymarl2 names them: (name, kwargs). optimizer absent or "rmsprop": ("rmsprop",
    None), the reference's RMSprop(lr, optim_alpha, optim_eps). "adam": torch.optim.Adam's lr, betas (adam_betas,
    default (0.9, 0.999)), eps (adam_eps, default 1e-8: torch's, pymarl2 does not pass optim_eps to Adam) and
    weight_decay (default 0, L2). Anything else, or adam_amsgrad: True, raises ValueError."""
    name = getattr(args, "optimizer", None)
    name = "rmsprop" if name is None else name
    if name not in OPTIMIZERS:
        raise ValueError("optimizer {} not recognised (one of {}).".format(name, ", ".join(OPTIMIZERS)))
    if name == "rmsprop":
        return name, None
    if getattr(args, "adam_amsgrad", False):
        raise ValueError("adam_amsgrad is not supported (optimizer: adam runs torch.optim.Adam's non-amsgrad step).")
    betas = tuple(float(b) for b in getattr(args, "adam_betas", (0.9, 0.999)))
    eps, wd = float(getattr(args, "adam_eps", 1e-8)), float(getattr(args, "weight_decay", 0.0))
    if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
        raise ValueError("adam_betas must be two values in [0, 1), got {}.".format(betas))
    if not eps > 0.0:
        raise ValueError("adam_eps must be > 0, got {}.".format(eps))
    if not wd >= 0.0:
        raise ValueError("weight_decay must be >= 0, got {}.".format(wd))
    return name, dict(lr=args.lr, betas=betas, eps=eps, weight_decay=wd)


def target_update_config(args):
    """epymarl's target_update_interval_or_tau: (mode, value). Key absent or None: (None, None), the reference's
    episode-counted target_update_interval applies. v > 1: ("hard", v), a hard update every v TRAINING STEPS
    (target_update_interval is then ignored). 0 < v <= 1: ("soft", v), a Polyak update with tau = v after every step.
    v <= 0, NaN or not a number (a bool is not one): ValueError."""
    v = getattr(args, "target_update_interval_or_tau", None)
    if v is None:
        return None, None
    if isinstance(v, bool) or not isinstance(v, numbers.Real):
        raise ValueError("target_update_interval_or_tau must be a number, got {!r}.".format(v))
    v = float(v)
    if not v > 0.0:   # NaN too
        raise ValueError("target_update_interval_or_tau must be > 0 (above 1: a hard update every that many training "
                         "steps; at most 1: the soft update's tau), got {}.".format(v))
    return ("hard", v) if v > 1.0 else ("soft", v)


def reward_norm_config(args):
    """epymarl's standardise_rewards: True standardises the rewards with running statistics before the TD target is
    formed. Key absent: False (epymarl's own default is True: its configs carry the key). Not a bool: ValueError; with
    learner_dp: ValueError (each rank would see only its shard's rewards)."""
    v = getattr(args, "standardise_rewards", False)
    if v is None:
        return False
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("standardise_rewards must be True or False, got {!r}.".format(v))
    if v and getattr(args, "learner_dp", False):
        raise ValueError("learner_dp is not supported with standardise_rewards: the running reward statistics belong "
                         "to one device's batches, and each rank would see only its shard")
    return bool(v)


REW_MS_INIT = (0.0, 1.0, 1e-4)   # running (mean, var, count) of a fresh learner, epymarl's RunningMeanStd


def is_per_batch(batch):
    """True for a PrioritizedReplayBuffer sample: train() runs it as a prioritized-replay step."""
    return isinstance(batch, PrioritizedBatch)


def _field_view(t, dtype):
    """(tensor usable by the kernels, t_stride): [B][T][...] with trailing dims contiguous and the right dtype."""
    if t.dtype != dtype:
        t = t.to(dtype)
    inner = 1
    for s in t.shape[2:]:
        inner *= s
    ok = t.stride(1) == inner and t.stride(0) % max(1, inner) == 0 and t[0, 0].is_contiguous()
    if not ok:
        t = t.contiguous()
    return t, t.stride(0) // max(1, inner)


def replay_view(batch, avail_bits=True):
    """MQReplay for an EpisodeBatch (episode-major storage) or a SampledBatch (storage + device ids).
    Returns (struct, keepalive) — keep the second alive until the kernels that read it have been queued.
    avail_bits: hand the kernels the buffer's avail bitmask (ReplayBuffer.avail_bits_current: rebuilt first if the
    storage was written behind its back), else they read the int32 avail_actions rows."""
    keep = []
    rep = _lib.MQReplay()
    if is_replay_view(batch):
        src = batch.source.data.transition_data
        tstride = batch.source.max_seq_length
        if is_per_batch(batch):
            # prioritized replay: the ids were written by the sampler kernel and exist on the device only
            ids = batch.ep_ids
            keep.append(ids)
            rep.ep_ids = ids.data_ptr()
            rep.ep_ids_host = None
        elif len(batch.ep_ids_np) <= _lib.INLINE_IDS:
            # ids travel in the kernel arguments: no host-to-device copy on the step's stream
            host = np.ascontiguousarray(batch.ep_ids_np, dtype=np.int64)
            keep.append(host)
            rep.ep_ids_host = host.ctypes.data
            rep.ep_ids = None
        else:
            ids = batch.ep_ids
            keep.append(ids)
            rep.ep_ids = ids.data_ptr()
        rep.n_episodes = batch.source.batch_size
        rep.t_len = batch.t_len
        tensors = {}
        for k, dt in _FIELDS:
            if k not in src:
                continue
            t = src[k]
            if t.dtype != dt or not t.is_contiguous():
                raise _lib.MQError("replay field {} must be a contiguous {} tensor".format(k, dt))
            tensors[k] = t
        cur = getattr(batch.source, "avail_bits_current", None)
        bits = cur() if (avail_bits and cur is not None) else None
        if bits is not None:
            keep.append(bits)
            rep.avail_bits = bits.data_ptr()
    else:
        src = batch.data.transition_data
        tensors, strides = {}, set()
        for k, dt in _FIELDS:
            if k not in src:
                continue
            t, ts = _field_view(src[k], dt)
            tensors[k] = t
            strides.add(ts)
        if len(strides) != 1:
            tensors = {k: v.contiguous() for k, v in tensors.items()}
            strides = {batch.max_seq_length}
        tstride = strides.pop()
        rep.ep_ids = None
        rep.n_episodes = batch.batch_size
        rep.t_len = batch.max_seq_length
    for k, t in tensors.items():
        keep.append(t)
        setattr(rep, k, t.data_ptr())
    _lib.require_gpu(tensors["obs"])
    rep.batch_size = batch.batch_size
    rep.t_stride = int(tstride)
    return rep, keep


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
        self._step_t = th.tensor(float(getattr(self, "_opt_steps", 0)))
        o = 0
        for p in self.params:
            n = p.numel()
            p.grad = self._grad[o:o + n].view_as(p)
            st = self.optimiser.state[p]
            if self.optim_name == "adam":   # torch.optim.Adam's state keys, in its order
                st["step"] = self._step_t
                st["exp_avg"] = self._m[o:o + n].view_as(p)
                st["exp_avg_sq"] = self._sq[o:o + n].view_as(p)
            else:
                st["square_avg"] = self._sq[o:o + n].view_as(p)
                st["step"] = self._step_t   # one shared counter: train() increments it once, not once per parameter
            o += n
        self._handle = None

    def _dp_active(self):
        if not self.dp:
            return False
        import torch.distributed as dist
        return dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1

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
        if self._online.is_cuda and self._handle is not None:
            _lib.check(self._handle.lib.mq_update_targets(self._handle.h, _lib.stream_ptr()))
        else:
            with th.no_grad():
                self._target.copy_(self._online)
        self.logger.console_logger.info("Updated target network")

    def cuda(self):
        dev = th.device("cuda", th.cuda.current_device())
        self._online = self._online.to(dev)
        self._target = self._target.to(dev)
        self._grad = self._grad.to(dev)
        self._sq = self._sq.to(dev)
        if self._m is not None:
            self._m = self._m.to(dev)
        self._stats = self._stats.to(dev)
        if self.rew_ms is not None:
            self.rew_ms = self.rew_ms.to(dev)
        self._relink()

    def reward_stats(self):
        """The running reward statistics as a dict of Python floats: mean, var, count (synchronises)."""
        if self.rew_ms is None:
            raise _lib.MQError("reward_stats() needs standardise_rewards: True")
        m, v, c = self.rew_ms.tolist()
        return dict(mean=m, var=v, count=c)

    def save_models(self, path):
        self.mac.save_models(path)
        if self.mixer is not None:
            th.save(self.mixer.state_dict(), "{}/mixer.th".format(path))
        # per-parameter step tensors in the file, as torch's RMSprop writes them: the live state shares one counter,
        # and a loader that kept it shared would count every parameter's update into it
        sd = self.optimiser.state_dict()
        sd["state"] = {i: dict(v, step=v["step"].clone()) if "step" in v else v for i, v in sd["state"].items()}
        th.save(sd, "{}/opt.th".format(path))
        # the epymarl keys' state, as plain dicts of Python numbers: the running reward statistics, and the counters
        # of the step-counted target schedule
        if self.rew_ms is not None:
            th.save(self.reward_stats(), "{}/rew_ms.th".format(path))
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
        # an opt.th of the other optimiser would load without complaint (torch checks only the group sizes) and
        # leave the moments this learner steps with at zero
        groups = sd.get("param_groups") or [{}]
        wrote = "adam" if "betas" in groups[0] else "rmsprop" if "alpha" in groups[0] else None
        if wrote is not None and wrote != self.optim_name:
            raise ValueError("{}/opt.th was written by {}, but this learner runs optimizer: {}.".format(
                path, {"adam": "Adam", "rmsprop": "RMSprop"}[wrote], self.optim_name))
        self.optimiser.load_state_dict(sd)
        # load_state_dict replaced the state tensors: copy back into the flat buffers
        flat = {"exp_avg": self._m, "exp_avg_sq": self._sq} if self.optim_name == "adam" else {"square_avg": self._sq}
        o = 0
        for p in self.params:
            n = p.numel()
            st = self.optimiser.state.get(p, {})
            for key, buf in flat.items():
                if key in st:
                    buf[o:o + n].copy_(st[key].reshape(-1))
            o += n
        steps = [float(self.optimiser.state[p]["step"]) for p in self.params if "step" in self.optimiser.state[p]]
        self._opt_steps = int(steps[0]) if steps else 0
        if self.rew_ms is not None:
            f = "{}/rew_ms.th".format(path)
            if os.path.exists(f):
                ms = th.load(f, map_location=ml, weights_only=True)
                vals = [float(ms["mean"]), float(ms["var"]), float(ms["count"])]
            else:   # a checkpoint written without standardise_rewards: start the statistics afresh, and say so
                vals = list(REW_MS_INIT)
                self.logger.console_logger.warning(
                    "{} not found: standardise_rewards starts from fresh reward statistics".format(f))
            self.rew_ms.copy_(th.tensor(vals, dtype=th.float64))
        if self.target_mode is not None:
            f = "{}/target_update.th".format(path)
            if os.path.exists(f):
                tu = th.load(f, map_location=ml, weights_only=True)
                self.training_steps = int(tu["training_steps"])
                self.last_target_update_step = int(tu["last_target_update_step"])
        self._relink()

    # -- extras (parity / diagnostics) -----------------------------------------------------------------------
    def collective(self):
        """How a data-parallel step sums the gradient buffer: "rccl-native" (the library's communicator),
        "torch.distributed", or None (not data parallel)."""
        if not self._dp_active():
            return None
        return "rccl-native" if (self._handle is not None and self._handle.native) else "torch.distributed"

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
        cnt = ctypes.c_int64()
        h = self._handle
        _lib.check(h.lib.mq_copy_intermediate(h.h, which, None, ctypes.byref(cnt), None))
        out = th.empty(cnt.value, dtype=th.float32, device=self._online.device)
        _lib.check(h.lib.mq_copy_intermediate(h.h, which, _lib.ptr(out), ctypes.byref(cnt), _lib.stream_ptr()))
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
