"""PPOLearner: epymarl's ppo_learner (configs mappo.yaml / ippo.yaml), MI355X-native, opt-in through
`learner: ppo_learner`. DESIGN.md §3l holds the specification it implements.

ActorCriticLearner with `epochs` optimisation epochs per train() on the clipped surrogate
min(ratio adv, clamp(ratio, 1 - eps_clip, 1 + eps_clip) adv): every key, refusal, buffer and checkpoint file is that
learner's. The returns, the standardised rewards and the running reward statistics are formed once per train(); each
epoch is one critic step and one actor step with the nets' current parameters, and the old policy is the policy at the
start of the train() (epoch 0's own log-probabilities: there is no second controller and nothing new is
checkpointed). All of train() is one launch sequence (include/ma_a2c.h ma_set_ppo, pymarl_amd/csrc/ppo_host.hpp) and
one synchronisation: the read-back of the per-epoch stats.

Keys of its own: `epochs` (an int >= 1, default 4) and `eps_clip` (0 < eps_clip < 1, default 0.2). Counters:
critic_training_steps counts train() calls (the target-update schedule runs once per train(), after the last epoch),
both optimisers' step counts advance by `epochs`.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch as th

from .. import _lib
from .actor_critic_learner import A2C_STATS, ActorCriticLearner, a2c_config
from ..components.episode_buffer import is_per_batch, replay_view
from ..modules.flat import to_current_device

CRITIC_STATS = ("critic_loss", "critic_grad_norm", "td_error_abs", "q_taken_mean", "target_mean")
PPO_STATS = A2C_STATS + ["clip_frac"]


def ppo_config(args):
    """a2c_config's namespace (every key and refusal of the actor-critic learner) with epochs and eps_clip, checked."""
    cfg = a2c_config(args)
    e = getattr(args, "epochs", 4)
    if isinstance(e, bool) or not isinstance(e, (int, np.integer)) or e < 1:
        raise ValueError("epochs must be an int >= 1, got {!r}.".format(e))
    c = getattr(args, "eps_clip", 0.2)
    if isinstance(c, bool) or not isinstance(c, (int, float, np.floating, np.integer)) or not 0.0 < float(c) < 1.0:
        raise ValueError("eps_clip must be a number with 0 < eps_clip < 1, got {!r}.".format(c))
    cfg.epochs, cfg.eps_clip = int(e), float(c)
    return cfg


class PPOLearner(ActorCriticLearner):
    def __init__(self, mac, scheme, logger, args):
        pc = ppo_config(args)   # before anything is built: a bad key of either learner is a ValueError
        self.epochs, self.eps_clip = pc.epochs, pc.eps_clip
        self._ppo_handle = None
        super().__init__(mac, scheme, logger, args)
        self._estats = th.zeros(self.epochs * _lib.MA_NSTATS, dtype=th.float32, device=self._stats.device)

    def _get_handle(self, batch):
        h = super()._get_handle(batch)
        if h is not self._ppo_handle:   # a new handle: switch it to the PPO step
            pp = _lib.MAPpo(epochs=self.epochs, eps_clip=self.eps_clip, epoch_stats=self._estats.data_ptr())
            _lib.check(h.lib.ma_set_ppo(h.h, ctypes.byref(pp)))
            self._ppo_handle = h
        return h

    def train(self, batch, t_env: int, episode_num: int):
        if is_per_batch(batch):
            raise ValueError("PPOLearner is on-policy and does not take a PrioritizedReplayBuffer batch: its loss "
                             "carries no importance weights and it writes no priorities back")
        _lib.require_gpu(self._agent)
        h = self._get_handle(batch)
        rep, keep = replay_view(batch)
        _lib.check(h.lib.ma_train_step(h.h, ctypes.byref(rep), self._opt_steps + 1, _lib.stream_ptr()))
        del keep
        rows = self._estats.view(self.epochs, _lib.MA_NSTATS).tolist()   # the one synchronisation per train()
        self._last_batch = (batch.batch_size, rep.t_len)
        M = rows[-1][_lib.A2C_MASK_ELEMS]
        per_epoch = [dict({k: r[i] for k, i in _lib.A2C_STATS.items()}, clipped=int(r[_lib.PPO_STAT_CLIPPED]))
                     for r in rows]
        self._last = dict(per_epoch[-1])   # the actor's stats are the last epoch's (epymarl's logging)
        del self._last["clipped"]
        for k in CRITIC_STATS:             # the critic's are the mean over the epochs
            self._last[k] = sum(e[k] for e in per_epoch) / self.epochs
        self._last["clip_frac"] = per_epoch[-1]["clipped"] / M if M > 0.0 else 0.0
        self._last["mask_elems"] = M
        self._last["epochs"] = per_epoch
        if not M > 0.0:
            return   # an empty batch: no epoch applied anything, nothing is counted
        self._opt_steps += self.epochs
        self._step_t += self.epochs
        self.critic_training_steps += 1
        self._target_schedule()

        if t_env - self.log_stats_t >= self.args.learner_log_interval:
            for key in PPO_STATS:
                self.logger.log_stat(key, self._last[key], t_env)
            self.log_stats_t = t_env

    def cuda(self):
        to_current_device(self, ("_estats",))
        super().cuda()

    def last_stats(self):
        """The last train()'s stats: the five critic stats as means over the epochs, the four actor stats and
        clip_frac (the share of live rows whose surrogate gradient was cut) of the last epoch, and under "epochs" one
        dict per epoch with all nine and `clipped`, that epoch's count of such rows."""
        return dict(self._last, epochs=[dict(e) for e in self._last["epochs"]])

    def last_intermediate(self, which):
        """ActorCriticLearner's ids (1, 3 and 4 hold the last epoch's values), and 5: old, the log-probabilities of the
        taken actions at the start of the train(), (B, T, n); 6: the last epoch's ratio, (B, T, n)."""
        if which not in (5, 6):
            return super().last_intermediate(which)
        B, Tp = self._last_batch
        out = self._handle.copy_intermediate(which, self._agent.device)
        return out.view(Tp - 1, B, self.n_agents).permute(1, 0, 2)
