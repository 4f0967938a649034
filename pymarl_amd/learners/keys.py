"""The opt-in config keys the learners share (pymarl2's optimizer, epymarl's target_update_interval_or_tau and
standardise_rewards), parsed and checked, and the running reward statistics' checkpoint file rew_ms.th."""
import numbers
import os

import numpy as np
import torch as th

from .. import _lib

OPTIMIZERS = ("rmsprop", "adam")
REW_MS_INIT = (0.0, 1.0, 1e-4)   # running (mean, var, count) of a fresh learner, epymarl's RunningMeanStd


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


def hard_target_update(handle, fn, target, online, logger, *args):
    """A learner's `_update_targets`: target := online, by the library (`fn`(handle, *args, stream)) once a handle
    exists on the device, by torch before that."""
    if online.is_cuda and handle is not None:
        _lib.check(getattr(handle.lib, fn)(handle.h, *args, _lib.stream_ptr()))
    else:
        with th.no_grad():
            target.copy_(online)
    logger.console_logger.info("Updated target network")


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


def reward_stats(rew_ms):
    """The running reward statistics as a dict of Python floats: mean, var, count (synchronises)."""
    if rew_ms is None:
        raise _lib.MQError("reward_stats() needs standardise_rewards: True")
    m, v, c = rew_ms.tolist()
    return dict(mean=m, var=v, count=c)


def save_rew_ms(rew_ms, path):
    """rew_ms.th: the statistics as a plain dict of Python numbers (no file without standardise_rewards)."""
    if rew_ms is not None:
        th.save(reward_stats(rew_ms), "{}/rew_ms.th".format(path))


def load_rew_ms(rew_ms, path, logger):
    """Read rew_ms.th into `rew_ms`. A checkpoint written without standardise_rewards has none: start the statistics
    afresh, and say so."""
    if rew_ms is None:
        return
    f = "{}/rew_ms.th".format(path)
    if os.path.exists(f):
        ms = th.load(f, map_location=lambda s, loc: s, weights_only=True)
        vals = [float(ms["mean"]), float(ms["var"]), float(ms["count"])]
    else:
        vals = list(REW_MS_INIT)
        logger.console_logger.warning("{} not found: standardise_rewards starts from fresh reward statistics".format(f))
    rew_ms.copy_(th.tensor(vals, dtype=th.float64))
