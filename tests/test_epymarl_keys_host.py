"""epymarl's two learner keys, the parts that need no GPU: parsing of target_update_interval_or_tau and
standardise_rewards with their ValueErrors, the step-counted hard target schedule, the float64 reference of the reward
statistics (tests/reward_norm_ref.py) against a torch transcription of the merge, and the argument checks of the new
C entry points that return before any launch."""
import ctypes
import math
from types import SimpleNamespace as SN

import numpy as np
import pytest
import torch as th

from pymarl_amd import _lib
from pymarl_amd.learners.q_learner import REW_MS_INIT, reward_norm_config, target_update_config
from tests import reward_norm_ref as R
from tests.golden_utils import Case
from tests.gpu_helpers import build


# ---------------------------------------------------------------------------------------------- parsing
def test_target_key_absent_or_none_keeps_the_episode_rule():
    assert target_update_config(SN()) == (None, None)
    assert target_update_config(SN(target_update_interval_or_tau=None)) == (None, None)


@pytest.mark.parametrize("v,want", [(200, ("hard", 200.0)), (2, ("hard", 2.0)), (1.5, ("hard", 1.5)),
                                    (1, ("soft", 1.0)), (1.0, ("soft", 1.0)), (0.01, ("soft", 0.01)),
                                    (np.float32(0.25), ("soft", 0.25)), (np.int64(3), ("hard", 3.0))])
def test_target_key_values(v, want):
    assert target_update_config(SN(target_update_interval_or_tau=v)) == want


@pytest.mark.parametrize("v", [0, 0.0, -1, -0.01, float("nan"), "200", "soft", True, False, [200], (0.01,)])
def test_target_key_errors(v):
    with pytest.raises(ValueError, match="target_update_interval_or_tau"):
        target_update_config(SN(target_update_interval_or_tau=v))


def test_standardise_rewards_parsing():
    assert reward_norm_config(SN()) is False
    assert reward_norm_config(SN(standardise_rewards=False)) is False
    assert reward_norm_config(SN(standardise_rewards=True)) is True
    assert reward_norm_config(SN(standardise_rewards=False, learner_dp=True)) is False
    for v in ("True", 1, 0.5):
        with pytest.raises(ValueError, match="standardise_rewards"):
            reward_norm_config(SN(standardise_rewards=v))
    with pytest.raises(ValueError, match="learner_dp is not supported with standardise_rewards"):
        reward_norm_config(SN(standardise_rewards=True, learner_dp=True))


@pytest.fixture(scope="module")
def case():
    return Case("tiny_qmix")


def test_learner_raises_at_construction(case):
    for v in (0, -2, float("nan"), "x"):
        with pytest.raises(ValueError, match="target_update_interval_or_tau"):
            build(case, device="cpu", target_update_interval_or_tau=v)
    with pytest.raises(ValueError, match="learner_dp is not supported with standardise_rewards"):
        build(case, device="cpu", standardise_rewards=True, learner_dp=True)


def test_learner_state_of_the_keys(case):
    _, _, _, plain, _ = build(case, device="cpu")
    assert plain.target_mode is None and plain.rew_ms is None
    assert plain.training_steps == 0 and plain.last_target_update_step == 0
    _, _, _, lr, _ = build(case, device="cpu", standardise_rewards=True, target_update_interval_or_tau=0.01)
    assert (lr.target_mode, lr.target_value) == ("soft", 0.01)
    assert lr.rew_ms.dtype == th.float64 and lr.rew_ms.tolist() == list(REW_MS_INIT) == list(R.INIT)
    assert lr.reward_stats() == dict(mean=0.0, var=1.0, count=1e-4)


# ---------------------------------------------------------------------------------------------- the schedule
@pytest.mark.parametrize("v", [2, 3, 200])
def test_hard_update_by_training_steps(case, v):
    """Seven train() calls' worth of the schedule (the part of train() behind the optimiser step) on a CPU learner:
    the update runs at call c exactly when (c - last) / v >= 1.0 with last the call of the previous update, i.e. at
    c = v, 2 v, ..; episode_num is chosen so that the episode rule would have fired at every call, and must be
    ignored."""
    _, _, _, learner, _ = build(case, device="cpu", target_update_interval_or_tau=v, target_update_interval=1)
    last, fired = 0, []
    for c in range(1, 8):
        with th.no_grad():
            learner._online += 1.0   # the optimiser step of this call
        before = learner._target.clone()
        learner._target_schedule(episode_num=1000 * c)
        due = (c - last) / v >= 1.0
        if due:
            last = c
            fired.append(c)
            assert th.equal(learner._target, learner._online)
        else:
            assert th.equal(learner._target, before)
        assert learner.training_steps == c and learner.last_target_update_step == last
        assert learner.last_target_update_episode == 0
    assert fired == [c for c in range(1, 8) if c % v == 0]


def test_soft_mode_and_absent_key_schedules(case):
    _, _, _, soft, _ = build(case, device="cpu", target_update_interval_or_tau=0.5, target_update_interval=1)
    before = soft._target.clone()
    with th.no_grad():
        soft._online += 1.0
    soft._target_schedule(episode_num=1000)
    assert th.equal(soft._target, before) and soft.training_steps == 1   # the kernel moves the targets, not this
    _, _, _, plain, _ = build(case, device="cpu", target_update_interval=200)
    with th.no_grad():
        plain._online += 1.0
    plain._target_schedule(episode_num=199)
    assert not th.equal(plain._target, plain._online)
    plain._target_schedule(episode_num=200)
    assert th.equal(plain._target, plain._online) and plain.last_target_update_episode == 200


# ---------------------------------------------------------------------------------------------- checkpoint files
def test_checkpoint_files_round_trip_on_the_host(case, tmp_path):
    _, _, _, a, _ = build(case, device="cpu", standardise_rewards=True, target_update_interval_or_tau=3)
    a.rew_ms.copy_(th.tensor([0.125, 2.5, 16777217.0001], dtype=th.float64))   # a count past 2^24
    a.training_steps, a.last_target_update_step = 7, 6
    a.save_models(str(tmp_path))
    ms = th.load(str(tmp_path / "rew_ms.th"), weights_only=True)
    assert ms == dict(mean=0.125, var=2.5, count=16777217.0001) and all(type(x) is float for x in ms.values())
    _, _, _, b, _ = build(case, device="cpu", standardise_rewards=True, target_update_interval_or_tau=3)
    b.load_models(str(tmp_path))
    assert b.rew_ms.tolist() == [0.125, 2.5, 16777217.0001]
    assert (b.training_steps, b.last_target_update_step) == (7, 6)


def test_missing_rew_ms_file_warns_once_and_keeps_fresh_statistics(case, tmp_path, caplog):
    _, _, _, a, _ = build(case, device="cpu")
    a.save_models(str(tmp_path))
    assert not (tmp_path / "rew_ms.th").exists() and not (tmp_path / "target_update.th").exists()
    _, _, _, b, _ = build(case, device="cpu", standardise_rewards=True)
    b.rew_ms.fill_(3.0)
    with caplog.at_level("WARNING"):
        b.load_models(str(tmp_path))
    assert b.rew_ms.tolist() == list(REW_MS_INIT)
    assert len([r for r in caplog.records if "rew_ms.th" in r.getMessage()]) == 1


# ---------------------------------------------------------------------------------------------- the reference
def torch_merge(state, x):
    """The merge as written in the specification, transcribed with torch's own mean / var on a float64 tensor."""
    mean, var, count = (th.tensor(v, dtype=th.float64) for v in state)
    x = th.as_tensor(np.asarray(x, np.float64)).reshape(-1)
    M = x.numel()
    bm = th.mean(x)
    bv = th.var(x, unbiased=True) if M > 1 else th.zeros((), dtype=th.float64)   # torch gives NaN at M = 1
    delta = bm - mean
    tot = count + M
    new_mean = mean + delta * M / tot
    new_var = (var * count + bv * M + delta ** 2 * count * M / tot) / tot
    return float(new_mean), float(new_var), float(tot)


def close(a, b, tol=1e-13):
    return all(abs(x - y) <= tol * max(1.0, abs(y)) for x, y in zip(a, b))


def test_reference_three_successive_batches():
    rng = np.random.default_rng(3)
    s_ref, s_th = R.INIT, R.INIT
    for k, shape in enumerate([(4, 7, 1), (3, 5, 1), (9, 130, 1)]):
        x = (rng.standard_normal(shape) * (k + 1) + 0.5 * k).astype(np.float32)
        s_th = torch_merge(s_th, x)
        s_ref, r_std = R.standardise(s_ref, x)
        assert close(s_ref, s_th), (k, s_ref, s_th)
        assert r_std.shape == shape and r_std.dtype == np.float64
        want = (x.astype(np.float64) - s_th[0]) / math.sqrt(s_th[1])
        assert np.abs(r_std - want).max() <= 1e-12 * np.abs(want).max()
    assert s_ref[2] == 1e-4 + 28 + 15 + 1170
    # the running statistics approach those of all the data seen (the initial pseudo-count is 1e-4 of a sample)
    assert s_ref[1] > 0


def test_reference_single_value_batch():
    s = R.merge(R.INIT, np.array([[[2.0]]], np.float32))
    assert s == torch_merge(R.INIT, [2.0])
    bm, bv, M = R.batch_moments([2.0])
    assert (bm, bv, M) == (2.0, 0.0, 1)
    tot = 1e-4 + 1
    assert s[2] == tot and abs(s[0] - 2.0 / tot) < 1e-15
    # var' = (1 * 1e-4 + 0 + 4 * 1e-4 / tot) / tot: finite and positive where torch's unbiased variance is NaN
    assert math.isfinite(s[1]) and abs(s[1] - (1e-4 + 4e-4 / tot) / tot) < 1e-18
    _, r_std = R.standardise(R.INIT, np.array([2.0], np.float32))
    assert np.isfinite(r_std).all()


def test_reference_all_equal_rewards_shrink_the_variance_but_keep_it_positive():
    x = np.full((5, 60, 1), 0.75, np.float32)
    s = R.INIT
    for _ in range(3):
        s1, r_std = R.standardise(s, x)
        assert close(s1, torch_merge(s, x))
        assert 0.0 < s1[1] < s[1]
        assert np.isfinite(r_std).all()
        s = s1
    assert abs(s[0] - 0.75) < 1e-6


# ---------------------------------------------------------------------------------------------- the C boundary
def test_new_entry_points_check_their_arguments_before_any_launch():
    lib = _lib.load()
    f = ctypes.c_float
    buf = ctypes.c_void_p(4096)   # never dereferenced: every call below fails its checks first
    assert lib.mq_soft_update(None, buf, 4, f(0.5), f(0.5), None) == 1 and b"NULL" in lib.mq_last_error()
    assert lib.mq_soft_update(buf, None, 4, f(0.5), f(0.5), None) == 1
    assert lib.mq_soft_update(buf, buf, -1, f(0.5), f(0.5), None) == 1 and b"n must be" in lib.mq_last_error()
    for tau in (0.0, -0.5, 1.5, float("nan")):
        assert lib.mq_soft_update(buf, buf, 4, f(1.0 - tau), f(tau), None) == 1
        assert b"tau" in lib.mq_last_error()
    assert lib.mq_soft_update(buf, buf, 0, f(0.0), f(1.0), None) == 0   # nothing to do, nothing launched
    assert lib.mq_set_soft_target(None, 0.5) == 1
    assert lib.mq_set_reward_norm(None, buf) == 1
    assert lib.mq_last_reward_norm(None) == -1 and lib.mq_last_soft_target(None) == -1
    assert "mq_soft_update" in _lib.EXPORTS and "mq_set_reward_norm" in _lib.EXPORTS
