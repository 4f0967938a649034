"""The PPO learner's host side, without a GPU: the registry, key parsing and every refusal (the
actor-critic learner's through PPOLearner included), ma_set_ppo's argument checks, the hand-derived dLoss/dlogits of
the clipped surrogate against autograd in float64, the reference's epoch 0 against tests/a2c_ref.py's step, the seed
conditions of tests/ppo_ref.py's rows, and a checkpoint round trip on CPU tensors."""
import ctypes
import os
from types import SimpleNamespace as SN

import numpy as np
import pytest
import torch as th

from pymarl_amd import _lib
from pymarl_amd.components.episode_buffer import PrioritizedBatch
from pymarl_amd.learners import REGISTRY as le_REGISTRY
from pymarl_amd.learners.actor_critic_learner import ActorCriticLearner
from pymarl_amd.learners.ppo_learner import PPOLearner, ppo_config
from tests import a2c_ref as R
from tests import ppo_ref as P
from tests.a2c_helpers import all_buffers
from tests.ppo_helpers import build_ppo, make_ppo_args


# ------------------------------------------------------------------------------------------ registry, keys
def test_registry_and_abi():
    assert le_REGISTRY["ppo_learner"] is PPOLearner and issubclass(PPOLearner, ActorCriticLearner)
    assert le_REGISTRY["actor_critic_learner"] is ActorCriticLearner
    lib = _lib.load()
    assert "ma_set_ppo" in _lib.MA_EXPORTS and hasattr(lib, "ma_set_ppo")
    assert ctypes.sizeof(_lib.MAPpo) == 16 and _lib.MAPpo.epoch_stats.offset == 8
    assert [k for k, _ in _lib.MAPlan._fields_][-2:] == ["epochs", "hoisted"]


def test_key_parsing_defaults_and_values():
    c = P.PPOCase("part")
    base = make_ppo_args(c)
    for k in ("epochs", "eps_clip", "q_nstep", "entropy_coef", "optimizer"):
        delattr(base, k)
    cfg = ppo_config(base)
    assert (cfg.epochs, cfg.eps_clip) == (4, 0.2) and type(cfg.epochs) is int
    assert (cfg.q_nstep, cfg.entropy_coef, cfg.optimizer[0]) == (5, 0.01, "adam")   # the actor-critic learner's
    cfg = ppo_config(make_ppo_args(c, epochs=np.int64(7), eps_clip=np.float32(0.5)))
    assert (cfg.epochs, cfg.eps_clip) == (7, 0.5)
    for name, critic in (("mappo", "cv_critic"), ("ippo", "ac_critic")):   # epymarl's two configurations
        cfg = ppo_config(make_ppo_args(c, critic_type=critic, epochs=4, eps_clip=0.2, q_nstep=5, entropy_coef=0.001,
                                       target_update_interval_or_tau=0.01, standardise_rewards=True))
        assert (cfg.critic_type, cfg.epochs, cfg.eps_clip, cfg.target) == (critic, 4, 0.2, ("soft", 0.01)), name
        assert cfg.standardise_rewards is True and cfg.entropy_coef == 0.001


@pytest.mark.parametrize("over,match", [
    # the actor-critic learner's refusals, through PPOLearner
    (dict(critic_type="coma"), "critic_type"), (dict(critic_type=None), "critic_type"),
    (dict(use_rnn=False), "use_rnn"), (dict(learner_dp=True), "learner_dp"),
    (dict(standardise_returns=True), "standardise_returns"), (dict(obs_individual_obs=True), "obs_individual_obs"),
    (dict(q_nstep=0), "q_nstep"), (dict(entropy_coef=-0.1), "entropy_coef"), (dict(optimizer="sgd"), "optimizer"),
    (dict(target_update_interval_or_tau=0), "target_update_interval_or_tau"),
    (dict(standardise_rewards="yes"), "standardise_rewards"), (dict(hidden_dim=96), "hidden_dim"),
    # its own two keys
    (dict(epochs=0), "epochs"), (dict(epochs=-1), "epochs"), (dict(epochs=True), "epochs"), (dict(epochs=2.0), "epochs"),
    (dict(epochs="4"), "epochs"), (dict(epochs=None), "epochs"),
    (dict(eps_clip=0), "eps_clip"), (dict(eps_clip=0.0), "eps_clip"), (dict(eps_clip=1), "eps_clip"),
    (dict(eps_clip=1.0), "eps_clip"), (dict(eps_clip=-0.2), "eps_clip"), (dict(eps_clip=True), "eps_clip"),
    (dict(eps_clip=False), "eps_clip"), (dict(eps_clip="0.2"), "eps_clip"), (dict(eps_clip=None), "eps_clip"),
    (dict(eps_clip=float("nan")), "eps_clip"),
])
def test_refusals_at_construction(over, match):
    c = P.PPOCase("part")
    scheme = {"state": {"vshape": c.S}, "obs": {"vshape": c.O, "group": "agents"}}
    mac = SN(parameters=lambda: [], agent=SN())
    with pytest.raises(ValueError, match=match):
        PPOLearner(mac, scheme, None, make_ppo_args(c, **over))


def test_prioritized_batch_is_refused():
    c = P.PPOCase("one")
    _, _, _, learner, _ = build_ppo(c, device="cpu")
    assert type(learner) is PPOLearner and (learner.epochs, learner.eps_clip) == (3, 0.01)
    with pytest.raises(ValueError, match="PrioritizedReplayBuffer"):
        learner.train(PrioritizedBatch.__new__(PrioritizedBatch), 0, 0)


def test_ma_set_ppo_refuses_bad_arguments():
    """The arguments are checked before the handle and before any HIP call, so the checks run without a GPU."""
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    good = ctypes.addressof(buf)
    assert good % 4 == 0
    for kw, msg in ((dict(epochs=0, eps_clip=0.2, epoch_stats=good), b"epochs"),
                    (dict(epochs=-3, eps_clip=0.2, epoch_stats=good), b"epochs"),
                    (dict(epochs=4, eps_clip=0.0, epoch_stats=good), b"eps_clip"),
                    (dict(epochs=4, eps_clip=1.0, epoch_stats=good), b"eps_clip"),
                    (dict(epochs=4, eps_clip=-0.1, epoch_stats=good), b"eps_clip"),
                    (dict(epochs=4, eps_clip=float("nan"), epoch_stats=good), b"eps_clip"),
                    (dict(epochs=4, eps_clip=0.2, epoch_stats=None), b"NULL"),
                    (dict(epochs=4, eps_clip=0.2, epoch_stats=good + 2), b"aligned"),
                    (dict(epochs=4, eps_clip=0.2, epoch_stats=good), b"NULL handle")):
        pp = _lib.MAPpo(**kw)
        assert lib.ma_set_ppo(None, ctypes.byref(pp)) != 0, kw
        assert msg in lib.mq_last_error(), (kw, lib.mq_last_error())
    assert lib.ma_set_ppo(None, None) != 0 and b"NULL handle" in lib.mq_last_error()


# ------------------------------------------------------------------------------------------ the gradient
def surrogate_formula(p, avail, actions, m, adv, ratio, lo, hi, ec, mbs, M):
    """DESIGN.md §3l's hand-derived dLoss/dlogits (the kernel's form, here with the 1 / M scale):
    w = 1 where lo <= ratio <= hi or ratio adv < clamp(ratio, lo, hi) adv, else 0; c = (w ratio) adv;
    g_j = -(m / M) [c [j == u] / (p_j + 1e-10) - ec (log(p_j + 1e-10) + p_j / (p_j + 1e-10))];
    dlogit_k = p_k (g_k - sum_j p_j g_j), zero at masked-before-softmax actions and on dead rows."""
    w = ((ratio >= lo) & (ratio <= hi)) | (ratio * adv < th.clamp(ratio, lo, hi) * adv)
    c = (w.to(p.dtype) * ratio) * adv
    onehot = th.zeros_like(p).scatter_(-1, actions, 1.0)
    den = p + 1e-10
    g = -(m / M).unsqueeze(-1) * (c.unsqueeze(-1) * onehot / den - ec * (th.log(den) + p / den))
    dl = p * (g - (p * g).sum(-1, keepdim=True))
    dl = dl * (m.unsqueeze(-1) != 0)
    return (dl.masked_fill(avail == 0, 0.0) if mbs else dl), w


@pytest.mark.parametrize("mbs", [True, False])
@pytest.mark.parametrize("ec", [0.0, 0.01])
def test_surrogate_formula_against_autograd_float64(mbs, ec):
    rng = np.random.Generator(np.random.PCG64(11))
    B, T, n, A = 4, 6, 2, 6
    logits = th.tensor(rng.standard_normal((B, T, n, A)), requires_grad=True)
    avail = th.tensor((rng.random((B, T, n, A)) < 0.6).astype(np.int64))
    avail[..., 1] = 1
    keys = th.tensor(rng.random((B, T, n, A))).masked_fill(avail == 0, -1.0)
    actions = keys.argmax(-1, keepdim=True)
    m = th.ones(B, T, n, dtype=th.float64)
    m[1, 3:] = 0
    m[2] = 0
    adv = th.tensor(rng.standard_normal((B, T, n))) * m
    adv[0, 0] = 0.0   # adv = 0 rows, one inside and one outside the range (old below)
    M = float(m.sum())
    lg = logits.masked_fill(avail == 0, -1e10) if mbs else logits
    p = th.softmax(lg, -1)
    pi = th.where(m.unsqueeze(-1) == 0, th.ones_like(p), p)
    ent = -(pi * th.log(pi + 1e-10)).sum(-1)
    lp = th.log(th.gather(pi, -1, actions).squeeze(-1) + 1e-10)
    # old log-probabilities that spread the ratios over about [0.9, 1.1], dead rows at ratio 1
    old = lp.detach() - th.tensor(rng.uniform(-0.1, 0.1, (B, T, n))) * (m != 0)
    old[0, 0, 0] = lp.detach()[0, 0, 0] - 0.001  # adv = 0 inside the range
    old[0, 0, 1] = lp.detach()[0, 0, 1] - 0.09   # adv = 0 outside the range
    ratio = th.exp(lp - old)
    # the bounds are two of the ratios themselves: one row sits exactly on lo, one exactly on hi
    live = m != 0
    r = ratio.detach()
    lo = float(r[live & (r < 0.97)].max())
    hi = float(r[live & (r > 1.03)].min())
    s1, s2 = ratio * adv, th.clamp(ratio, lo, hi) * adv
    loss = -((th.min(s1, s2) + ec * ent) * m).sum() / M
    loss.backward()
    want, w = surrogate_formula(p.detach(), avail, actions, m, adv, r, lo, hi, ec, mbs, M)
    assert (logits.grad - want).abs().max().item() < 1e-15
    inside = (r >= lo) & (r <= hi)
    # every kind of row is present
    assert int((live & inside & (r > lo) & (r < hi)).sum()) >= 5
    assert int((live & ~inside & ~w).sum()) >= 3 and int((live & ~inside & w & (adv != 0)).sum()) >= 3
    assert int((live & (r == lo)).sum()) == 1 and int((live & (r == hi)).sum()) == 1 and bool(w[r == lo].all()) and \
        bool(w[r == hi].all())
    assert bool((adv[0, 0] == 0).all()) and bool(inside[0, 0, 0]) and not bool(inside[0, 0, 1])
    assert bool((~live).any()) and th.all(logits.grad[~live] == 0.0) and th.all(r[~live] == 1.0)
    if mbs:
        assert bool((avail == 0).any()) and th.all(logits.grad[avail == 0] == 0.0)
    # where the gradient is cut and there is no entropy term, nothing reaches the logits
    if ec == 0.0:
        assert th.all(logits.grad[live & ~w] == 0.0)


@pytest.mark.parametrize("row", ["part", "part_n10", "part_ac"])
def test_epoch_zero_is_the_actor_critic_step(row):
    """ratio = exp(0) = 1 at epoch 0, so the surrogate's gradient is the policy gradient's: the reference's epoch 0
    gives tests/a2c_ref.py's step, gradients, moments and parameters alike, to float64 rounding."""
    c = P.PPOCase(row)
    st, b = c.init_state(), c.batch()
    e = P.ppo_ref_epoch(c, st, b, None, None, P.F64)
    a = R.a2c_ref_step(c, st, b, R.F64)
    assert e.clipped == 0 and e.outside_kept == 0 and np.all(e.ratio == 1.0) and np.all(e.w)
    assert np.array_equal(e.ret, a.ret) and np.array_equal(e.V, a.V) and np.array_equal(e.critic_grads, a.critic_grads)
    scale = np.abs(a.agent_grads).max()
    assert np.abs(e.agent_grads - a.agent_grads).max() <= 1e-13 * scale
    assert np.abs(e.dlogits - a.dlogits).max() <= 1e-15
    for k in ("agent", "critic", "a_v", "c_v"):
        assert np.abs(e.new[k] - a.new[k]).max() <= 1e-12, k
    assert e.new["rew_ms"] == a.new["rew_ms"] and e.new["step"] == a.new["step"] == 1
    for k in R.STATS:
        if k != "pg_loss":   # -(adv + ec H), not -(adv log pi_u + ec H)
            assert abs(e.stats[k] - a.stats[k]) <= 1e-12 * max(1.0, abs(a.stats[k])), k


# ------------------------------------------------------------------------------------------ seeds
@pytest.mark.parametrize("row", list(P.ROWS))
def test_seed_conditions(row):
    rep = P.seed_report(row)
    assert P.seed_ok(row, rep) == [], (row, rep)
    c = P.PPOCase(row)
    assert len(rep["clipped"]) == c.epochs and rep["clipped"][0] == 0   # epoch 0 cuts nothing: ratio = 1
    if row == "default":
        assert (c.eps_clip, c.epochs) == (0.2, 4) and not any(rep["clipped"]) and not any(rep["outside_kept"])
    else:
        assert (c.eps_clip, c.epochs) == (0.01, 3) and rep["clipped"][-1] > 0   # the clipped branch runs on every row


def test_clip_range_is_formed_as_the_host_forms_it():
    c = P.PPOCase("part")
    e32 = np.float32(0.01)
    assert c.lo == float(np.float32(1.0 - float(e32))) and c.hi == float(np.float32(1.0 + float(e32)))
    assert c.lo == float(np.float32(c.lo)) and c.hi == float(np.float32(c.hi))


# ------------------------------------------------------------------------------------------ checkpoints
@pytest.mark.parametrize("row", ["part", "part_n10"])
def test_checkpoint_round_trip_on_cpu_tensors(row, tmp_path):
    c = P.PPOCase(row)
    _, _, _, learner, _ = build_ppo(c, device="cpu")
    rng = np.random.Generator(np.random.PCG64(1))
    with th.no_grad():   # a state as two train() calls of three epochs would have left it
        for name in ("_asq", "_csq", "_am", "_cm"):
            t = getattr(learner, name)
            if t is not None:
                t.copy_(th.tensor(rng.random(t.numel()), dtype=th.float32))
        learner._opt_steps = 6
        learner._step_t += 6
        if learner.rew_ms is not None:
            learner.rew_ms.copy_(th.tensor([0.4, 0.09, 36.0001], dtype=th.float64))
    learner.save_models(str(tmp_path))
    files = {"agent.th", "critic.th", "agent_opt.th", "critic_opt.th"} | ({"rew_ms.th"} if learner.rew_ms is not None
                                                                         else set())
    assert set(os.listdir(tmp_path)) == files   # the actor-critic learner's files: nothing new is checkpointed
    _, _, _, fresh, _ = build_ppo(P.PPOCase(row, seed=c.seed + 7), device="cpu")
    fresh.load_models(str(tmp_path))
    a, b = all_buffers(learner), all_buffers(fresh)
    for k in a:
        if k not in ("_agrad", "_cgrad"):
            assert np.array_equal(a[k], b[k]), k
    assert fresh._opt_steps == 6 and float(fresh.critic_optimiser.state[fresh.critic_params[0]]["step"]) == 6.0
    if learner.rew_ms is not None:
        assert th.equal(fresh.rew_ms, learner.rew_ms)
