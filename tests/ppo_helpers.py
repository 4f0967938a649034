"""Build the PPO learner on a tests/ppo_ref.py case (same data and weights as the reference's state)."""
from __future__ import annotations

from tests.a2c_helpers import make_a2c_args
from tests.gpu_helpers import build_learner, load_actor_critic


def make_ppo_args(case, **over):
    kw = dict(learner="ppo_learner", epochs=case.epochs, eps_clip=case.eps_clip)
    kw.update(over)
    return make_a2c_args(case, **kw)


def build_ppo(case, device="cuda", data=None, **over):
    out = build_learner(case, make_ppo_args(case, **over), "ppo_learner", "ppo-test", device, data=data)
    load_actor_critic(case, out[2], out[3])
    return out


def build_a2c_on(case, device="cuda", **over):
    """ActorCriticLearner on the same case (its keys without the two PPO ones): the `epochs: 1` comparison."""
    out = build_learner(case, make_a2c_args(case, **over), "actor_critic_learner", "ma-test", device)
    load_actor_critic(case, out[2], out[3])
    return out
