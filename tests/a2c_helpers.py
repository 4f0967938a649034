"""Build the actor-critic learner on a tests/a2c_ref.py case (same data and weights as the reference's state)."""
from __future__ import annotations

from types import SimpleNamespace as SN

import numpy as np

from tests.gpu_helpers import build_learner, load_actor_critic


def make_a2c_args(case, **over):
    k = case.keys
    a = SN(n_agents=case.n, n_actions=case.A, state_shape=case.S, obs_shape=case.O, rnn_hidden_dim=64,
           hidden_dim=k["hidden_dim"], lr=k["lr"], optim_alpha=k["optim_alpha"], optim_eps=k["optim_eps"],
           grad_norm_clip=k["grad_norm_clip"], gamma=k["gamma"], target_update_interval=200, learner_log_interval=0,
           obs_last_action=k["obs_last_action"], obs_agent_id=True, agent="rnn", mac="basic_mac",
           agent_output_type="pi_logits", action_selector="soft_policies", mask_before_softmax=k["mask_before_softmax"],
           critic_type=k["critic_type"], q_nstep=k["q_nstep"], add_value_last_step=k["add_value_last_step"],
           entropy_coef=k["entropy_coef"], optimizer=k["optimizer"], standardise_rewards=k["standardise_rewards"],
           batch_size=case.B, learner="actor_critic_learner", device="cuda", use_cuda=True)
    for key, v in over.items():
        setattr(a, key, v)
    return a


def build_a2c(case, device="cuda", data=None, **over):
    out = build_learner(case, make_a2c_args(case, **over), "actor_critic_learner", "ma-test", device, data=data)
    load_actor_critic(case, out[2], out[3])
    return out


def learner_state(learner):
    """The learner's state in tests/a2c_ref.py's layout: flat float32 numpy copies, the Adam step count, the running
    reward statistics."""
    f = lambda t: None if t is None else t.detach().cpu().numpy().copy()   # noqa: E731
    Pa, Pc = learner.n_agent_params, learner.n_critic_params
    z = lambda n: np.zeros(n, np.float32)   # noqa: E731
    am, cm = f(learner._am), f(learner._cm)
    rew = tuple(learner.rew_ms.tolist()) if learner.rew_ms is not None else (0.0, 1.0, 1e-4)
    return dict(agent=f(learner._agent)[:Pa], critic=f(learner._critic)[:Pc], target=f(learner._tcritic)[:Pc],
                a_m=z(Pa) if am is None else am, a_v=f(learner._asq), c_m=z(Pc) if cm is None else cm,
                c_v=f(learner._csq), step=int(learner._opt_steps), rew_ms=rew)


def all_buffers(learner):
    """Every device buffer a train() may write, as numpy copies (the bitwise tests): parameters, target, gradients,
    moments, and the running reward statistics when the learner keeps them."""
    names = ("_agent", "_critic", "_tcritic", "_agrad", "_asq", "_cgrad", "_csq", "_am", "_cm", "rew_ms")
    return {k: getattr(learner, k).detach().cpu().numpy().copy() for k in names if getattr(learner, k) is not None}
