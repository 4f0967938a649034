"""NonSharedMAC: epymarl's non-shared controller (`mac: non_shared_mac`, src/controllers/non_shared_controller.py) for
`agent: rnn_ns`: every agent has its own network (modules/agents/rnn_ns_agent.py).

BasicMAC's interface, input building (`obs_last_action`, `obs_agent_id`, the three replay routes), policy (`pi_logits`
with `soft_policies`, through `mc_policy`) and `agent.th` checkpoint. `forward(ep_batch, t)` is one launch of the
grouped forward kernel (`ma_actor_ns_forward`, pymarl_amd/csrc/ffn_actor_ns_kernels.hpp) over the B n rows of the step:
each 64-row tile holds one agent's rows and runs through that agent's weights. It serves the actor-critic and PPO
learners; `agent` other than `rnn_ns`, `learner: coma_learner` and `learner: q_learner` are refused.
"""
import torch as th

from .. import _lib
from ..modules.agents.rnn_agent import hidden_dim
from .basic_controller import BasicMAC

LEARNERS = ("actor_critic_learner", "ppo_learner")


class NonSharedMAC(BasicMAC):
    def __init__(self, scheme, groups, args):
        if getattr(args, "agent", None) != "rnn_ns":
            raise ValueError("mac: non_shared_mac needs agent: rnn_ns, got agent: {!r}.".format(
                getattr(args, "agent", None)))
        learner = getattr(args, "learner", None)
        if learner is not None and learner not in LEARNERS:
            raise ValueError("mac: non_shared_mac is not supported with learner: {} (one of {}): non-shared agents are "
                             "built for the actor-critic and PPO learners only.".format(learner, ", ".join(LEARNERS)))
        super().__init__(scheme, groups, args)

    def _forward(self, ep_batch, t, test_mode=False):
        flat = self.agent.flat_params()
        h = th.empty(self.n_agents, ep_batch.batch_size, hidden_dim(self.args), dtype=th.float32, device=flat.device)
        out = self._forward_ma(ep_batch, t, test_mode, "ma_actor_ns_forward", self._ma_config(_lib.AGENT_FFN_NS, 64),
                               flat, h)
        self.hidden_states = h.permute(1, 0, 2)   # (bs, n, H): the kernel writes it agent-major
        return out
