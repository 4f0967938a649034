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
from ..components.episode_buffer import replay_view
from ..modules.agents.rnn_agent import hidden_dim, obs_dim
from .basic_controller import BasicMAC, _on_device

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
        self._ws = None

    def _config(self):
        cfg = _lib.MAConfig()
        a = self.args
        cfg.n_agents, cfg.n_actions = a.n_agents, a.n_actions
        cfg.obs_dim = obs_dim(a, self.agent.input_dim)
        cfg.state_dim, cfg.rnn_hidden_dim, cfg.critic_hidden, cfg.critic_type = 1, 64, 64, _lib.MA_CRITIC_CV
        cfg.obs_last_action, cfg.obs_agent_id = int(bool(a.obs_last_action)), int(bool(a.obs_agent_id))
        cfg.agent = _lib.AGENT_FFN_NS
        return cfg

    def _forward(self, ep_batch, t, test_mode=False):
        if self.agent_output_type != "pi_logits":
            raise NotImplementedError("agent_output_type {!r}".format(self.agent_output_type))
        flat = self.agent.flat_params()
        _lib.require_gpu(flat)
        dev, t_run = flat.device, t
        ep_view = ep_batch
        if not _on_device(ep_batch):   # host-resident (buffer_cpu_only): the step's rows to the device
            ep_view, t_run = self._device_step(ep_batch, t, dev)
        rep, keep = replay_view(ep_view)
        bs, n, H = ep_batch.batch_size, self.n_agents, hidden_dim(self.args)
        lib, cfg = _lib.load(), self._config()
        need = lib.ma_actor_ns_forward_workspace(cfg, bs)
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = th.empty(need, dtype=th.float32, device=dev)
        q = th.empty(bs * n, self.args.n_actions, dtype=th.float32, device=dev)
        h = th.empty(n, bs, H, dtype=th.float32, device=dev)
        _lib.check(lib.ma_actor_ns_forward(_lib.ptr(flat), cfg, rep, int(t_run), _lib.ptr(q), _lib.ptr(h),
                                           _lib.ptr(self._ws), _lib.stream_ptr()))
        del keep
        self.hidden_states = h.permute(1, 0, 2)   # (bs, n, H): the kernel writes it agent-major
        avail = ep_batch["avail_actions"][:, t].to(device=dev, dtype=th.int32).contiguous()
        eps = float(getattr(self.action_selector, "epsilon", 0.0))   # soft_policies has none: no floor
        _lib.check(lib.mc_policy(_lib.ptr(q), _lib.ptr(avail), q.shape[0], q.shape[1], eps,
                                 int(bool(getattr(self.args, "mask_before_softmax", True))), int(bool(test_mode)),
                                 _lib.stream_ptr()))
        return q.view(bs, n, -1)
