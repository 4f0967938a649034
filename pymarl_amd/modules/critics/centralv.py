"""The V critics of the actor-critic learner (epymarl's `cv_critic` and `ac_critic`).

fc1 (K -> Hc) -> ReLU -> fc2 (Hc -> Hc) -> ReLU -> fc3 (Hc -> 1), Hc = `args.hidden_dim` (64 or 128), one value per
(episode, step, agent) row. `parameters()` order and state_dict names are fc1.weight .. fc3.bias. The per-row input:

* CentralVCritic (`cv_critic`): state | the last joint one-hot actions of all agents, when `obs_last_action` (zero at
  t = 0 and behind unfilled slots) | one-hot agent id;
* ACCritic (`ac_critic`, modules/critics/ac.py): the row's own obs | one-hot agent id.

Inside ActorCriticLearner.train the critic runs as HIP kernels on this module's flat parameter buffer
(include/ma_a2c.h). `forward(batch, t=None)` is the standalone HIP path `ma_critic_forward`; it returns values, not an
autograd graph. `build_inputs` restates the input in torch (any device): the tests compare the kernels' X against it.
"""
import torch as th
import torch.nn as nn

from ... import _lib
from ...components.episode_buffer import replay_view
from ..flat import FlatModule

CRITIC_WIDTHS = (64, 128)


def _width(v):
    return v if isinstance(v, int) else int(v[0])


def critic_hidden(args):
    """The critic's hidden width: `hidden_dim` (epymarl's key), 64 when absent; 64 or 128."""
    v = getattr(args, "hidden_dim", None)
    v = 64 if v is None else v
    if isinstance(v, bool) or v not in CRITIC_WIDTHS:
        raise ValueError("hidden_dim (the critic's width) must be 64 or 128, got {!r}.".format(v))
    return int(v)


class VCritic(FlatModule):
    KIND = None   # _lib.MA_CRITIC_*

    def __init__(self, scheme, args):
        super().__init__()
        self.args = args
        self.n_actions = args.n_actions
        self.n_agents = args.n_agents
        self.state_dim = _width(scheme["state"]["vshape"])
        self.obs_dim = _width(scheme["obs"]["vshape"])
        self.obs_last_action = bool(getattr(args, "obs_last_action", False))
        self.hidden_dim = critic_hidden(args)
        self.input_dim = self._input_dim()
        self.output_type = "v"
        self.fc1 = nn.Linear(self.input_dim, self.hidden_dim)
        self.fc2 = nn.Linear(self.hidden_dim, self.hidden_dim)
        self.fc3 = nn.Linear(self.hidden_dim, 1)
        self._init_flat()

    def _input_dim(self):
        raise NotImplementedError

    def build_inputs(self, batch, t=None):
        raise NotImplementedError

    def _ids(self, bs, tq, device):
        return th.eye(self.n_agents, device=device).unsqueeze(0).unsqueeze(0).expand(bs, tq, -1, -1)

    def _config(self):
        cfg = _lib.MAConfig()
        cfg.n_agents, cfg.n_actions = self.n_agents, self.n_actions
        cfg.obs_dim, cfg.state_dim = self.obs_dim, self.state_dim
        cfg.rnn_hidden_dim = 64
        cfg.critic_hidden = self.hidden_dim
        cfg.critic_type = self.KIND
        cfg.obs_last_action = int(self.obs_last_action)
        return cfg

    def forward(self, batch, t=None):
        """v (bs, max_t, n_agents, 1) for every stored step (t=None) or step t (max_t = 1)."""
        rep, keep = replay_view(batch)
        _lib.require_gpu(self._flat)
        tq = rep.t_len if t is None else 1
        if t is not None and not (0 <= int(t) < rep.t_len):
            raise IndexError("t={} outside the batch's {} steps".format(t, rep.t_len))
        cfg = self._config()
        lib = _lib.load()
        n_ws = lib.ma_critic_forward_workspace(cfg, batch.batch_size, tq)
        ws = th.empty(max(int(n_ws), 1), dtype=th.float32, device=self._flat.device)
        v = th.empty(batch.batch_size, tq, self.n_agents, 1, dtype=th.float32, device=self._flat.device)
        _lib.check(lib.ma_critic_forward(_lib.ptr(self._flat), cfg, rep, -1 if t is None else int(t), _lib.ptr(v),
                                         _lib.ptr(ws), _lib.stream_ptr()))
        del keep
        return v


class CentralVCritic(VCritic):
    KIND = _lib.MA_CRITIC_CV

    def _input_dim(self):
        return self.state_dim + (self.n_agents * self.n_actions if self.obs_last_action else 0) + self.n_agents

    def build_inputs(self, batch, t=None):
        """(bs, max_t, n_agents, K) in torch, on the batch's device."""
        bs, n = batch.batch_size, self.n_agents
        max_t = batch.max_seq_length if t is None else 1
        ts = slice(None) if t is None else slice(t, t + 1)
        parts = [batch["state"][:, ts].unsqueeze(2).expand(-1, -1, n, -1)]
        if self.obs_last_action:
            oh = batch["actions_onehot"] * batch["filled"].unsqueeze(2).to(batch["actions_onehot"].dtype)
            last = th.cat([th.zeros_like(oh[:, 0:1]), oh[:, :-1]], dim=1)[:, ts]
            parts.append(last.reshape(bs, max_t, 1, -1).expand(-1, -1, n, -1))
        parts.append(self._ids(bs, max_t, batch["state"].device))
        return th.cat([p.float() for p in parts], dim=-1)
