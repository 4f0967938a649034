"""RNNAgent: fc1 -> ReLU -> GRUCell -> fc2 (reference: src/modules/agents/rnn_agent.py:7-36).

Same submodules and parameter names (fc1, rnn, fc2), so state_dicts interchange with the reference. `forward`
runs the HIP `mq_agent_forward` kernel; inside the learner the whole unroll is fused into the train step.

Opt-in `use_rnn: False` (epymarl's key): `rnn` is then `nn.Linear(64, 64)` followed by a ReLU instead of the GRUCell,
    x1 = relu(fc1(inputs));  h = relu(rnn(x1));  q = fc2(h)
with the incoming hidden state ignored and `h` returned in its place; the state_dict is epymarl's (fc1.weight,
fc1.bias, rnn.weight, rnn.bias, fc2.weight, fc2.bias). Without the key, or with True, nothing changes.
"""
from collections import OrderedDict

import numpy as np
import torch as th
import torch.nn as nn

from ... import _lib
from ..flat import FlatModule
from ..mixers.qmix import hypernet_config

Q_TARGETS = ("one_step", "td_lambda")


def input_dim(input_shape):
    if isinstance(input_shape, (dict, OrderedDict)):
        return int(input_shape["1d"][0])
    if isinstance(input_shape, tuple):
        assert len(input_shape) == 1, "Input shape has unsupported dimensionality: {}".format(input_shape)
        return int(input_shape[0])
    return int(input_shape)


def use_rnn_config(args):
    """epymarl's use_rnn: True (or the key absent / None) is the GRU agent, False the feed-forward one. Not a bool:
    ValueError."""
    v = getattr(args, "use_rnn", True)
    if v is None:
        return True
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("use_rnn must be True or False, got {!r}.".format(v))
    return bool(v)


def hidden_dim(args):
    """The agent's hidden width: rnn_hidden_dim, or epymarl's hidden_dim when rnn_hidden_dim is absent."""
    v = getattr(args, "rnn_hidden_dim", None)
    if v is None:
        v = getattr(args, "hidden_dim", None)
    if v is None:
        raise AttributeError("args has neither rnn_hidden_dim nor hidden_dim")
    return int(v)


def agent_kind(args):
    """MQ_AGENT_* of the args (mq_config.agent)."""
    return _lib.AGENT_GRU if use_rnn_config(args) else _lib.AGENT_FFN


def obs_dim(args, width):
    """The observation's share of an agent input of `width` values (the last action and the agent id follow it)."""
    return int(width - (args.n_actions if args.obs_last_action else 0) - (args.n_agents if args.obs_agent_id else 0))


def state_dim(args):
    st = getattr(args, "state_shape", 1)
    return int(st if isinstance(st, int) else th.Size(st).numel())


def make_config(args, mixer, input_dim=None, max_batch=1, max_seq=2):
    """mq_config of `args` for the Q learner's step (learners/q_learner.py) or, with mixer MIXER_NONE, the agent's own
    inference handle."""
    cfg = _lib.MQConfig()
    cfg.n_agents = args.n_agents
    cfg.n_actions = args.n_actions
    obs = getattr(args, "obs_shape", None)
    if obs is None and input_dim is not None:
        obs = obs_dim(args, input_dim)
    cfg.obs_dim = int(obs)
    cfg.state_dim = state_dim(args)
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


class RNNAgent(FlatModule):
    def __init__(self, input_shape, args):
        super().__init__()
        self.args = args
        self.input_shape = input_shape
        self.input_dim = input_dim(input_shape)
        self.use_rnn = use_rnn_config(args)
        self.hidden_dim = hidden_dim(args)
        self.fc1 = nn.Linear(self.input_dim, self.hidden_dim)
        if self.use_rnn:
            self.rnn = nn.GRUCell(self.hidden_dim, self.hidden_dim)
        else:
            self.rnn = nn.Linear(self.hidden_dim, self.hidden_dim)
        self.fc2 = nn.Linear(self.hidden_dim, args.n_actions)
        self._init_flat()
        self._handle = None

    def init_hidden(self):
        return self.fc1.weight.new_zeros(1, self.hidden_dim)

    def handle(self):
        """Inference handle (agent-only layout) bound to this module's flat parameters."""
        if self._handle is None or self._handle[1] != self._flat.data_ptr():
            cfg = make_config(self.args, mixer=_lib.MIXER_NONE, input_dim=self.input_dim, max_batch=1, max_seq=2)
            h = _lib.Handle(cfg)
            _lib.check(h.lib.mq_bind(h.h, _lib.ptr(self._flat), None, None, None, None, None))
            self._handle = (h, self._flat.data_ptr())
        return self._handle[0]

    def forward(self, inputs, hidden_state=None):
        if isinstance(inputs, (dict, OrderedDict)):
            inputs = inputs["1d"]
        _lib.require_gpu(inputs)
        x = inputs.reshape(-1, self.input_dim).float().contiguous()
        q = th.empty(x.shape[0], self.args.n_actions, dtype=th.float32, device=x.device)
        hd = self.handle()
        if self.use_rnn:
            h_in = hidden_state.reshape(-1, self.hidden_dim).float().contiguous()
            h_out = th.empty_like(h_in)
        else:   # any hidden_state: it is not read
            h_in = None
            h_out = th.empty(x.shape[0], self.hidden_dim, dtype=th.float32, device=x.device)
        _lib.check(hd.lib.mq_agent_forward(hd.h, _lib.ptr(x), x.shape[0], _lib.ptr(h_in), _lib.ptr(h_out),
                                           _lib.ptr(q), 0, _lib.stream_ptr()))
        return q, h_out

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_handle"] = None
        return d
