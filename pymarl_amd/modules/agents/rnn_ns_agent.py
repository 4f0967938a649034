"""RNNNSAgent: epymarl's non-shared agent (`agent: rnn_ns`, src/modules/agents/rnn_ns_agent.py), one network per agent.

`self.agents` is a ModuleList of n_agents plain agents, so the state_dict is epymarl's (`agents.<g>.fc1.weight`,
`agents.<g>.fc1.bias`, `agents.<g>.rnn.weight`, `agents.<g>.rnn.bias`, `agents.<g>.fc2.weight`, `agents.<g>.fc2.bias`)
and `parameters()` runs agent by agent: the flat buffer is n_agents copies of the feed-forward agent's layout, one after
another. Row (b, g) of the input goes through `agents[g]`:
    x1 = relu(fc1_g(inputs));  h = relu(rnn_g(x1));  logits = fc2_g(h)
Only `use_rnn: False` is built: the non-shared GRU actor is not. The module holds the parameters; the
forward is NonSharedMAC's (one grouped HIP kernel over the B n rows of a step, pymarl_amd/csrc/ffn_actor_ns_kernels.hpp)
and the learners' (the same kernel over every step of the batch). There is no eager path.
"""
import torch.nn as nn

from ..flat import FlatModule
from .rnn_agent import hidden_dim, input_dim, use_rnn_config


class _Agent(nn.Module):
    """One agent's parameters, under RNNAgent's names."""

    def __init__(self, width, hidden, n_actions):
        super().__init__()
        self.fc1 = nn.Linear(width, hidden)
        self.rnn = nn.Linear(hidden, hidden)
        self.fc2 = nn.Linear(hidden, n_actions)


class RNNNSAgent(FlatModule):
    non_shared = True
    use_rnn = False

    def __init__(self, input_shape, args):
        super().__init__()
        if getattr(args, "use_rnn", None) is None or use_rnn_config(args):
            raise ValueError("agent: rnn_ns needs use_rnn: False, got use_rnn: {!r}: the non-shared GRU actor is not "
                             "built.".format(getattr(args, "use_rnn", None)))
        self.args = args
        self.input_shape = input_shape
        self.input_dim = input_dim(input_shape)
        self.hidden_dim = hidden_dim(args)
        self.n_agents = args.n_agents
        self.agents = nn.ModuleList([_Agent(self.input_dim, self.hidden_dim, args.n_actions)
                                     for _ in range(self.n_agents)])
        self._init_flat()

    def init_hidden(self):
        return self._flat.new_zeros(1, self.hidden_dim)

    def forward(self, inputs, hidden_state=None):
        raise NotImplementedError("RNNNSAgent has no forward of its own: NonSharedMAC.forward runs the grouped kernel")
