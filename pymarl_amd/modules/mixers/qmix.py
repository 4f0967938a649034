"""QMixer: state-conditioned monotonic mixing (reference: src/modules/mixers/qmix.py:7-47).

Holds the hypernetwork parameters under the reference's names (hyper_w_1, hyper_w_final, hyper_b_1, V.0, V.2)
so mixer.th interchanges. Inside QLearner.train the forward/backward run fused into the HIP train step (hypernet
contraction on fp32 MFMA, mixing + TD + backward in `mix_kernel`); `forward(agent_qs, states)` is the standalone
HIP kernel `mq_qmix_forward` (include/mq_learner.h) for callers outside train(). It returns values, not an
autograd graph (the learner computes the mixer's gradients itself).

`args.hypernet_layers` (default 1) and `args.hypernet_embed` (default 64) are upstream PyMARL's keys: with 2 layers
hyper_w_1 and hyper_w_final are Linear(S, hypernet_embed) -> ReLU -> Linear(hypernet_embed, .), under upstream's
state_dict keys (hyper_w_1.0.weight, hyper_w_1.2.weight, ..), so a mixer.th of either side loads on the other. The
train step then runs the hypernet as launches of its own (csrc/hyper2_kernels.hpp) and forward() is
`mq_qmix_forward2`.
"""
import numpy as np
import torch as th
import torch.nn as nn

from ... import _lib
from ..flat import FlatModule


def hypernet_config(args):
    """(hypernet_layers, hypernet_embed) of `args` as upstream reads them, validated."""
    layers = getattr(args, "hypernet_layers", 1)
    embed = getattr(args, "hypernet_embed", 64)
    if layers == 1:
        return 1, int(embed)
    if layers == 2:
        if not 1 <= int(embed) <= _lib.HYPERNET_EMBED_MAX:
            raise ValueError("hypernet_embed {} is outside the kernels' limit: 1 to {}".format(
                embed, _lib.HYPERNET_EMBED_MAX))
        return 2, int(embed)
    if isinstance(layers, (int, float)) and layers > 2:
        raise Exception("Sorry >2 hypernet layers is not implemented!")
    raise Exception("Error setting number of hypernet layers.")


class QMixer(FlatModule):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.n_agents = args.n_agents
        self.state_dim = int(np.prod(args.state_shape))
        self.embed_dim = args.mixing_embed_dim
        self.hypernet_layers, self.hypernet_embed = hypernet_config(args)
        if self.hypernet_layers == 1:
            self.hyper_w_1 = nn.Linear(self.state_dim, self.embed_dim * self.n_agents)
            self.hyper_w_final = nn.Linear(self.state_dim, self.embed_dim)
        else:
            he = self.hypernet_embed
            self.hyper_w_1 = nn.Sequential(nn.Linear(self.state_dim, he), nn.ReLU(),
                                           nn.Linear(he, self.embed_dim * self.n_agents))
            self.hyper_w_final = nn.Sequential(nn.Linear(self.state_dim, he), nn.ReLU(),
                                               nn.Linear(he, self.embed_dim))
        self.hyper_b_1 = nn.Linear(self.state_dim, self.embed_dim)
        self.V = nn.Sequential(nn.Linear(self.state_dim, self.embed_dim), nn.ReLU(), nn.Linear(self.embed_dim, 1))
        self._init_flat()

    def forward(self, agent_qs, states):
        """qmix.py:28-47: agent_qs (bs, T, n_agents), states (bs, T, state_dim) -> q_tot (bs, T, 1)."""
        bs = agent_qs.size(0)
        qs = agent_qs.detach().reshape(-1, self.n_agents).float().contiguous()
        st = states.detach().reshape(-1, self.state_dim).float().contiguous()
        _lib.require_gpu(qs)
        _lib.require_gpu(self._flat)
        rows = qs.shape[0]
        if st.shape[0] != rows:
            raise ValueError("agent_qs has {} rows but states has {}".format(rows, st.shape[0]))
        out = th.empty(rows, dtype=th.float32, device=qs.device)
        lib = _lib.load()
        if self.hypernet_layers == 2:
            _lib.check(lib.mq_qmix_forward2(_lib.ptr(self._flat), self.n_agents, self.state_dim, self.embed_dim,
                                            self.hypernet_embed, _lib.ptr(qs), _lib.ptr(st), _lib.ptr(out), rows,
                                            _lib.stream_ptr()))
        else:
            _lib.check(lib.mq_qmix_forward(_lib.ptr(self._flat), self.n_agents, self.state_dim, self.embed_dim,
                                           _lib.ptr(qs), _lib.ptr(st), _lib.ptr(out), rows, _lib.stream_ptr()))
        return out.view(bs, -1, 1)
