"""DMAQer: the QPLEX duplex-dueling mixer (pymarl2's `mixer: dmaq`, its dmaq_general.DMAQer with
`adv_hypernet_layers: 1`), MI355X-native.

Holds the parameters under pymarl2's names (hyper_w_final.{0,2}, V.{0,2}, si_weight.key_extractors.<k>,
si_weight.agents_extractors.<k>, si_weight.action_extractors.<k>) in its parameters() order, so mixer.th interchanges.
Inside QLearner.train the mixer runs fused into the HIP train step (csrc/dmaq_kernels.hpp: every state-fed product as one
MFMA GEMM, the mix and its backward in dmaq_mix_kernel, every weight gradient as one split GEMM);
`forward(agent_qs, states, actions, max_q_i, is_v)` is the standalone HIP kernel `mq_dmaq_forward`
(include/mq_learner.h). It returns values, not an autograd graph.

Keys and defaults (pymarl2's qplex.yaml as recalled; no copy of pymarl2 was at hand): hypernet_embed 64, num_kernel 4,
adv_hypernet_layers 1, adv_hypernet_embed 64 (not read at one layer), is_minus_one True, weighted_head True,
is_stop_gradient True. Only adv_hypernet_layers 1 and is_stop_gradient True are built.
"""
import ctypes

import numpy as np
import torch as th
import torch.nn as nn

from ... import _lib
from ..flat import FlatModule


def dmaq_config(args):
    """The DMAQ keys of `args`, validated: dict(hypernet_embed, num_kernel, weighted_head, is_minus_one). Every refusal
    is a ValueError naming its key, raised before any library call."""
    he = int(getattr(args, "hypernet_embed", 64))
    nk = int(getattr(args, "num_kernel", 4))
    if getattr(args, "hypernet_layers", 1) == 2:
        raise ValueError("hypernet_layers: 2 is QMIX's two-layer hypernet; mixer: dmaq takes hypernet_layers: 1")
    if int(getattr(args, "adv_hypernet_layers", 1)) != 1:
        raise ValueError("adv_hypernet_layers {} is not built: only 1".format(args.adv_hypernet_layers))
    if not bool(getattr(args, "is_stop_gradient", True)):
        raise ValueError("is_stop_gradient False is not built: only True")
    if not 1 <= nk <= _lib.DMAQ_KERNEL_MAX:
        raise ValueError("num_kernel {} is outside the kernels' limit: 1 to {}".format(nk, _lib.DMAQ_KERNEL_MAX))
    if not 1 <= he <= _lib.HYPERNET_EMBED_MAX:
        raise ValueError("hypernet_embed {} is outside the kernels' limit: 1 to {}".format(he, _lib.HYPERNET_EMBED_MAX))
    if not 1 <= int(args.n_agents) <= _lib.DMAQ_AGENTS_MAX:
        raise ValueError("n_agents {} is outside mixer: dmaq's limit: 1 to {}".format(args.n_agents,
                                                                                      _lib.DMAQ_AGENTS_MAX))
    return dict(hypernet_embed=he, num_kernel=nk, weighted_head=bool(getattr(args, "weighted_head", True)),
                is_minus_one=bool(getattr(args, "is_minus_one", True)))


class SIWeight(nn.Module):
    """pymarl2's DMAQ_SI_Weight at adv_hypernet_layers = 1: per head a key, an agents and an action extractor."""

    def __init__(self, state_dim, n_agents, n_actions, num_kernel):
        super().__init__()
        self.key_extractors = nn.ModuleList(nn.Linear(state_dim, 1) for _ in range(num_kernel))
        self.agents_extractors = nn.ModuleList(nn.Linear(state_dim, n_agents) for _ in range(num_kernel))
        self.action_extractors = nn.ModuleList(nn.Linear(state_dim + n_agents * n_actions, n_agents)
                                               for _ in range(num_kernel))


class DMAQer(FlatModule):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.n_agents = args.n_agents
        self.n_actions = args.n_actions
        self.state_dim = int(np.prod(args.state_shape))
        cfg = dmaq_config(args)
        self.hypernet_embed, self.num_kernel = cfg["hypernet_embed"], cfg["num_kernel"]
        self.weighted_head, self.is_minus_one = cfg["weighted_head"], cfg["is_minus_one"]
        he = self.hypernet_embed
        self.hyper_w_final = nn.Sequential(nn.Linear(self.state_dim, he), nn.ReLU(), nn.Linear(he, self.n_agents))
        self.V = nn.Sequential(nn.Linear(self.state_dim, he), nn.ReLU(), nn.Linear(he, self.n_agents))
        self.si_weight = SIWeight(self.state_dim, self.n_agents, self.n_actions, self.num_kernel)
        self._init_flat()

    def dmaq_struct(self):
        """The module's mq_dmaq (mq_set_dmaq, mq_dmaq_forward)."""
        return _lib.MQDmaq(num_kernel=self.num_kernel, hypernet_embed=self.hypernet_embed,
                           weighted_head=int(self.weighted_head), is_minus_one=int(self.is_minus_one))

    def forward(self, agent_qs, states, actions=None, max_q_i=None, is_v=False):
        """agent_qs (bs, T, n_agents), states (bs, T, state_dim) and, unless is_v, actions (bs, T, n_agents, n_actions)
        one-hot and max_q_i (bs, T, n_agents) -> (bs, T, 1): V_tot when is_v, else A_tot."""
        bs = agent_qs.size(0)
        flat = lambda x, w: x.detach().reshape(-1, w).float().contiguous()  # noqa: E731
        qs, st = flat(agent_qs, self.n_agents), flat(states, self.state_dim)
        _lib.require_gpu(qs)
        _lib.require_gpu(self._flat)
        rows = qs.shape[0]
        if st.shape[0] != rows:
            raise ValueError("agent_qs has {} rows but states has {}".format(rows, st.shape[0]))
        act = mx = None
        if not is_v:
            if actions is None or max_q_i is None:
                raise ValueError("DMAQer.forward needs actions and max_q_i unless is_v")
            act, mx = flat(actions, self.n_agents * self.n_actions), flat(max_q_i, self.n_agents)
            if act.shape[0] != rows or mx.shape[0] != rows:
                raise ValueError("actions / max_q_i do not have agent_qs' {} rows".format(rows))
        out = th.empty(rows, dtype=th.float32, device=qs.device)
        q = self.dmaq_struct()
        _lib.check(_lib.load().mq_dmaq_forward(_lib.ptr(self._flat), ctypes.byref(q), self.n_agents, self.n_actions,
                                               self.state_dim, _lib.ptr(qs), _lib.ptr(st), _lib.ptr(act), _lib.ptr(mx),
                                               int(bool(is_v)), _lib.ptr(out), rows, _lib.stream_ptr()))
        return out.view(bs, -1, 1)
