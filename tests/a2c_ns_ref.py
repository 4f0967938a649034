"""tests/a2c_ref.py's and tests/ppo_ref.py's restatements with the non-shared actor (agent: rnn_ns): the
actor is `RefNSAgent`, a plain torch ModuleList of n feed-forward agents, row (b, g) through agents[g], differentiated
by autograd and stepped by a real torch.optim over all n Pa1 parameters under one clip_grad_norm_.

a2c_ref_step / ppo_ref_epoch / judge / judge_updates serve as they are inside `with non_shared():`, which puts
`ns_unroll` and `ns_grad_blocks` in ref64.unroll's and ref64.grad_blocks' places for its duration (both are looked up
at call time). A block is per agent and per tensor (fc1.weight also by input kind), so one agent's gradient landing in
another's region cannot pass.

A seed is valid when every kink minimum (the critic's two relus and every agent's two) stays above ref64.KINK_EPS at
both steps, the float32 run's update standing in for the GPU's; the PPO rows add tests/a2c_ffn_ref.py's conditions at
each of the four epochs. `python -m tests.a2c_ns_ref` prints the first valid seed of 0..63 per row. `ns_walk` keeps all
but one episode short, as §3k's `split` does: 320 full-length rows per agent leave no seed above the margin."""
import contextlib
from collections import OrderedDict

import torch as th
from torch import nn

from pymarl_amd.utils.synthetic import init_params
from tests import a2c_ffn_ref as F
from tests import a2c_ref as R
from tests import ppo_ref as PR
from tests import ref64
from tests.ffn_ref import RefFFAgent, ff_agent_shapes

_PART = R._PART
_WALK = (16, 2, 1, 3) + (1,) * 16
# TB = T B rows per agent in 64-row tiles; I = O + A + n
ROWS = OrderedDict([
    ("ns_part", dict(n=3, A=5, t_len=10, S=7, O=5, B=2, lengths=(9, 4), seed=0)),               # TB = 18
    ("ns_tile64", dict(n=2, A=5, t_len=17, S=7, O=5, B=4, lengths=(16, 2, 1, 3), seed=0)),       # TB = 64
    ("ns_tile65", dict(n=2, A=5, t_len=14, S=7, O=5, B=5, lengths=(13, 2, 1, 3, 1), seed=0)),    # TB = 65
    ("ns_walk", dict(n=3, A=5, t_len=17, S=7, O=5, B=20, lengths=_WALK, seed=1)),                # TB = 320: five tiles
    ("ns_n10", dict(n=10, A=18, t_len=4, S=7, O=5, B=2, lengths=(3, 1), seed=1)),                # cfg5's n and A
    ("ns_A33", dict(_PART, A=33, seed=2)),
    ("ns_wideI", dict(_PART, O=256, seed=0)),   # I = 264 > 248: W1 streamed, per agent
])
PPO_SEEDS = dict(ns_part=10, ns_walk=1)
PPO_KEYS = dict(PR.CLIP, epochs=4)


class RefNSAgent(nn.Module):
    """epymarl's RNNNSAgent with use_rnn = False, restated: x (..., n, I) -> logits (..., n, A), h, and the two relus'
    pre-activations (..., n, H)."""

    def __init__(self, n, input_dim, n_actions):
        super().__init__()
        self.agents = nn.ModuleList([RefFFAgent(input_dim, n_actions) for _ in range(n)])

    def forward(self, x):
        outs = []
        for g, a in enumerate(self.agents):
            pre1 = a.fc1(x[..., g, :])
            pre2 = a.rnn(th.relu(pre1))
            h = th.relu(pre2)
            outs.append((a.fc2(h), h, pre1, pre2))
        return tuple(th.stack(z, -2) for z in zip(*outs))


def ns_unroll(p, obs, onehot, flags, dtype, relu_mask=None, hid_mask=None):
    """ref64.unroll's contract for parameters named agents.<g>.*: (logits, fc1 pre-activations, second relu's)."""
    B, Tp, n, _ = obs.shape
    parts = [obs]
    if flags[0]:
        parts.append(th.cat([th.zeros_like(onehot[:, :1]), onehot[:, :-1]], 1))
    if flags[1]:
        parts.append(th.eye(n, dtype=dtype).expand(B, Tp, n, n))
    x = th.cat(parts, -1)
    mod = RefNSAgent(n, x.shape[-1], onehot.shape[-1])
    logits, _, pre1, pre2 = th.func.functional_call(mod, dict(p), (x,))
    return logits, pre1, pre2


def ns_grad_blocks(view):
    """ref64.grad_blocks' table per agent: every tensor of agents.<g>, and its fc1.weight by input kind."""
    blocks, full = OrderedDict(), slice(None)
    for k in view.agent_shapes:
        blocks[k] = (k, (full,))
    for g in range(view.n):
        w, o = "agents.{}.fc1.weight".format(g), 0
        kinds = [("obs", view.O)] + ([("last_action", view.A)] if view.obs_last_action else []) + [("agent_id", view.n)]
        for kind, width in kinds:
            blocks["{}[{}]".format(w, kind)] = (w, (full, slice(o, o + width)))
            o += width
    return blocks


@contextlib.contextmanager
def non_shared():
    keep = ref64.unroll, ref64.grad_blocks
    ref64.unroll, ref64.grad_blocks = ns_unroll, ns_grad_blocks
    try:
        yield
    finally:
        ref64.unroll, ref64.grad_blocks = keep


def _ns(case):
    ff = ff_agent_shapes(case.I, case.A)
    name = "agents.{}.{}".format
    case.agent_shapes = OrderedDict((name(g, k), s) for g in range(case.n) for k, s in ff.items())
    case.agent_params = OrderedDict((name(g, k), v) for g in range(case.n)
                                    for k, v in init_params(ff, seed=case.seed + 1 + g).items())


class A2CNSCase(R.A2CCase):
    def __init__(self, row, seed=None):
        R.ROWS["_ns"] = ROWS[row]   # A2CCase reads its row from a2c_ref.ROWS
        try:
            super().__init__("_ns", seed)
        finally:
            del R.ROWS["_ns"]
        self.row = row
        _ns(self)


class PPONSCase(PR.PPOCase):
    def __init__(self, row, seed=None):
        R.ROWS["_ns"], PR.ROWS["_ns"] = ROWS[row], dict(PPO_KEYS, base="_ns", seed=PPO_SEEDS[row])
        try:
            super().__init__("_ns", seed)
        finally:
            del R.ROWS["_ns"], PR.ROWS["_ns"]
        self.row = row
        _ns(self)


def seed_minimum(case, ppo):
    with non_shared():
        return F.seed_minimum(case, ppo)


def build_ns(case, learner="actor_critic_learner", device="cuda", **over):
    """tests/gpu_helpers.build_learner through `mac: non_shared_mac`: (args, replay, mac, learner) on the case's data and
    weights."""
    import logging

    from tests import gpu_helpers as G
    from tests.a2c_helpers import make_a2c_args
    from tests.ppo_helpers import make_ppo_args
    keys = dict(dict(agent="rnn_ns", mac="non_shared_mac", use_rnn=False, learner=learner), **over)
    args = (make_ppo_args if learner == "ppo_learner" else make_a2c_args)(case, **keys)
    groups = {"agents": case.n}
    buf = G.ReplayBuffer(G.make_scheme(case), groups, case.n_episodes, case.T + 1, device=device,
                         preprocess={"actions": ("actions_onehot", [G.OneHot(out_dim=case.A)])})
    buf.load_arrays(case.data)
    mac = G.mac_REGISTRY[args.mac](buf.scheme, groups, args)
    made = G.le_REGISTRY[learner](mac, buf.scheme, G.Logger(logging.getLogger("ns-test")), args)
    if device != "cpu":
        made.cuda()
    G.load_actor_critic(case, mac, made)
    return args, buf, mac, made


if __name__ == "__main__":
    for ppo, rows, mk in ((False, ROWS, A2CNSCase), (True, PPO_SEEDS, PPONSCase)):
        for row in rows:
            ok = next(((s, v) for s in range(64) for v in [seed_minimum(mk(row, s), ppo)] if v > R.MARGIN), None)
            print("ppo" if ppo else "a2c", row, "first valid seed (minimum):", ok or "none in 0..63", flush=True)
