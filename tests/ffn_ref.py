"""The feed-forward agent (use_rnn: False, epymarl's key): its restated module and its cases, torch on the CPU.

* `RefFFAgent`: epymarl's RNNAgent with use_rnn = False restated (rnn = nn.Linear(64, 64), a ReLU behind it, the
  incoming hidden state ignored), the module the state_dict interchange and the acting path are judged by.
* `SynthCaseF`: a SynthCase with the feed-forward agent's shapes, weights and `unflatten`.

The step's reference is tests/ref64.ref_step, which reads the agent from the case's parameter names and the mixer
from `mixer` / `He`. In float64 it is the reference; in float32 its error against the float64 run is `e32`, the role
the numpy oracle's error plays in tests/test_gpu_grad_blocks.py (oracle/ has no feed-forward agent). The tolerance rule
is ref64's, unchanged: tol = min(TOL_CAP, TOL_ROOM * max(e32, E32_FLOOR)).

Discrete decisions. The double-Q argmax and both relus (fc1's and rnn's) are read from the implementation under test
and followed (`cur_max_override`, `relu_override`, `hid_relu_override`); ref64.classify counts where they differ from
the float64 reference's own outside near-ties. The mixer's kinks cannot be read back: ref64.assert_clear_of_kinks holds
them clear, and the seeds below are chosen so that the float64 reference alone satisfies it (tests/test_ffn_host.py
asserts that without a GPU).
"""
from __future__ import annotations

from collections import OrderedDict

import torch.nn as nn

from tests import hyper2_ref
from tests.golden_utils import SynthCase
from tests.ref64 import H
from pymarl_amd.utils.synthetic import init_params


class RefFFAgent(nn.Module):
    """epymarl's RNNAgent with use_rnn = False, restated."""

    def __init__(self, input_dim, n_actions, hidden_dim=H):
        super().__init__()
        self.fc1 = nn.Linear(input_dim, hidden_dim)
        self.rnn = nn.Linear(hidden_dim, hidden_dim)
        self.fc2 = nn.Linear(hidden_dim, n_actions)

    def forward(self, inputs, hidden_state=None):
        x = nn.functional.relu(self.fc1(inputs))
        h = nn.functional.relu(self.rnn(x))
        return self.fc2(h), h


def ff_agent_shapes(input_dim, n_actions, hidden_dim=H):
    """The feed-forward agent's parameters in state_dict / parameters() order."""
    return OrderedDict([
        ("fc1.weight", (hidden_dim, input_dim)), ("fc1.bias", (hidden_dim,)),
        ("rnn.weight", (hidden_dim, hidden_dim)), ("rnn.bias", (hidden_dim,)),
        ("fc2.weight", (n_actions, hidden_dim)), ("fc2.bias", (n_actions,)),
    ])


class SynthCaseF(SynthCase):
    """A SynthCase whose agent is the feed-forward one. mixer: "qmix" / "vdn" / "none"; He: the two-layer QMIX
    hypernet's width (None: one layer)."""

    def __init__(self, name, He=None, **kw):
        super().__init__(name, **kw)
        seed = kw.get("weight_seed", 12)
        self.agent_shapes = ff_agent_shapes(self.I, self.A)
        self.agent_params = init_params(self.agent_shapes, seed=seed)
        self.He = He
        if He is not None:
            self.mixer_shapes = hyper2_ref.mixer2_shapes(self.S, self.n, He)
            self.mixer_params = init_params(self.mixer_shapes, seed=seed + 100)

    def over(self):
        """The learner arguments that select this agent (gpu_helpers.build(case, **case.over()))."""
        o = dict(use_rnn=False)
        if self.He is not None:
            o.update(hypernet_layers=2, hypernet_embed=self.He)
        return o


# The rows of tests/test_gpu_ffn.py, (n, A, O, S, T, B): the smallest shapes at which each thing can go wrong. Every
# episode is full length except in `ragged`. A weight seed other than SynthCase's default is one whose float64 reference
# keeps the mixer's pre-activations of live rows clear of 0 over both steps (test_ffn_host asserts it for every row).
ROW_SHAPES = OrderedDict([
    ("one", dict(dims=dict(n=1, A=2, O=5, S=7, T=1, B=1))),          # one row, one step
    ("part", dict(dims=dict(n=3, A=9, O=30, S=48, T=4, B=3))),       # RT = 45 < a 64-row tile; I = 42, I % 4 != 0
    ("tiles", dict(dims=dict(n=7, A=9, O=30, S=48, T=6, B=3))),      # RT = 147: several tiles and a remainder
    ("wideI", dict(dims=dict(n=3, A=5, O=150, S=48, T=3, B=4))),     # I > 128: dW1 has a second column tile
    ("A33", dict(dims=dict(n=2, A=33, O=12, S=16, T=3, B=3))),       # fc2 past 32 columns; past the fast mixers
    ("n17", dict(dims=dict(n=17, A=5, O=16, S=40, T=3, B=2))),       # n > 16: the stream mixer
    ("ragged", dict(dims=dict(n=3, A=9, O=30, S=48, T=4, B=3), ragged=True)),   # padded steps, unfilled previous slots
    ("part_h2", dict(dims=dict(n=3, A=9, O=30, S=48, T=4, B=3), He=20)),        # the two-layer hypernet beside it
    # The chain's own partitions (step_plan.hpp): split-K slices of [dWr | dbr] and dW1 need RT >= 512 to be more than
    # one, and ffn_dp2_kernel walks a second round of four rows only past RT = 4096 (or under MQ_PLAN ffn_dp2_blocks).
    # RT = 576: two split-K slices. Of the weight seeds 12, 21 .. 28 the one whose float64 reference keeps the 3e4
    # hypernet pre-activations of live rows furthest from 0 over both steps: min |.| 2.7e-5 (the default seed: 9e-6)
    ("split", dict(dims=dict(n=4, A=6, O=20, S=24, T=15, B=9), seeds=dict(weight_seed=25))),
    # RT = 4224: 16 split-K slices, 528 workgroups of two rounds. VDN: 1.8e5 hypernet outputs would hold values inside
    # KINK_EPS (ref64.SHAPES "wide" has the same reason)
    ("walk", dict(dims=dict(n=8, A=5, O=12, S=20, T=32, B=16), mixer="vdn")),
])
FLAGS = [(True, True), (True, False), (False, True), (False, False)]   # (obs_last_action, obs_agent_id) on `part`


def synth_case(row, mixer=None, steps=2, flags=(True, True)):
    spec = ROW_SHAPES[row]
    mixer = mixer or spec.get("mixer", "qmix")
    kw = dict(spec["dims"], **spec.get("seeds", {}))
    return SynthCaseF("ffn_{}_{}".format(row, mixer), He=spec.get("He"), n_episodes=kw["B"], steps=steps, mixer=mixer,
                      ragged=bool(spec.get("ragged", False)), min_len=1, obs_last_action=flags[0],
                      obs_agent_id=flags[1], **kw)
