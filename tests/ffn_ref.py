"""The reference of the feed-forward agent (use_rnn: False, epymarl's key), torch on the CPU.

* `RefFFAgent`: epymarl's RNNAgent with use_rnn = False restated (rnn = nn.Linear(64, 64), a ReLU behind it, the
  incoming hidden state ignored), the module the state_dict interchange and the acting path are judged by.
* `ref_step`: tests/ref64.ref64_step with the agent replaced and the dtype a parameter; the mixer, the masks and the
  loss are ref64's (the two-layer mixer: tests/hyper2_ref._qmix2). In float64 it is the reference; in float32 its error
  against the float64 run is `e32`, the role the numpy oracle's error plays in tests/test_gpu_grad_blocks.py (oracle/
  has no feed-forward agent). The tolerance rule is ref64's, unchanged:
  tol = min(TOL_CAP, TOL_ROOM * max(e32, E32_FLOOR)).
* `SynthCaseF`: a SynthCase with the feed-forward agent's shapes, weights and `unflatten`.

Discrete decisions. The double-Q argmax and both relus (fc1's and rnn's) are read from the implementation under test
and followed (`cur_max_override`, `relu_override`, `hid_relu_override`); `classify` counts where they differ from the
float64 reference's own outside near-ties, by test_gpu_parity.classify_decisions' rule. The mixer's kinks cannot be
read back: ref64.assert_clear_of_kinks holds them clear, and the seeds below are chosen so that the float64 reference
alone satisfies it (tests/test_ffn_host.py asserts that without a GPU).
"""
from __future__ import annotations

from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch as th
import torch.nn as nn

from oracle.qlearner_np import NEG
from tests import hyper2_ref, ref64
from tests.golden_utils import SynthCase
from tests.ref64 import E, H
from pymarl_amd.utils.synthetic import init_params

MARGIN_EPS = 1e-5   # tests/test_gpu_parity.py's near-tie rules
RELU_EPS = 1e-5


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


def _named(case, flat, grad, dtype):
    out = OrderedDict()
    for k, v in case.unflatten(np.asarray(flat)).items():
        t = th.tensor(np.asarray(v, np.float64), dtype=dtype)
        out[k] = t.requires_grad_(True) if grad else t
    return out


def _unroll(p, obs, onehot, flags, dtype, relu_mask=None, hid_mask=None):
    """BasicMAC.forward over t with the feed-forward agent: Q (B,Tp,n,A), fc1 pre-activations and rnn pre-activations
    (B,Tp,n,H). Nothing is carried from step to step."""
    B, Tp, n, _ = obs.shape
    A = onehot.shape[-1]
    eye = th.eye(n, dtype=dtype).expand(B, n, n)
    qs, pres, pre2s = [], [], []
    for t in range(Tp):
        parts = [obs[:, t]]
        if flags[0]:
            parts.append(th.zeros(B, n, A, dtype=dtype) if t == 0 else onehot[:, t - 1])
        if flags[1]:
            parts.append(eye)
        x = th.cat(parts, -1).reshape(B * n, -1)
        pre = x @ p["fc1.weight"].T + p["fc1.bias"]
        pres.append(pre.reshape(B, n, H))
        x1 = th.relu(pre) if relu_mask is None else pre * relu_mask[:, t].reshape(B * n, H)
        pre2 = x1 @ p["rnn.weight"].T + p["rnn.bias"]
        pre2s.append(pre2.reshape(B, n, H))
        h = th.relu(pre2) if hid_mask is None else pre2 * hid_mask[:, t].reshape(B * n, H)
        qs.append((h @ p["fc2.weight"].T + p["fc2.bias"]).reshape(B, n, A))
    return th.stack(qs, 1), th.stack(pres, 1), th.stack(pre2s, 1)


def ref_step(case, flat_params, flat_targets, batch, dtype=th.float64, cur_max_override=None, relu_override=None,
             hid_relu_override=None, hyp_relu_override=None):
    """ref64.ref64_step for a SynthCaseF, in `dtype`. relu_override / hid_relu_override (B, T+1, n, H) bool: the
    online net's fc1 / rnn relu decisions; hyp_relu_override: hyper2_ref.ref_step's (two-layer mixer only). The result
    has ref64_step's fields, pre2 (B, T+1, n, H), the online rnn pre-activations, and hid (B, T+1, n, H), relu of it."""
    cfg = case.cfg()
    n = case.n
    gamma = float(np.float32(cfg["gamma"]))
    flags = (bool(case.obs_last_action), bool(case.obs_agent_id))
    names = list(case.agent_shapes) + list(case.mixer_shapes)
    P = _named(case, flat_params, True, dtype)
    TP = _named(case, flat_targets, False, dtype)
    tt = lambda a: th.tensor(np.asarray(a, np.float64), dtype=dtype)  # noqa: E731
    obs, onehot = tt(batch["obs"]), tt(batch["actions_onehot"])
    rewards = tt(batch["reward"][:, :-1])
    terminated = tt(batch["terminated"][:, :-1])
    actions = th.tensor(np.asarray(batch["actions"][:, :-1], np.int64))
    avail = th.tensor(np.asarray(batch["avail_actions"]) != 0)
    mask = tt(batch["filled"][:, :-1]).clone()
    mask[:, 1:] = mask[:, 1:] * (1.0 - terminated[:, :-1])
    rm = None if relu_override is None else tt(np.asarray(relu_override, bool))
    hm = None if hid_relu_override is None else tt(np.asarray(hid_relu_override, bool))

    mac_out, pre, pre2 = _unroll(P, obs, onehot, flags, dtype, rm, hm)
    chosen = th.gather(mac_out[:, :-1], 3, actions).squeeze(3)
    with th.no_grad():
        tmo = _unroll(TP, obs, onehot, flags, dtype)[0]
        tmo = tmo[:, 1:].masked_fill(~avail[:, 1:], float(NEG))
        masked_q = mac_out.detach().masked_fill(~avail, float(NEG))[:, 1:] if case.double_q else tmo
        cur_max = masked_q.argmax(3)
        if cur_max_override is not None:
            cur_max = th.tensor(np.asarray(cur_max_override, np.int64))
        target_max = th.gather(tmo, 3, cur_max.unsqueeze(3)).squeeze(3) if case.double_q else tmo.max(3)[0]
    hw1 = hwf = hv = a1 = None
    B, T = chosen.shape[:2]
    if case.mixer == "qmix":
        state = tt(batch["state"])
        if case.He is not None:
            hr = None if hyp_relu_override is None else tt(np.asarray(hyp_relu_override, bool)).reshape(B * T, -1)
            q_tot, hw1, hwf, hv, a1 = hyper2_ref._qmix2(P, chosen, state[:, :-1], n, hr)
            with th.no_grad():
                tq_tot = hyper2_ref._qmix2(TP, target_max, state[:, 1:], n)[0]
        else:
            q_tot, hw1, hwf, hv = ref64._qmix(P, chosen, state[:, :-1], n)
            with th.no_grad():
                tq_tot = ref64._qmix(TP, target_max, state[:, 1:], n)[0]
    elif case.mixer == "vdn":
        q_tot, tq_tot = chosen.sum(2, keepdim=True), target_max.sum(2, keepdim=True)
    else:
        q_tot, tq_tot = chosen, target_max
    targets = rewards + gamma * (1.0 - terminated) * tq_tot
    td = q_tot - targets.detach()
    m = mask.expand_as(td)
    mtd = td * m
    msum = m.sum()
    loss = (mtd ** 2).sum() / msum
    loss.backward()

    grads = OrderedDict((k, P[k].grad.double().numpy().copy()) for k in names)
    if dtype == th.float64:
        norm = float(np.sqrt(sum(float((g * g).sum()) for g in grads.values())))
        coef = min(cfg["grad_norm_clip"] / (norm + 1e-6), 1.0)
    else:   # clip_grad_norm_ in the run's own precision
        g32 = [g.astype(np.float32) for g in grads.values()]
        norm32 = np.sqrt(np.sum(np.array([np.sum(g * g, dtype=np.float32) for g in g32], np.float32),
                                dtype=np.float32))
        norm = float(norm32)
        coef = float(min(np.float32(cfg["grad_norm_clip"]) / (norm32 + np.float32(1e-6)), np.float32(1.0)))
    clipped = OrderedDict((k, g * coef) for k, g in grads.items())
    ms = float(msum)
    with th.no_grad():
        stats = dict(loss=loss.item(), grad_norm=norm, td_error_abs=mtd.abs().sum().item() / ms,
                     q_taken_mean=(q_tot * m).sum().item() / (ms * n),
                     target_mean=(targets * m).sum().item() / (ms * n))
    det = lambda x: None if x is None else x.detach().double().numpy()  # noqa: E731
    return SimpleNamespace(grads=grads, norm=norm, clipped=clipped,
                           clipped_flat=np.concatenate([g.ravel() for g in clipped.values()]), loss=loss.item(),
                           stats=stats, hw1=det(hw1), hwf=det(hwf), hv=det(hv), pre=det(pre), pre2=det(pre2),
                           x1=det(th.relu(pre)), hid=det(th.relu(pre2)), mac_out=det(mac_out),
                           a1=None if a1 is None else det(a1).reshape(B, T, -1),
                           target_mac_out=det(tmo), target_mac_out_full=det(_unroll(TP, obs, onehot, flags, dtype)[0]),
                           masked_q=det(masked_q), cur_max_actions=cur_max.numpy(), mask=det(m))


def classify(r, got_cur_max, got_relu, got_hid_relu):
    """The implementation's decisions (cur_max (B,T,n), fc1 relu and rnn relu (B,T+1,n,H) bool) against the float64
    reference's own (`r`, run without overrides from the same state): test_gpu_parity.classify_decisions' counts, plus
    the rnn relu's. Flips outside near-ties must be 0."""
    q = r.masked_q
    top2 = -np.sort(-q, axis=3)[..., :2]
    margin = top2[..., 0] - top2[..., 1]
    tie = margin <= MARGIN_EPS * np.maximum(1.0, np.abs(top2[..., 0]))
    live = np.broadcast_to(r.mask > 0, tie.shape)
    dq_flip = np.asarray(got_cur_max) != r.cur_max_actions
    relu_tie = np.abs(r.pre) <= RELU_EPS
    relu_flip = np.asarray(got_relu, bool) != (r.pre > 0)
    hid_tie = np.abs(r.pre2) <= RELU_EPS
    hid_flip = np.asarray(got_hid_relu, bool) != (r.pre2 > 0)
    return dict(dq_decisions=int(live.sum()), dq_ties=int((tie & live).sum()), dq_flips=int(dq_flip.sum()),
                dq_flips_outside_ties=int((dq_flip & ~tie).sum()), relu_ties=int(relu_tie.sum()),
                relu_flips=int(relu_flip.sum()), relu_flips_outside_ties=int((relu_flip & ~relu_tie).sum()),
                hid_relu_decisions=int(hid_tie.size), hid_relu_ties=int(hid_tie.sum()),
                hid_relu_flips=int(hid_flip.sum()), hid_relu_flips_outside_ties=int((hid_flip & ~hid_tie).sum()))


def grad_blocks(case):
    """{block name: (tensor name, index)}: every tensor; fc1.weight by input kind (obs / last action / agent id, as the
    case's flags give); then the mixer's blocks as ref64 (one layer) or hyper2_ref (two layers) has them."""
    blocks = OrderedDict()
    full = slice(None)
    for k in list(case.agent_shapes) + list(case.mixer_shapes):
        blocks[k] = (k, (full,))
    o = case.O
    blocks["fc1.weight[obs]"] = ("fc1.weight", (full, slice(0, o)))
    if case.obs_last_action:
        blocks["fc1.weight[last_action]"] = ("fc1.weight", (full, slice(o, o + case.A)))
        o += case.A
    if case.obs_agent_id:
        blocks["fc1.weight[agent_id]"] = ("fc1.weight", (full, slice(o, o + case.n)))
    if case.mixer == "qmix":
        w1 = ("hyper_w_1.weight", "hyper_w_1.bias") if case.He is None else ("hyper_w_1.2.weight", "hyper_w_1.2.bias")
        for k in w1:
            for a in range(case.n):
                blocks["{}[agent{}]".format(k, a)] = (k, (slice(a * E, (a + 1) * E),))
    return blocks


def block_errors(got_flat, ref_named, case):
    """ref64.block_errors over grad_blocks above."""
    return ref64.block_errors(got_flat, ref_named, case, blocks=grad_blocks(case))


def rmsprop(case, params, sq, clipped_flat):
    """torch.optim.RMSprop's step in float64 on flat vectors: (new params, new square_avg)."""
    return hyper2_ref.rmsprop(case, params, sq, clipped_flat)


def adam(params, m, v, clipped_flat, t, lr=5e-4, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's step t (1-based) in float64 on flat vectors: (new params, exp_avg, exp_avg_sq)."""
    g = np.asarray(clipped_flat, np.float64)
    m = b1 * np.asarray(m, np.float64) + (1.0 - b1) * g
    v = b2 * np.asarray(v, np.float64) + (1.0 - b2) * g * g
    step = lr / (1.0 - b1 ** t)
    return np.asarray(params, np.float64) - step * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps), m, v


def flat_of(case):
    return np.concatenate([v.ravel() for v in list(case.agent_params.values()) + list(case.mixer_params.values())])
