"""The reference of the two-layer QMIX hypernetwork (hypernet_layers: 2), torch on the CPU.

* `RefQMixer2`: upstream PyMARL's two-layer QMixer restated (hyper_w_1 / hyper_w_final as Linear -> ReLU -> Linear;
  hyper_b_1 and V as with one layer), the module the state_dict interchange and the standalone forward are judged by.
* `ref_step`: tests/ref64.ref64_step with the mixer replaced and the dtype a parameter. In float64 it is the
  reference; in float32 its error against the float64 run is `e32`, the role the numpy oracle's error plays in
  tests/test_gpu_grad_blocks.py (oracle/ has no two-layer mixer). The tolerance rule is ref64's, unchanged:
  tol = min(TOL_CAP, TOL_ROOM * max(e32, E32_FLOOR)).
* `SynthCase2`: a SynthCase with the two-layer mixer's shapes, weights and `unflatten`.

Discrete decisions. The double-Q argmax, the fc1 relu and the hypernet's layer-1 relu are read from the implementation
under test and followed (`cur_max_override`, `relu_override`, `hyp_relu_override`); `classify` counts where they
differ from the float64 reference's own outside near-ties, by test_gpu_parity.classify_decisions' rule. The abs on
the second-layer outputs and V's relu cannot be read back: ref64.assert_clear_of_kinks holds every such
pre-activation of a live row further than KINK_EPS from 0, and the seeds below are chosen so that the float64
reference alone satisfies it (tests/test_hyper2_host.py asserts that without a GPU).
"""
from __future__ import annotations

from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch as th
import torch.nn as nn

from oracle.qlearner_np import NEG
from tests import ref64
from tests.golden_utils import Case, SynthCase
from tests.ref64 import E, H
from pymarl_amd.utils.synthetic import init_params

MARGIN_EPS = 1e-5   # tests/test_gpu_parity.py's near-tie rules
RELU_EPS = 1e-5


class RefQMixer2(nn.Module):
    """Upstream PyMARL's QMixer with hypernet_layers = 2, restated."""

    def __init__(self, n_agents, state_dim, embed_dim=E, hypernet_embed=64):
        super().__init__()
        self.n_agents, self.state_dim, self.embed_dim = n_agents, state_dim, embed_dim
        self.hyper_w_1 = nn.Sequential(nn.Linear(state_dim, hypernet_embed), nn.ReLU(),
                                       nn.Linear(hypernet_embed, embed_dim * n_agents))
        self.hyper_w_final = nn.Sequential(nn.Linear(state_dim, hypernet_embed), nn.ReLU(),
                                           nn.Linear(hypernet_embed, embed_dim))
        self.hyper_b_1 = nn.Linear(state_dim, embed_dim)
        self.V = nn.Sequential(nn.Linear(state_dim, embed_dim), nn.ReLU(), nn.Linear(embed_dim, 1))

    def forward(self, agent_qs, states):
        bs = agent_qs.size(0)
        states = states.reshape(-1, self.state_dim)
        agent_qs = agent_qs.view(-1, 1, self.n_agents)
        w1 = th.abs(self.hyper_w_1(states)).view(-1, self.n_agents, self.embed_dim)
        b1 = self.hyper_b_1(states).view(-1, 1, self.embed_dim)
        hidden = nn.functional.elu(th.bmm(agent_qs, w1) + b1)
        w_final = th.abs(self.hyper_w_final(states)).view(-1, self.embed_dim, 1)
        v = self.V(states).view(-1, 1, 1)
        return (th.bmm(hidden, w_final) + v).view(bs, -1, 1)


def mixer2_shapes(S, n, He, embed=E):
    """The two-layer QMixer's parameters in state_dict / parameters() order."""
    return OrderedDict([
        ("hyper_w_1.0.weight", (He, S)), ("hyper_w_1.0.bias", (He,)),
        ("hyper_w_1.2.weight", (embed * n, He)), ("hyper_w_1.2.bias", (embed * n,)),
        ("hyper_w_final.0.weight", (He, S)), ("hyper_w_final.0.bias", (He,)),
        ("hyper_w_final.2.weight", (embed, He)), ("hyper_w_final.2.bias", (embed,)),
        ("hyper_b_1.weight", (embed, S)), ("hyper_b_1.bias", (embed,)),
        ("V.0.weight", (embed, S)), ("V.0.bias", (embed,)),
        ("V.2.weight", (1, embed)), ("V.2.bias", (1,)),
    ])


class SynthCase2(SynthCase):
    """A QMIX SynthCase whose mixer is the two-layer one (hypernet_embed = He)."""

    def __init__(self, name, He=64, **kw):
        super().__init__(name, mixer="qmix", **kw)
        self.He = He
        self.mixer_shapes = mixer2_shapes(self.S, self.n, He)
        self.mixer_params = init_params(self.mixer_shapes, seed=kw.get("weight_seed", 12) + 100)

    def over(self):
        """The learner arguments that select this mixer (gpu_helpers.build(case, **case.over()))."""
        return dict(hypernet_layers=2, hypernet_embed=self.He)


class GoldenCase2(Case):
    """tests/golden/tiny_qmix_h2.npz (make_golden_hyper2.py: the reference's CPU QLearner with the two-layer mixer), in
    make_golden.py's format; golden_utils.Case with the two-layer mixer's shapes and seeded weights."""

    def __init__(self, name="tiny_qmix_h2"):
        super().__init__(name)
        self.He = int(self.z["hypernet_embed"])
        self.mixer_shapes = mixer2_shapes(self.S, self.n, self.He)
        self.mixer_params = init_params(self.mixer_shapes, seed=int(self.z["weight_seed"]) + 100)

    over = SynthCase2.over


# The rows of tests/test_gpu_hyper2.py: ref64.SHAPES entries (ragged, min_len = 1, E = 32) and `one`, with He and the
# seeds. A weight seed other than SynthCase's default is the one of 12, 21 .. 26 whose float64 reference keeps the
# second-layer outputs and V.0's pre-activations of live rows furthest from 0 over both steps (step 1 from the
# reference's own RMSprop update): min |.| is then 2.4e-5 (tiles_r21, whose default seed gives 5e-6) to 1.6e-4, against
# KINK_EPS = 1e-5. test_hyper2_host asserts the condition for every row.
ROW_SHAPES = OrderedDict([
    ("base", dict(shape="base", He=64, seeds=dict(weight_seed=25))),
    ("base_he20", dict(shape="base", He=20)),
    ("gemm", dict(shape="gemm", He=64, seeds=dict(weight_seed=21))),
    ("stream", dict(shape="stream", He=64, seeds=dict(weight_seed=22))),
    ("tiles_r21", dict(shape="tiles_r21", He=64, seeds=dict(weight_seed=25))),
    ("one", dict(dims=dict(n=3, A=9, O=30, S=48, T=1, B=1), He=64)),
])


def synth_case2(row, steps=2):
    spec = ROW_SHAPES[row]
    d = spec.get("dims") or ref64.SHAPES[spec["shape"]]
    return SynthCase2("h2_" + row, He=spec["He"], n_episodes=d["B"], steps=steps, ragged=True, min_len=1,
                      **dict(d, **spec.get("seeds", {})))


def _named(case, flat, grad, dtype):
    out = OrderedDict()
    for k, v in case.unflatten(np.asarray(flat)).items():
        t = th.tensor(np.asarray(v, np.float64), dtype=dtype)
        out[k] = t.requires_grad_(True) if grad else t
    return out


def _unroll(p, obs, onehot, flags, dtype, relu_mask=None):
    """ref64._unroll in `dtype`."""
    B, Tp, n, _ = obs.shape
    A = onehot.shape[-1]
    eye = th.eye(n, dtype=dtype).expand(B, n, n)
    h = th.zeros(B * n, H, dtype=dtype)
    qs, pres = [], []
    w_ih, w_hh, b_ih, b_hh = p["rnn.weight_ih"], p["rnn.weight_hh"], p["rnn.bias_ih"], p["rnn.bias_hh"]
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
        gi = x1 @ w_ih.T + b_ih
        gh = h @ w_hh.T + b_hh
        r = th.sigmoid(gi[:, :H] + gh[:, :H])
        z = th.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        c = th.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1.0 - z) * c + z * h
        qs.append((h @ p["fc2.weight"].T + p["fc2.bias"]).reshape(B, n, A))
    return th.stack(qs, 1), th.stack(pres, 1)


def _qmix2(mp, agent_qs, states, n, hyp_relu=None):
    """The two-layer QMixer.forward. Returns y (B,T,1), the pre-abs / pre-relu outputs hw1, hwf, hv and the layer-1
    pre-activations a1 (B*T, 2 He) = [hyper_w_1.0 | hyper_w_final.0]. hyp_relu (B*T, 2 He): 0/1 factors in place of
    the layer-1 relu's own decisions."""
    B, T = agent_qs.shape[:2]
    s = states.reshape(B * T, -1)
    q = agent_qs.reshape(B * T, 1, n)
    a1w = s @ mp["hyper_w_1.0.weight"].T + mp["hyper_w_1.0.bias"]
    a1f = s @ mp["hyper_w_final.0.weight"].T + mp["hyper_w_final.0.bias"]
    He = a1w.shape[1]
    if hyp_relu is None:
        x1w, x1f = th.relu(a1w), th.relu(a1f)
    else:
        x1w, x1f = a1w * hyp_relu[:, :He], a1f * hyp_relu[:, He:]
    hw1 = x1w @ mp["hyper_w_1.2.weight"].T + mp["hyper_w_1.2.bias"]
    hwf = x1f @ mp["hyper_w_final.2.weight"].T + mp["hyper_w_final.2.bias"]
    b1 = s @ mp["hyper_b_1.weight"].T + mp["hyper_b_1.bias"]
    hid = th.nn.functional.elu(th.bmm(q, hw1.abs().reshape(B * T, n, E)) + b1.reshape(B * T, 1, E))
    hv = s @ mp["V.0.weight"].T + mp["V.0.bias"]
    v = th.relu(hv) @ mp["V.2.weight"].T + mp["V.2.bias"]
    y = th.bmm(hid, hwf.abs().reshape(B * T, E, 1)) + v.reshape(B * T, 1, 1)
    return y.reshape(B, T, 1), hw1, hwf, hv, th.cat([a1w, a1f], 1)


def ref_step(case, flat_params, flat_targets, batch, dtype=th.float64, cur_max_override=None, relu_override=None,
             hyp_relu_override=None):
    """ref64.ref64_step for a SynthCase2, in `dtype`. hyp_relu_override (B, T, 2 He) bool: the online net's layer-1
    relu decisions. The result has ref64_step's fields and a1 (B, T, 2 He), the online layer-1 pre-activations."""
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

    mac_out, pre = _unroll(P, obs, onehot, flags, dtype, rm)
    chosen = th.gather(mac_out[:, :-1], 3, actions).squeeze(3)
    with th.no_grad():
        tmo, _ = _unroll(TP, obs, onehot, flags, dtype)
        tmo = tmo[:, 1:].masked_fill(~avail[:, 1:], float(NEG))
        masked_q = mac_out.detach().masked_fill(~avail, float(NEG))[:, 1:] if case.double_q else tmo
        cur_max = masked_q.argmax(3)
        if cur_max_override is not None:
            cur_max = th.tensor(np.asarray(cur_max_override, np.int64))
        target_max = th.gather(tmo, 3, cur_max.unsqueeze(3)).squeeze(3) if case.double_q else tmo.max(3)[0]
    state = tt(batch["state"])
    B, T = chosen.shape[:2]
    hr = None if hyp_relu_override is None else tt(np.asarray(hyp_relu_override, bool)).reshape(B * T, -1)
    q_tot, hw1, hwf, hv, a1 = _qmix2(P, chosen, state[:, :-1], n, hr)
    with th.no_grad():
        tq_tot = _qmix2(TP, target_max, state[:, 1:], n)[0]
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
    det = lambda x: x.detach().double().numpy()  # noqa: E731
    return SimpleNamespace(grads=grads, norm=norm, clipped=clipped,
                           clipped_flat=np.concatenate([g.ravel() for g in clipped.values()]), loss=loss.item(),
                           stats=stats, hw1=det(hw1), hwf=det(hwf), hv=det(hv), pre=det(pre), mac_out=det(mac_out),
                           a1=det(a1).reshape(B, T, -1), target_mac_out=det(tmo), masked_q=det(masked_q),
                           cur_max_actions=cur_max.numpy(), mask=det(m))


def classify(r, got_cur_max, got_relu, got_hyp_relu):
    """The implementation's decisions (cur_max (B,T,n), fc1 relu (B,T+1,n,H) bool, layer-1 relu (B,T,2He) bool) against
    the float64 reference's own (`r`, run without overrides from the same state): test_gpu_parity.classify_decisions'
    counts, plus the hypernet's. Flips outside near-ties must be 0."""
    q = r.masked_q
    top2 = -np.sort(-q, axis=3)[..., :2]
    margin = top2[..., 0] - top2[..., 1]
    tie = margin <= MARGIN_EPS * np.maximum(1.0, np.abs(top2[..., 0]))
    live = np.broadcast_to(r.mask > 0, tie.shape)
    dq_flip = np.asarray(got_cur_max) != r.cur_max_actions
    relu_tie = np.abs(r.pre) <= RELU_EPS
    relu_flip = np.asarray(got_relu, bool) != (r.pre > 0)
    hyp_tie = np.abs(r.a1) <= RELU_EPS
    hyp_flip = np.asarray(got_hyp_relu, bool) != (r.a1 > 0)
    return dict(dq_decisions=int(live.sum()), dq_ties=int((tie & live).sum()), dq_flips=int(dq_flip.sum()),
                dq_flips_outside_ties=int((dq_flip & ~tie).sum()), relu_ties=int(relu_tie.sum()),
                relu_flips=int(relu_flip.sum()), relu_flips_outside_ties=int((relu_flip & ~relu_tie).sum()),
                hyp_relu_decisions=int(hyp_tie.size), hyp_relu_ties=int(hyp_tie.sum()),
                hyp_relu_flips=int(hyp_flip.sum()), hyp_relu_flips_outside_ties=int((hyp_flip & ~hyp_tie).sum()))


def grad_blocks(case):
    """ref64.grad_blocks for the two-layer mixer: every tensor, fc1.weight by input kind, the GRU's tensors by gate,
    hyper_w_1.2.weight / .bias into the n per-agent row blocks of E."""
    blocks = OrderedDict()
    full = slice(None)
    for k in list(case.agent_shapes) + list(case.mixer_shapes):
        blocks[k] = (k, (full,))
    o = case.O
    blocks["fc1.weight[obs]"] = ("fc1.weight", (full, slice(0, o)))
    blocks["fc1.weight[last_action]"] = ("fc1.weight", (full, slice(o, o + case.A)))
    o += case.A
    blocks["fc1.weight[agent_id]"] = ("fc1.weight", (full, slice(o, o + case.n)))
    for k in ("rnn.weight_ih", "rnn.weight_hh", "rnn.bias_ih", "rnn.bias_hh"):
        for j, gate in enumerate("rzn"):
            blocks["{}[{}]".format(k, gate)] = (k, (slice(j * H, (j + 1) * H),))
    for k in ("hyper_w_1.2.weight", "hyper_w_1.2.bias"):
        for a in range(case.n):
            blocks["{}[agent{}]".format(k, a)] = (k, (slice(a * E, (a + 1) * E),))
    return blocks


def block_errors(got_flat, ref_named, case):
    """ref64.block_errors over grad_blocks above."""
    got = case.unflatten(np.asarray(got_flat, np.float64))
    out = OrderedDict()
    for name, (k, idx) in grad_blocks(case).items():
        ref = np.asarray(ref_named[k], np.float64)
        scale = float(np.abs(ref[idx]).max())
        if scale == 0.0:
            scale = float(np.abs(ref).max())
        out[name] = float(np.abs(got[k][idx] - ref[idx]).max()) / max(scale, 1e-300)
    return out


def rmsprop(case, params, sq, clipped_flat):
    """torch.optim.RMSprop's step in float64 on flat vectors: (new params, new square_avg)."""
    cfg = case.cfg()
    g = np.asarray(clipped_flat, np.float64)
    sq = cfg["optim_alpha"] * np.asarray(sq, np.float64) + (1.0 - cfg["optim_alpha"]) * g * g
    return np.asarray(params, np.float64) - cfg["lr"] * g / (np.sqrt(sq) + cfg["optim_eps"]), sq


def flat_of(case):
    return np.concatenate([v.ravel() for v in list(case.agent_params.values()) + list(case.mixer_params.values())])
