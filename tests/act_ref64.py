"""Float64 references of the acting path and the standalone module forwards, and the inputs their tests run on.

The kernels gated here choose the actions that fill the replay: one RNNAgent / BasicMAC step (`mac_step_kernel`), the
masked greedy argmax (`greedy_kernel`), the pi_logits post-processing (`mc_policy_kernel`) and the one-layer
QMixer.forward (`qmix_forward_kernel`). Each reference restates the operation in torch / numpy float64 on the CPU
from the reference project's behaviour (rnn_agent.py, basic_controller.py, action_selectors.py, qmix.py); none shares
code or indexing with the kernels. tests/test_act_ref64_host.py pins every one of them against torch's own modules
(`ModAgent`, `ModMixer`, softmax, max(dim)), which in float32 are also the fp32 counterparts that set the tolerance.

The value gate is tests/test_gpu_hyper2.py::test_standalone_forward's rule, per output (and per step of a chain):

    err <= TOL_ROOM * max(e32, E32_FLOOR * scale)

err = max|got - ref64|, scale = max|ref64|, e32 = max|fp32 counterpart - ref64| on the same inputs. `ratio` is
err / max(e32, E32_FLOOR * scale), the figure recorded per row. Discrete outputs (actions) compare exactly.
"""
from __future__ import annotations

from collections import OrderedDict
from types import SimpleNamespace as SN

import numpy as np
import torch as th
import torch.nn as nn

from tests import ref64
from tests.ref64 import E32_FLOOR, TOL_ROOM

H = 64
F64 = th.float64


# ------------------------------------------------------------------------------------------------------ the gate
def ratio(got, ref, c32):
    """(err / max(e32, E32_FLOOR * scale), err, e32, scale) of one output; non-finite entries must agree as such."""
    got, ref, c32 = (np.asarray(a, np.float64) for a in (got, ref, c32))
    assert got.shape == ref.shape == c32.shape, (got.shape, ref.shape, c32.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN pattern differs from the float64 reference"
    assert np.array_equal(got[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)]), "infinities differ"
    if not fin.any():
        return 0.0, 0.0, 0.0, 0.0
    scale = float(np.abs(ref[fin]).max())
    err = float(np.abs(got[fin] - ref[fin]).max())
    e32 = float(np.abs(c32[fin] - ref[fin]).max())
    den = max(e32, E32_FLOOR * scale)
    return (err / den if den > 0 else (0.0 if err == 0 else float("inf"))), err, e32, scale


def passes(r):
    return r <= TOL_ROOM


# ------------------------------------------------------------------------------------------------------ the agent
def named64(sd):
    return OrderedDict((k, th.as_tensor(np.asarray(v, np.float64))) for k, v in sd.items())


def _sig(x):
    return 1.0 / (1.0 + th.exp(-x))


def agent_step(p, x, h):
    """RNNAgent.forward: x (rows, I), h (rows, 64) -> q (rows, A), h' (rows, 64), and the fc1 pre-activations and the
    two gates (for the host test's coverage assertions). Written out: no nn module, no functional."""
    pre = x @ p["fc1.weight"].T + p["fc1.bias"]
    x1 = pre.clamp(min=0.0)
    gi = x1 @ p["rnn.weight_ih"].T + p["rnn.bias_ih"]
    gh = h @ p["rnn.weight_hh"].T + p["rnn.bias_hh"]
    r = _sig(gi[:, :H] + gh[:, :H])
    z = _sig(gi[:, H:2 * H] + gh[:, H:2 * H])
    c = th.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    h1 = c + z * (h - c)
    return h1 @ p["fc2.weight"].T + p["fc2.bias"], h1, SN(pre=pre, r=r, z=z)


def agent_chain(p, xs, h0):
    """agent_step over a list of inputs, h fed back: [(q_t, h_t)]."""
    out, h = [], h0
    for x in xs:
        q, h, _ = agent_step(p, x, h)
        out.append((q, h))
    return out


def build_inputs(obs, actions, filled, t, n_actions, flags, dtype=F64):
    """BasicMAC._build_inputs from the RAW replay fields: [obs_t | onehot(a_{t-1}) | onehot(agent id)] as (B * n, I).
    obs (B, Tp, n, O), actions (B, Tp, n, 1) integers, filled (B, Tp, 1); flags = (obs_last_action, obs_agent_id).
    The one-hot is zero at t = 0 and where slot t - 1 is unfilled: the reference's actions_onehot is zero-initialised
    and written for filled slots only."""
    obs = th.as_tensor(np.asarray(obs), dtype=dtype)
    B, _, n, _ = obs.shape
    cols = [obs[:, t]]
    if flags[0]:
        oh = th.zeros(B, n, n_actions, dtype=dtype)
        if t > 0:
            prev = np.asarray(actions)[:, t - 1, :, 0]
            live = np.asarray(filled)[:, t - 1, 0] != 0
            for b in range(B):
                if live[b]:
                    for a in range(n):
                        oh[b, a, int(prev[b, a])] = 1.0
        cols.append(oh)
    if flags[1]:
        ident = th.zeros(B, n, n, dtype=dtype)
        for a in range(n):
            ident[:, a, a] = 1.0
        cols.append(ident)
    return th.cat(cols, dim=2).reshape(B * n, -1)


def mac_chain(p, data, n_actions, flags, steps):
    """BasicMAC.forward for t = 0 .. steps - 1 from init_hidden (zeros): q (steps, B * n, A), h (steps, B * n, 64)."""
    B, _, n, _ = data["obs"].shape
    xs = [build_inputs(data["obs"], data["actions"], data["filled"], t, n_actions, flags) for t in range(steps)]
    out = agent_chain(p, xs, th.zeros(B * n, H, dtype=F64))
    return th.stack([q for q, _ in out]), th.stack([h for _, h in out])


class ModAgent(nn.Module):
    """torch's own fc1 -> relu -> GRUCell -> fc2: in float64 the pin of agent_step, in float32 its fp32 counterpart.
    GRU weights and biases are scaled by `gru_gain` so that some gates saturate."""

    def __init__(self, input_dim, n_actions, gru_gain=1.0):
        super().__init__()
        self.fc1 = nn.Linear(input_dim, H)
        self.rnn = nn.GRUCell(H, H)
        self.fc2 = nn.Linear(H, n_actions)
        with th.no_grad():
            for prm in self.rnn.parameters():
                prm.mul_(gru_gain)

    def forward(self, x, h):
        h1 = self.rnn(th.relu(self.fc1(x)), h)
        return self.fc2(h1), h1


def agent_case(I, A, rows, seed=0):
    """Parameters (a float32 ModAgent, GRU gain 8) and inputs of test a: x = 3 * randn with the last row zero, h =
    tanh(randn) with the first row zero (rows > 1; one row cannot hold both, it keeps the random values)."""
    g = th.Generator().manual_seed(10007 * I + 101 * A + rows + seed)
    with th.random.fork_rng():
        th.manual_seed(977 * I + 31 * A + seed)
        mod = ModAgent(I, A, gru_gain=8.0)
    x = 3.0 * th.randn(rows, I, generator=g)
    h = th.tanh(th.randn(rows, H, generator=g))
    if rows > 1:
        x[-1] = 0.0
        h[0] = 0.0
    return mod, x, h


AGENT_SHAPES = [(1, 1, 1), (5, 2, 3), (48, 9, 12), (257, 64, 5), (20, 6, 257)]   # (I, A, rows)
CHAIN_SHAPE, CHAIN_STEPS = (48, 9, 12), 20


def chain_inputs(I, rows, steps, seed=0):
    g = th.Generator().manual_seed(4242 + seed)
    return [3.0 * th.randn(rows, I, generator=g) for _ in range(steps)]


# ------------------------------------------------------------------------------------------------------ the MAC case
MAC = dict(A=5, O=7, S=4, T=6, n_episodes=6)
MAC_FLAGS = [(True, True), (True, False), (False, True), (False, False)]
MAC_DATA_SEED = 7   # lengths of the six episodes include 1 and T (asserted by the host test)


def mac_case(flags, n=3):
    """The synthetic MAC case of test b: 6 ragged episodes of at most T = 6 steps (T + 1 slots)."""
    from tests.golden_utils import SynthCase
    return SynthCase("act_mac_{}{}_n{}".format(int(flags[0]), int(flags[1]), n), n=n, B=MAC["n_episodes"], steps=1,
                     mixer="vdn", ragged=True, min_len=1, data_seed=MAC_DATA_SEED, weight_seed=29,
                     obs_last_action=flags[0], obs_agent_id=flags[1], **MAC)


# ------------------------------------------------------------------------------------------------------ greedy
def greedy(q, avail):
    """masked_q[avail == 0] = -inf; masked_q.max(-1)[1], stated without max(dim): a NaN at an available action wins
    (first such index), else the first index holding the maximum; a row with nothing available gives 0."""
    q = np.asarray(q, np.float64)
    m = np.where(np.asarray(avail) == 0, -np.inf, q)
    nan = np.isnan(m)
    top = np.where(nan, -np.inf, m).max(axis=-1, keepdims=True)
    at_top = (m == top) & ~nan
    first = lambda mask: np.where(mask.any(-1), mask.argmax(-1), 0)   # noqa: E731  (argmax of bools: first True)
    return np.where(nan.any(-1), first(nan), first(at_top)).astype(np.int64)


def greedy_case(rows, A, seed=0, nans=True):
    """q (rows, A) float32 and avail (rows, A) int32 holding, as far as the shape allows: exact ties at the maximum
    (values from a grid of 4), avail values 2 and -1, all-unavailable rows, -inf at an available action (alone and
    beside finite ones), an unavailable action above every available one, and (nans) a NaN at an available
    non-first index and at an unavailable index."""
    g = np.random.Generator(np.random.PCG64(7919 * rows + 13 * A + seed))
    q = g.integers(0, 4, size=(rows, A)).astype(np.float32) - 1.5   # a grid: ties are the rule, not the exception
    avail = (g.random((rows, A)) < 0.7).astype(np.int32)
    avail[avail == 1] = g.choice(np.array([1, 2, -1], np.int32), size=int((avail == 1).sum()))
    kinds = g.integers(0, 8, size=rows)
    for r in range(rows):
        k, j = kinds[r], int(g.integers(0, A))
        if k == 0:
            avail[r] = 0                                    # nothing available
        elif k == 1:
            avail[r, j], q[r, j] = 1, -np.inf                # -inf at an available action
        elif k == 2:
            avail[r], q[r] = 1, -np.inf                      # only -inf, all available: first index
        elif k == 3:
            avail[r, j], q[r, j] = 0, 100.0                  # the overall maximum is unavailable
        elif k == 4 and nans and A > 1:
            j = max(j, 1)
            avail[r, j], q[r, j] = 2, np.nan                 # NaN at an available non-first index
            if j + 1 < A:
                avail[r, j + 1], q[r, j + 1] = 1, 50.0       # and a larger finite value after it
        elif k == 5 and nans:
            avail[r, j], q[r, j] = 0, np.nan                 # NaN at an unavailable index: masked
    return q, avail


GREEDY_ROWS, GREEDY_A = (1, 255, 256, 257, 1000), (1, 2, 9, 64)


# ------------------------------------------------------------------------------------------------------ pi_logits
def policy(logits, avail, eps, mask_before_softmax, test_mode, dtype=F64):
    """BasicMAC.forward's pi_logits branch on (rows, A): the -1e10 mask, softmax (written out), the epsilon floor over
    the available count (masking on) or over A, masked entries zeroed."""
    x = th.as_tensor(np.asarray(logits), dtype=dtype).clone()
    un = th.as_tensor(np.asarray(avail)) == 0
    if mask_before_softmax:
        x[un] = -1e10
    e = th.exp(x - x.max(dim=1, keepdim=True)[0])
    p = e / e.sum(dim=1, keepdim=True)
    if not test_mode:
        count = float(x.shape[1])
        if mask_before_softmax:
            count = (~un).sum(dim=1, keepdim=True).to(dtype)
        p = (1.0 - eps) * p + eps / (count + th.zeros_like(p))
        if mask_before_softmax:
            p[un] = 0.0
    return p


def policy_mod(logits, avail, eps, mask_before_softmax, test_mode, dtype):
    """The same through torch's own softmax / masked_fill / where: the pin (float64) and fp32 counterpart."""
    x = th.as_tensor(np.asarray(logits), dtype=dtype)
    av = th.as_tensor(np.asarray(avail))
    if mask_before_softmax:
        x = x.masked_fill(av == 0, -1e10)
    p = th.nn.functional.softmax(x, dim=-1)
    if test_mode:
        return p
    num = av.sum(dim=1, keepdim=True).to(dtype) if mask_before_softmax else p.size(-1)
    p = (1 - eps) * p + th.ones_like(p) * eps / num
    return th.where(av == 0, th.zeros_like(p), p) if mask_before_softmax else p


def policy_case(rows, A, seed=0):
    """logits (rows, A) float32 in 2 * randn with entries of +-80, avail (rows, A) in {0, 1} int32; as far as the
    shape allows row 0 has a single available action and the last row none."""
    g = np.random.Generator(np.random.PCG64(104729 * rows + 17 * A + seed))
    lg = (2.0 * g.standard_normal((rows, A))).astype(np.float32)
    big = g.random((rows, A)) < 0.1
    lg[big] = np.where(g.random(int(big.sum())) < 0.5, 80.0, -80.0).astype(np.float32)
    avail = (g.random((rows, A)) < 0.7).astype(np.int32)
    avail[np.arange(rows), g.integers(0, A, size=rows)] = 1
    avail[0] = 0
    avail[0, A // 2] = 1
    if rows > 1:
        avail[-1] = 0
    return lg, avail


POLICY_A, POLICY_ROWS, POLICY_EPS = (1, 5, 64), (1, 3, 4, 5, 1023), (0.0, 0.3, 1.0)


# ------------------------------------------------------------------------------------------------------ the mixer
def qmix(mp, agent_qs, states):
    """One-layer QMixer.forward on rows: agent_qs (rows, n), states (rows, S) -> q_tot (rows,) and the elu
    pre-activations (rows, E). ref64.qmix, fed as a batch of one-step episodes."""
    n = agent_qs.shape[1]
    y, hw1, _, _, _ = ref64.qmix(mp, agent_qs.unsqueeze(1), states.unsqueeze(1), n)
    Em = mp["hyper_w_final.weight"].shape[0]
    b1 = states @ mp["hyper_b_1.weight"].T + mp["hyper_b_1.bias"]
    pre = (agent_qs.unsqueeze(2) * hw1.abs().reshape(-1, n, Em)).sum(1) + b1
    return y.reshape(-1), pre


class ModMixer(nn.Module):
    """The one-layer QMixer from torch's own Linear / elu / bmm (state_dict names as the project's QMixer)."""

    def __init__(self, n, S, E):
        super().__init__()
        self.n, self.S, self.E = n, S, E
        self.hyper_w_1 = nn.Linear(S, E * n)
        self.hyper_w_final = nn.Linear(S, E)
        self.hyper_b_1 = nn.Linear(S, E)
        self.V = nn.Sequential(nn.Linear(S, E), nn.ReLU(), nn.Linear(E, 1))

    def forward(self, agent_qs, states):
        bs = agent_qs.size(0)
        s = states.reshape(-1, self.S)
        q = agent_qs.reshape(-1, 1, self.n)
        w1 = th.abs(self.hyper_w_1(s)).view(-1, self.n, self.E)
        b1 = self.hyper_b_1(s).view(-1, 1, self.E)
        hidden = nn.functional.elu(th.bmm(q, w1) + b1)
        wf = th.abs(self.hyper_w_final(s)).view(-1, self.E, 1)
        v = self.V(s).view(-1, 1, 1)
        return (th.bmm(hidden, wf) + v).view(bs, -1, 1)


MIXER_SHAPES = [(1, 1, 1, 1), (3, 48, 32, 33), (3, 30, 17, 6), (8, 40, 64, 5), (17, 7, 32, 3), (64, 48, 64, 5)]


def mixer_case(n, S, E, rows, seed=0):
    """A float32 ModMixer and inputs of test e: agent qs 2 * randn (both signs), states randn. The single-row shape
    cannot hold both signs of its one elu pre-activation; every other shape does (asserted by the host test)."""
    g = th.Generator().manual_seed(7 * n + 1009 * S + 11 * E + rows + seed)
    with th.random.fork_rng():
        th.manual_seed(3 * n + S + 101 * E + seed)
        mod = ModMixer(n, S, E)
    return mod, 2.0 * th.randn(rows, n, generator=g), th.randn(rows, S, generator=g)
