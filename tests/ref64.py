"""An independent float64 reference of one QMIX / VDN / IQL learner step, and the per-block gradient gate built on it.

`ref64_step` restates the step's loss in torch float64 on the CPU and lets autograd differentiate it: agent unroll
over `[obs | last-action one-hot | agent id]`, fc1 -> relu -> GRU cell -> fc2, double-Q or max target, QMixer / sum /
none, the -9999999 masks and the masked L2 loss. It shares no hand-derived backward with the numpy oracle
(oracle/qlearner_np.py) or with the kernels; only constants are taken from the oracle. Huber and TD(lambda) are out
of scope; COMA's train() has its own reference on the same gate in tests/coma_ref64.py.

The gate (DESIGN.md "Parity"): every block named by `grad_blocks` is judged on its own max,
`block_errors` = max|got - ref| / max|ref| per block, against `tolerances(e32)` where e32 is the fp32 numpy
oracle's own error against this reference on the same block, from the same state with the same overrides:

    tol(block) = min(TOL_CAP, TOL_ROOM * max(e32(block), E32_FLOOR))

* E32_FLOOR = 2e-7 is about 2 ulp of the block max (fp32 eps 1.19e-7): a block where the oracle was lucky does not get
  an impossible bound;
* TOL_ROOM = 16 is room for a different summation order over the same terms (MFMA k-order, per-row slabs, two-pass
  reduction); the kernels use expf / tanhf, so no more than that is expected;
* TOL_CAP = 1e-5 is a condition, not a measurement: no block is ever judged looser than ten times tighter than the
  global 1e-4 gate of the teacher-forced tests.

The comparison has discrete decisions that may differ under fp32 rounding. The double-Q argmax and the fc1 relu are
taken from the implementation under test (`cur_max_override`, `relu_override`). The mixer's kinks (abs on hw1 / hwf,
V's relu on hv) cannot be read back, so `kink_minima` / `assert_clear_of_kinks` require every such pre-activation of
a live row to be further than KINK_EPS from 0.
"""
from __future__ import annotations

from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch as th

from oracle.qlearner_np import NEG   # the reference's mask constant (q_learner.py:68,74); nothing else is shared

H = 64          # rnn_hidden_dim of every case
E = 32          # mixing_embed_dim of every case
KINK_EPS = 1e-5
E32_FLOOR = 2e-7
TOL_ROOM = 16.0
TOL_CAP = 1e-5
F64 = th.float64


def _named(case, flat, grad):
    """Case.unflatten's layout as float64 torch tensors (leaf tensors with grad when `grad`)."""
    out = OrderedDict()
    for k, v in case.unflatten(np.asarray(flat)).items():
        t = th.tensor(np.asarray(v, np.float64), dtype=F64)
        out[k] = t.requires_grad_(True) if grad else t
    return out


def _unroll(p, obs, onehot, flags, relu_mask=None):
    """BasicMAC.forward over t with RNNAgent. obs (B,Tp,n,O), onehot (B,Tp,n,A) -> Q (B,Tp,n,A), fc1 pre (B,Tp,n,H)."""
    B, Tp, n, _ = obs.shape
    A = onehot.shape[-1]
    eye = th.eye(n, dtype=F64).expand(B, n, n)
    h = th.zeros(B * n, H, dtype=F64)
    qs, pres = [], []
    w_ih, w_hh, b_ih, b_hh = p["rnn.weight_ih"], p["rnn.weight_hh"], p["rnn.bias_ih"], p["rnn.bias_hh"]
    for t in range(Tp):
        parts = [obs[:, t]]
        if flags[0]:
            parts.append(th.zeros(B, n, A, dtype=F64) if t == 0 else onehot[:, t - 1])
        if flags[1]:
            parts.append(eye)
        x = th.cat(parts, -1).reshape(B * n, -1)
        pre = x @ p["fc1.weight"].T + p["fc1.bias"]
        pres.append(pre.reshape(B, n, H))
        if relu_mask is None:
            x1 = th.relu(pre)
        else:   # the other implementation's on/off decisions, a constant 0/1 factor on the pre-activation
            x1 = pre * relu_mask[:, t].reshape(B * n, H)
        gi = x1 @ w_ih.T + b_ih
        gh = h @ w_hh.T + b_hh
        r = th.sigmoid(gi[:, :H] + gh[:, :H])
        z = th.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        c = th.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1.0 - z) * c + z * h
        qs.append((h @ p["fc2.weight"].T + p["fc2.bias"]).reshape(B, n, A))
    return th.stack(qs, 1), th.stack(pres, 1)


def _qmix(mp, agent_qs, states, n):
    """QMixer.forward. agent_qs (B,T,n), states (B,T,S) -> y (B,T,1) and the pre-abs / pre-relu hypernet outputs."""
    B, T = agent_qs.shape[:2]
    E = mp["hyper_w_final.weight"].shape[0]   # the module constant on every learner case; tests/act_ref64.py: 1 .. 64
    s = states.reshape(B * T, -1)
    q = agent_qs.reshape(B * T, 1, n)
    hw1 = s @ mp["hyper_w_1.weight"].T + mp["hyper_w_1.bias"]
    b1 = s @ mp["hyper_b_1.weight"].T + mp["hyper_b_1.bias"]
    hid = th.nn.functional.elu(th.bmm(q, hw1.abs().reshape(B * T, n, E)) + b1.reshape(B * T, 1, E))
    hwf = s @ mp["hyper_w_final.weight"].T + mp["hyper_w_final.bias"]
    hv = s @ mp["V.0.weight"].T + mp["V.0.bias"]
    v = th.relu(hv) @ mp["V.2.weight"].T + mp["V.2.bias"]
    y = th.bmm(hid, hwf.abs().reshape(B * T, E, 1)) + v.reshape(B * T, 1, 1)
    return y.reshape(B, T, 1), hw1, hwf, hv


def ref64_step(case, flat_params, flat_targets, batch, cur_max_override=None, relu_override=None):
    """One learner step's loss and its autograd gradient in float64.

    flat_params / flat_targets: flat float32 vectors in Case.unflatten's layout; batch: the numpy batch of
    case.batch(k). cur_max_override (B,T,n) / relu_override (B,T+1,n,H): as in OracleQLearner.forward.
    Returns a namespace: grads (raw, per named tensor, float64 numpy), norm, clipped (per named tensor),
    clipped_flat, loss, stats (the five), hw1 / hwf / hv ((B*T, .), None without a QMixer), pre (fc1
    pre-activations, (B,T+1,n,H)), mac_out, target_mac_out (masked, steps 1..T), masked_q (the Q the target's
    argmax decision is taken on), cur_max_actions, mask (B,T,1 or n)."""
    cfg = case.cfg()
    n, gamma = case.n, float(np.float32(cfg["gamma"]))
    flags = (bool(case.obs_last_action), bool(case.obs_agent_id))
    names = list(case.agent_shapes) + list(case.mixer_shapes)
    P = _named(case, flat_params, True)
    TP = _named(case, flat_targets, False)
    t64 = lambda a: th.tensor(np.asarray(a, np.float64), dtype=F64)  # noqa: E731
    obs, onehot = t64(batch["obs"]), t64(batch["actions_onehot"])
    rewards = t64(batch["reward"][:, :-1])
    terminated = t64(batch["terminated"][:, :-1])
    actions = th.tensor(np.asarray(batch["actions"][:, :-1], np.int64))
    avail = th.tensor(np.asarray(batch["avail_actions"]) != 0)
    mask = t64(batch["filled"][:, :-1]).clone()
    mask[:, 1:] = mask[:, 1:] * (1.0 - terminated[:, :-1])
    rm = None if relu_override is None else t64(np.asarray(relu_override, bool))

    mac_out, pre = _unroll(P, obs, onehot, flags, rm)
    chosen = th.gather(mac_out[:, :-1], 3, actions).squeeze(3)
    with th.no_grad():
        tmo, _ = _unroll(TP, obs, onehot, flags)
        tmo = tmo[:, 1:].masked_fill(~avail[:, 1:], float(NEG))
        if case.double_q:
            masked_q = mac_out.detach().masked_fill(~avail, float(NEG))[:, 1:]
        else:
            masked_q = tmo
        cur_max = masked_q.argmax(3)
        if cur_max_override is not None:
            cur_max = th.tensor(np.asarray(cur_max_override, np.int64))
        target_max = th.gather(tmo, 3, cur_max.unsqueeze(3)).squeeze(3) if case.double_q else tmo.max(3)[0]
    hw1 = hwf = hv = None
    if case.mixer == "qmix":
        state = t64(batch["state"])
        q_tot, hw1, hwf, hv = _qmix(P, chosen, state[:, :-1], n)
        with th.no_grad():
            tq_tot = _qmix(TP, target_max, state[:, 1:], n)[0]
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

    grads = OrderedDict((k, P[k].grad.numpy().copy()) for k in names)
    norm = float(np.sqrt(sum(float((g * g).sum()) for g in grads.values())))
    coef = min(cfg["grad_norm_clip"] / (norm + 1e-6), 1.0)
    clipped = OrderedDict((k, g * coef) for k, g in grads.items())
    ms = float(msum)
    with th.no_grad():
        stats = dict(loss=loss.item(), grad_norm=norm, td_error_abs=mtd.abs().sum().item() / ms,
                     q_taken_mean=(q_tot * m).sum().item() / (ms * n),
                     target_mean=(targets * m).sum().item() / (ms * n))
    det = lambda x: None if x is None else x.detach().numpy()  # noqa: E731
    return SimpleNamespace(grads=grads, norm=norm, clipped=clipped,
                           clipped_flat=np.concatenate([g.ravel() for g in clipped.values()]), loss=loss.item(),
                           stats=stats, hw1=det(hw1), hwf=det(hwf), hv=det(hv), pre=det(pre), mac_out=det(mac_out),
                           target_mac_out=tmo.numpy(), masked_q=masked_q.numpy(), cur_max_actions=cur_max.numpy(),
                           mask=m.numpy())


def kink_minima(r):
    """min |hw1|, |hwf|, |hv| over the live rows (mask > 0) of a QMIX ref64_step result."""
    live = r.mask.reshape(-1) > 0
    return {k: float(np.abs(getattr(r, k)[live]).min()) for k in ("hw1", "hwf", "hv")}


def assert_clear_of_kinks(r, what):
    """The mixer's abs / relu kinks cannot be read back from the implementation under test; a sign decided the other
    way moves a gradient element by about one term in M, far above the tolerance. So the case must keep clear."""
    for k, v in kink_minima(r).items():
        assert v > KINK_EPS, ("{}: min|{}| = {:.3g} over live rows is within KINK_EPS = {:g} of the mixer's kink; "
                              "choose another seed for this case".format(what, k, v, KINK_EPS))


def grad_blocks(case):
    """{block name: (tensor name, index)}: the blocks each judged on their own max. Every parameter tensor; fc1.weight
    by columns into obs / last-action / agent-id (as the case's flags give); the GRU's four tensors by rows into
    r / z / n; hyper_w_1.weight / .bias into the n per-agent row blocks of E."""
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
    for k in ("rnn.weight_ih", "rnn.weight_hh", "rnn.bias_ih", "rnn.bias_hh"):
        for j, gate in enumerate("rzn"):
            blocks["{}[{}]".format(k, gate)] = (k, (slice(j * H, (j + 1) * H),))
    if case.mixer == "qmix":
        for k in ("hyper_w_1.weight", "hyper_w_1.bias"):
            for a in range(case.n):
                blocks["{}[agent{}]".format(k, a)] = (k, (slice(a * E, (a + 1) * E),))
    return blocks


def block_errors(got_flat, ref_named, case, blocks=None):
    """{block: max|got - ref| / max|ref|} of a flat gradient against a named float64 one. A block whose reference max
    is exactly 0 (a last-action column block of actions never taken) is measured on its parent tensor's max.
    blocks: another table over case.unflatten's tensors than grad_blocks(case) (tests/coma_ref64.py: the critic's)."""
    got = case.unflatten(np.asarray(got_flat, np.float64))
    out = OrderedDict()
    for name, (k, idx) in (grad_blocks(case) if blocks is None else blocks).items():
        ref = np.asarray(ref_named[k], np.float64)
        scale = float(np.abs(ref[idx]).max())
        if scale == 0.0:
            scale = float(np.abs(ref).max())
        out[name] = float(np.abs(got[k][idx] - ref[idx]).max()) / max(scale, 1e-300)
    return out


def tolerances(e32):
    """The allowed error per block from the fp32 oracle's own error e32 against ref64 (module docstring)."""
    return OrderedDict((k, min(TOL_CAP, TOL_ROOM * max(v, E32_FLOOR))) for k, v in e32.items())


def ratios(errs, e32):
    """err / max(e32, E32_FLOOR) per block: the figure recorded per case (a block passes its tolerance while this is
    <= TOL_ROOM and err <= TOL_CAP)."""
    return OrderedDict((k, errs[k] / max(e32[k], E32_FLOOR)) for k in errs)


def failures(errs, tol):
    """The blocks over their tolerance, as {block: (err, tol)}."""
    return OrderedDict((k, (errs[k], tol[k])) for k in errs if not errs[k] <= tol[k])


# The shapes of tests/test_gpu_grad_blocks.py: (n, A, O, S, T, B), n_episodes = B, ragged with min_len = 1, the
# SynthCase default seeds. Each is the smallest at which its path still has the thing that can go wrong.
SHAPES = {
    "base": dict(n=3, A=9, O=30, S=48, T=17, B=4),        # fused pair forward, lean fused BPTT, hyper ws, R = 12
    "lds": dict(n=3, A=5, O=20, S=30, T=12, B=4),         # S % 4 != 0: the LDS hypernet
    "gemm": dict(n=2, A=6, O=24, S=200, T=9, B=3),        # S > 192: the hypernet as a GEMM
    "fast32": dict(n=3, A=17, O=20, S=32, T=12, B=4),     # A = 17: past the fused kernels, the 32-action fast mixer
    "stream": dict(n=17, A=5, O=16, S=40, T=6, B=2),      # n = 17: past the fast mixers
    "tiles_r21": dict(n=7, A=9, O=30, S=48, T=17, B=3),   # R = 21: partial 16-row and 32-row tiles
    "tiles_kq40": dict(n=3, A=5, O=100, S=48, T=6, B=4),  # O in 81..160: the <40> tile kernels
    "tiles_kq80": dict(n=3, A=5, O=300, S=48, T=4, B=4),  # O in 289..320: the <80> tile kernels
    "wide": dict(n=8, A=6, O=12, S=20, T=12, B=72),       # R = 576 > 512: VDN only (2e5 hypernet outputs would
}                                                         # hold values inside KINK_EPS)


def synth_case(shape, mixer="qmix", steps=2):
    from tests.golden_utils import SynthCase
    d = SHAPES[shape]
    return SynthCase("{}_{}".format(shape, mixer), n_episodes=d["B"], steps=steps, mixer=mixer, ragged=True,
                     min_len=1, **d)
