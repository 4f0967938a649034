"""An independent float64 reference of one QMIX / VDN / IQL learner step, and the per-block gradient gate built on it.

`ref_step` restates the step's loss in torch on the CPU and lets autograd differentiate it: agent unroll over
`[obs | last-action one-hot | agent id]`, fc1 -> relu -> GRU cell (or, under use_rnn: False, Linear -> relu) -> fc2,
double-Q or max target, QMixer with a one- or two-layer hypernet / sum / none, the -9999999 masks and the masked L2
loss. It shares no hand-derived backward with the numpy oracle (oracle/qlearner_np.py) or with the kernels; only
constants are taken from the oracle. The three opt-in tails are restated the same way: TD(lambda) targets
(`lambda_returns`: the reference's build_td_lambda_targets recurrence in the run's dtype), the masked Huber loss
(`td_loss`, differentiated by autograd) and prioritized replay's per-episode importance weights on the loss.
COMA's train() and the actor-critic learner's have their own references on the same gate and the same helpers in
tests/coma_ref64.py and tests/a2c_ref.py.

In float64 `ref_step` is the reference. In float32 its error against the float64 run is `e32` for the cases the
oracle does not cover (the two-layer hypernet, tests/hyper2_ref.py; the feed-forward agent, tests/ffn_ref.py).

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

The comparison has discrete decisions that may differ under fp32 rounding. The double-Q argmax, the fc1 relu, the
feed-forward agent's second relu and the two-layer hypernet's layer-1 relu are taken from the implementation under
test (`cur_max_override`, `relu_override`, `hid_relu_override`, `hyp_relu_override`); `classify` counts where they
differ from the reference's own outside near-ties (`near_ties`, MARGIN_EPS, RELU_EPS). The mixer's kinks (abs on
hw1 / hwf, V's relu on hv) cannot be read back, so `kink_minima` / `assert_clear_of_kinks` require every such
pre-activation of a live row to be further than KINK_EPS from 0.
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
MARGIN_EPS = 1e-5   # argmax-equal wherever the top-2 gap exceeds 1e-5 * max(1, |Q|)
RELU_EPS = 1e-5
F64 = th.float64


def named(case, flat, grad, dtype):
    """Case.unflatten's layout as torch tensors of `dtype` (leaf tensors with grad when `grad`)."""
    out = OrderedDict()
    for k, v in case.unflatten(np.asarray(flat)).items():
        t = th.tensor(np.asarray(v, np.float64), dtype=dtype)
        out[k] = t.requires_grad_(True) if grad else t
    return out


def unroll(p, obs, onehot, flags, dtype, relu_mask=None, hid_mask=None):
    """BasicMAC.forward over t. obs (B,Tp,n,O), onehot (B,Tp,n,A) -> Q (B,Tp,n,A), the fc1 pre-activations (B,Tp,n,H)
    and, for the feed-forward agent (`rnn.weight` in p: nothing carried from step to step), its second relu's
    pre-activations (B,Tp,n,H), else None. relu_mask / hid_mask: the other implementation's on/off decisions, a
    constant 0/1 factor on the pre-activation."""
    B, Tp, n, _ = obs.shape
    A = onehot.shape[-1]
    Hd = p["fc1.weight"].shape[0]
    gru = "rnn.weight_ih" in p
    eye = th.eye(n, dtype=dtype).expand(B, n, n)
    h = th.zeros(B * n, Hd, dtype=dtype)
    qs, pres, pre2s = [], [], []
    for t in range(Tp):
        parts = [obs[:, t]]
        if flags[0]:
            parts.append(th.zeros(B, n, A, dtype=dtype) if t == 0 else onehot[:, t - 1])
        if flags[1]:
            parts.append(eye)
        x = th.cat(parts, -1).reshape(B * n, -1)
        pre = x @ p["fc1.weight"].T + p["fc1.bias"]
        pres.append(pre.reshape(B, n, Hd))
        x1 = th.relu(pre) if relu_mask is None else pre * relu_mask[:, t].reshape(B * n, Hd)
        if gru:
            gi = x1 @ p["rnn.weight_ih"].T + p["rnn.bias_ih"]
            gh = h @ p["rnn.weight_hh"].T + p["rnn.bias_hh"]
            r = th.sigmoid(gi[:, :Hd] + gh[:, :Hd])
            z = th.sigmoid(gi[:, Hd:2 * Hd] + gh[:, Hd:2 * Hd])
            c = th.tanh(gi[:, 2 * Hd:] + r * gh[:, 2 * Hd:])
            h = (1.0 - z) * c + z * h
        else:
            pre2 = x1 @ p["rnn.weight"].T + p["rnn.bias"]
            pre2s.append(pre2.reshape(B, n, Hd))
            h = th.relu(pre2) if hid_mask is None else pre2 * hid_mask[:, t].reshape(B * n, Hd)
        qs.append((h @ p["fc2.weight"].T + p["fc2.bias"]).reshape(B, n, A))
    return th.stack(qs, 1), th.stack(pres, 1), None if gru else th.stack(pre2s, 1)


def qmix(mp, agent_qs, states, n, hyp_relu=None):
    """QMixer.forward with a one- or two-layer hypernet (`hyper_w_1.0.weight` in mp). agent_qs (B,T,n), states (B,T,S)
    -> y (B,T,1), the pre-abs / pre-relu hypernet outputs hw1, hwf, hv and, with two layers, the layer-1
    pre-activations a1 (B*T, 2 He) = [hyper_w_1.0 | hyper_w_final.0] (else None). hyp_relu (B*T, 2 He): 0/1 factors in
    place of the layer-1 relu's own decisions."""
    B, T = agent_qs.shape[:2]
    Em = mp["hyper_b_1.weight"].shape[0]   # the module constant on every learner case; tests/act_ref64.py: 1 .. 64
    s = states.reshape(B * T, -1)
    q = agent_qs.reshape(B * T, 1, n)
    a1 = None
    if "hyper_w_1.0.weight" in mp:
        a1w = s @ mp["hyper_w_1.0.weight"].T + mp["hyper_w_1.0.bias"]
        a1f = s @ mp["hyper_w_final.0.weight"].T + mp["hyper_w_final.0.bias"]
        He = a1w.shape[1]
        if hyp_relu is None:
            x1w, x1f = th.relu(a1w), th.relu(a1f)
        else:
            x1w, x1f = a1w * hyp_relu[:, :He], a1f * hyp_relu[:, He:]
        hw1 = x1w @ mp["hyper_w_1.2.weight"].T + mp["hyper_w_1.2.bias"]
        hwf = x1f @ mp["hyper_w_final.2.weight"].T + mp["hyper_w_final.2.bias"]
        a1 = th.cat([a1w, a1f], 1)
    else:
        hw1 = s @ mp["hyper_w_1.weight"].T + mp["hyper_w_1.bias"]
        hwf = s @ mp["hyper_w_final.weight"].T + mp["hyper_w_final.bias"]
    b1 = s @ mp["hyper_b_1.weight"].T + mp["hyper_b_1.bias"]
    hid = th.nn.functional.elu(th.bmm(q, hw1.abs().reshape(B * T, n, Em)) + b1.reshape(B * T, 1, Em))
    hv = s @ mp["V.0.weight"].T + mp["V.0.bias"]
    v = th.relu(hv) @ mp["V.2.weight"].T + mp["V.2.bias"]
    y = th.bmm(hid, hwf.abs().reshape(B * T, Em, 1)) + v.reshape(B * T, 1, 1)
    return y.reshape(B, T, 1), hw1, hwf, hv, a1


def clip(grads, max_norm, dtype):
    """clip_grad_norm_ on {name: gradient}: (norm, clipped). Under float32 the norm is accumulated in the run's own
    precision (numpy arrays); under float64 numpy arrays and torch tensors both pass."""
    if dtype == F64:
        norm = float(np.sqrt(sum(float((g * g).sum()) for g in grads.values())))
        coef = min(max_norm / (norm + 1e-6), 1.0)
    else:
        g32 = [g.astype(np.float32) for g in grads.values()]
        norm32 = np.sqrt(np.sum(np.array([np.sum(g * g, dtype=np.float32) for g in g32], np.float32),
                                dtype=np.float32))
        norm = float(norm32)
        coef = float(min(np.float32(max_norm) / (norm32 + np.float32(1e-6)), np.float32(1.0)))
    return norm, OrderedDict((k, g * coef) for k, g in grads.items())


def lambda_returns(rew, term, mask, y, gamma, lam):
    """The reference's build_td_lambda_targets, as tests/lambda_oracle.td_lambda_returns states it, in the tensors'
    own dtype: rew, term, mask (B, L, 1), y = y' (B, L, k), y'[:, t] the target net's value at step t + 1.
    Returns (targets (B, L, k), bootstrap (B, k) = y'[L-1] (1 - sum_t term))."""
    lg, og = lam * gamma, (1.0 - lam) * gamma
    L = y.shape[1]
    boot = y[:, L - 1] * (1.0 - term.sum(1))
    ret, out = boot, [None] * L
    for t in range(L - 1, -1, -1):
        ret = lg * ret + mask[:, t] * (rew[:, t] + og * y[:, t] * (1.0 - term[:, t]))
        out[t] = ret
    return th.stack(out, 1), boot


def td_loss(td, m, delta):
    """The loss term per transition on x = td * m: x^2, or with delta > 0 the Huber form 0.5 x^2 for |x| <= delta,
    else delta (|x| - 0.5 delta). Returns (term, x)."""
    x = td * m
    if delta > 0:
        ax = x.abs()
        return th.where(ax <= delta, 0.5 * x * x, delta * (ax - 0.5 * delta)), x
    return x ** 2, x


def ref_step(case, flat_params, flat_targets, batch, dtype=F64, cur_max_override=None, relu_override=None,
             hid_relu_override=None, hyp_relu_override=None, td_lambda=None, huber_delta=0.0, weights=None):
    """One learner step's loss and its autograd gradient in `dtype`.

    The agent is read from the case's parameter names (`rnn.weight_ih`: GRU; `rnn.weight`: feed-forward), the mixer
    from case.mixer and case.He (absent or None: one hypernet layer). flat_params / flat_targets: flat float32 vectors
    in Case.unflatten's layout; batch: the numpy batch of case.batch(k). cur_max_override (B,T,n) / relu_override
    (B,T+1,n,H): as in OracleQLearner.forward; hid_relu_override (B,T+1,n,H) bool: the feed-forward agent's second
    relu; hyp_relu_override (B,T,2 He) bool: the online two-layer hypernet's layer-1 relu.
    td_lambda: None for the one-step target, else lambda of `lambda_returns` over the target-side mix y' (per agent
    without a mixer), lambda and gamma as the C ABI carries them (rounded to f32). huber_delta > 0: `td_loss`'s Huber
    form (delta rounded to f32 likewise). weights (B,): loss = sum_b w_b sum_t l(td m) / sum m; the other four stats
    stay unweighted (tests/per_oracle.py).
    Returns a namespace, every array float64 numpy: grads (raw, per named tensor), norm, clipped (per named tensor),
    clipped_flat, loss, stats (the five), hw1 / hwf / hv ((B*T, .), None without a QMixer), a1 ((B,T,2 He), None
    without a two-layer hypernet), pre (fc1 pre-activations, (B,T+1,n,H)), mac_out, target_mac_out (masked, steps
    1..T), masked_q (the Q the target's argmax decision is taken on), cur_max_actions, mask (B,T,1 or n); for the
    feed-forward agent pre2 (its second relu's pre-activations), x1 / hid (both relus' outputs) and
    target_mac_out_full (unmasked, every step), None for the GRU; targets and y_next (y', the target-side mix), both
    (B,T,1 or n); bootstrap ((B,1 or n), None at the one-step target); mtd = td mask (B,T,1 or n) and abs_mtd, its
    absolute value as (B,T,1), summed over the agents without a mixer."""
    cfg = case.cfg()
    n, gamma = case.n, float(np.float32(cfg["gamma"]))
    flags = (bool(case.obs_last_action), bool(case.obs_agent_id))
    names = list(case.agent_shapes) + list(case.mixer_shapes)
    P = named(case, flat_params, True, dtype)
    TP = named(case, flat_targets, False, dtype)
    tt = lambda a: th.tensor(np.asarray(a, np.float64), dtype=dtype)  # noqa: E731
    mask01 = lambda a: None if a is None else tt(np.asarray(a, bool))  # noqa: E731
    obs, onehot = tt(batch["obs"]), tt(batch["actions_onehot"])
    rewards = tt(batch["reward"][:, :-1])
    terminated = tt(batch["terminated"][:, :-1])
    actions = th.tensor(np.asarray(batch["actions"][:, :-1], np.int64))
    avail = th.tensor(np.asarray(batch["avail_actions"]) != 0)
    mask = tt(batch["filled"][:, :-1]).clone()
    mask[:, 1:] = mask[:, 1:] * (1.0 - terminated[:, :-1])

    mac_out, pre, pre2 = unroll(P, obs, onehot, flags, dtype, mask01(relu_override), mask01(hid_relu_override))
    chosen = th.gather(mac_out[:, :-1], 3, actions).squeeze(3)
    B, T = chosen.shape[:2]
    with th.no_grad():
        tmo_full = unroll(TP, obs, onehot, flags, dtype)[0]
        tmo = tmo_full[:, 1:].masked_fill(~avail[:, 1:], float(NEG))
        masked_q = mac_out.detach().masked_fill(~avail, float(NEG))[:, 1:] if case.double_q else tmo
        cur_max = masked_q.argmax(3)
        if cur_max_override is not None:
            cur_max = th.tensor(np.asarray(cur_max_override, np.int64))
        target_max = th.gather(tmo, 3, cur_max.unsqueeze(3)).squeeze(3) if case.double_q else tmo.max(3)[0]
    hw1 = hwf = hv = a1 = None
    if case.mixer == "qmix":
        state = tt(batch["state"])
        hr = mask01(hyp_relu_override)
        q_tot, hw1, hwf, hv, a1 = qmix(P, chosen, state[:, :-1], n, None if hr is None else hr.reshape(B * T, -1))
        with th.no_grad():
            tq_tot = qmix(TP, target_max, state[:, 1:], n)[0]
    elif case.mixer == "vdn":
        q_tot, tq_tot = chosen.sum(2, keepdim=True), target_max.sum(2, keepdim=True)
    else:
        q_tot, tq_tot = chosen, target_max
    boot = None
    if td_lambda is None:
        targets = rewards + gamma * (1.0 - terminated) * tq_tot
    else:
        targets, boot = lambda_returns(rewards, terminated, mask, tq_tot, gamma, float(np.float32(td_lambda)))
    td = q_tot - targets.detach()
    m = mask.expand_as(td)
    ell, mtd = td_loss(td, m, float(np.float32(huber_delta)))
    msum = m.sum()
    if weights is not None:
        ell = tt(weights).reshape(B, 1, 1) * ell
    loss = ell.sum() / msum
    loss.backward()

    grads = OrderedDict((k, P[k].grad.double().numpy().copy()) for k in names)
    norm, clipped = clip(grads, cfg["grad_norm_clip"], dtype)
    ms = float(msum)
    with th.no_grad():
        stats = dict(loss=loss.item(), grad_norm=norm, td_error_abs=mtd.abs().sum().item() / ms,
                     q_taken_mean=(q_tot * m).sum().item() / (ms * n),
                     target_mean=(targets * m).sum().item() / (ms * n))
    det = lambda x: None if x is None else x.detach().double().numpy()  # noqa: E731
    ff = pre2 is not None
    return SimpleNamespace(grads=grads, norm=norm, clipped=clipped,
                           clipped_flat=np.concatenate([g.ravel() for g in clipped.values()]), loss=loss.item(),
                           stats=stats, hw1=det(hw1), hwf=det(hwf), hv=det(hv), pre=det(pre), pre2=det(pre2),
                           x1=det(th.relu(pre)) if ff else None, hid=det(th.relu(pre2)) if ff else None,
                           mac_out=det(mac_out), a1=None if a1 is None else det(a1).reshape(B, T, -1),
                           target_mac_out=det(tmo), target_mac_out_full=det(tmo_full) if ff else None,
                           masked_q=det(masked_q), cur_max_actions=cur_max.numpy(), mask=det(m),
                           targets=det(targets), y_next=det(tq_tot), bootstrap=det(boot),
                           mtd=det(mtd), abs_mtd=det(mtd.abs().sum(2, keepdim=True)))


def near_ties(masked_q, mask):
    """(tie, live), both (B,T,n) bool: the double-Q decisions whose top-2 margin is within MARGIN_EPS * max(1, |Q|),
    and the live transitions. Padded slots (every action masked) are ties by construction but never reach the loss."""
    top2 = -np.sort(-masked_q, axis=3)[..., :2]
    margin = top2[..., 0] - top2[..., 1]
    tie = margin <= MARGIN_EPS * np.maximum(1.0, np.abs(top2[..., 0]))
    return tie, np.broadcast_to(mask > 0, tie.shape)


def classify(r, got_cur_max, got_relu, got_hid_relu=None, got_hyp_relu=None):
    """The implementation's decisions (cur_max (B,T,n), fc1 relu (B,T+1,n,H) bool and, where given, the feed-forward
    agent's second relu (B,T+1,n,H) bool and the hypernet's layer-1 relu (B,T,2He) bool) against the float64
    reference's own (`r`, run without overrides from the same state): test_gpu_parity.classify_decisions' counts,
    plus those of the relus given. Flips outside near-ties must be 0."""
    tie, live = near_ties(r.masked_q, r.mask)
    dq_flip = np.asarray(got_cur_max) != r.cur_max_actions
    relu_tie = np.abs(r.pre) <= RELU_EPS
    relu_flip = np.asarray(got_relu, bool) != (r.pre > 0)
    out = dict(dq_decisions=int(live.sum()), dq_ties=int((tie & live).sum()), dq_flips=int(dq_flip.sum()),
               dq_flips_outside_ties=int((dq_flip & ~tie).sum()), relu_ties=int(relu_tie.sum()),
               relu_flips=int(relu_flip.sum()), relu_flips_outside_ties=int((relu_flip & ~relu_tie).sum()))
    for key, got, pre in (("hid_relu", got_hid_relu, r.pre2), ("hyp_relu", got_hyp_relu, r.a1)):
        if got is not None:
            t = np.abs(pre) <= RELU_EPS
            flip = np.asarray(got, bool) != (pre > 0)
            out.update({key + "_decisions": int(t.size), key + "_ties": int(t.sum()), key + "_flips": int(flip.sum()),
                        key + "_flips_outside_ties": int((flip & ~t).sum())})
    return out


def kink_minima(r):
    """min |hw1|, |hwf|, |hv| over the live rows (mask > 0) of a QMIX ref_step result."""
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
    by columns into obs / last-action / agent-id (as the case's flags give); a GRU's four tensors by rows into
    r / z / n; hyper_w_1.weight / .bias (two layers: hyper_w_1.2) into the n per-agent row blocks of E."""
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
    if "rnn.weight_ih" in case.agent_shapes:
        for k in ("rnn.weight_ih", "rnn.weight_hh", "rnn.bias_ih", "rnn.bias_hh"):
            for j, gate in enumerate("rzn"):
                blocks["{}[{}]".format(k, gate)] = (k, (slice(j * H, (j + 1) * H),))
    if case.mixer == "qmix":
        w1 = "hyper_w_1" if getattr(case, "He", None) is None else "hyper_w_1.2"
        for k in (w1 + ".weight", w1 + ".bias"):
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


def rmsprop(case, params, sq, clipped_flat):
    """torch.optim.RMSprop's step in float64 on flat vectors: (new params, new square_avg)."""
    cfg = case.cfg()
    g = np.asarray(clipped_flat, np.float64)
    sq = cfg["optim_alpha"] * np.asarray(sq, np.float64) + (1.0 - cfg["optim_alpha"]) * g * g
    return np.asarray(params, np.float64) - cfg["lr"] * g / (np.sqrt(sq) + cfg["optim_eps"]), sq


def adam(params, m, v, clipped_flat, t, lr=5e-4, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's step t (1-based) in float64 on flat vectors: (new params, exp_avg, exp_avg_sq)."""
    g = np.asarray(clipped_flat, np.float64)
    m = b1 * np.asarray(m, np.float64) + (1.0 - b1) * g
    v = b2 * np.asarray(v, np.float64) + (1.0 - b2) * g * g
    step = lr / (1.0 - b1 ** t)
    return np.asarray(params, np.float64) - step * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps), m, v


def flat_of(case):
    """The case's initial parameters as one flat vector, in Case.unflatten's layout."""
    return np.concatenate([v.ravel() for v in list(case.agent_params.values()) + list(case.mixer_params.values())])


class FlatView:
    """What grad_blocks / block_errors read of a case, over one flat parameter vector of an actor-critic case
    (tests/coma_ref64.py, tests/a2c_ref.py): the agent's (`agent`) or the critic's `shapes`."""

    def __init__(self, case, shapes, agent, obs_last_action):
        self.n, self.A, self.O = case.n, case.A, case.O
        self.agent_shapes = shapes if agent else OrderedDict()
        self.mixer_shapes = OrderedDict() if agent else shapes
        self.obs_last_action, self.obs_agent_id = obs_last_action, True
        self.mixer = "none"

    def unflatten(self, flat):
        out, o = OrderedDict(), 0
        for k, s in list(self.agent_shapes.items()) + list(self.mixer_shapes.items()):
            sz = int(np.prod(s))
            out[k] = flat[o:o + sz].reshape(s)
            o += sz
        return out


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


# The replay seeds of the TD(lambda) rows (tests/test_gpu_tail_blocks.py): `fast32` and `stream` have an episode of a
# single transition at the SynthCase default; `base` has none there, 46 is the first seed after it with one beside
# three episodes of (nearly) full length.
LAMBDA_SEEDS = {"base": 46, "fast32": 11, "stream": 11}


def lambda_case(shape, mixer="qmix", steps=2, data_seed=None):
    """synth_case for the TD(lambda) rows, a case of its own: one episode has a single transition, and the longest
    episode's `terminated` flag is cleared (make_replay terminates every episode shorter than T), so that the
    recurrence's bootstrap y'[L-1] (1 - sum term) is not zero."""
    case = synth_case(shape, mixer, steps, LAMBDA_SEEDS[shape] if data_seed is None else data_seed)
    lens = case.data["filled"].sum(1).reshape(-1)
    assert lens.min() == 2, (shape, lens)
    case.data["terminated"][int(np.argmax(lens))] = 0
    return case


def synth_case(shape, mixer="qmix", steps=2, data_seed=11):
    from tests.golden_utils import SynthCase
    d = SHAPES[shape]
    return SynthCase("{}_{}".format(shape, mixer), n_episodes=d["B"], steps=steps, mixer=mixer, ragged=True,
                     min_len=1, data_seed=data_seed, **d)
