"""An independent float64 reference of one COMALearner.train(), and the per-block gate of the COMA critic and actor.

`coma_ref64_step` restates the whole train() in torch float64 on the CPU and lets autograd differentiate it: the critic
inputs (state | obs | joint one-hot actions with the agent's own block zeroed | last joint actions | agent id), the
target critic's all-steps pass, build_td_lambda_targets, then for t reversed over the live steps one critic step each
(forward with the current critic, masked L2 loss, autograd, clip_grad_norm_, RMSprop), and the actor (the agent unroll
of tests/ref64.py, the pi_logits policy for both values of mask_before_softmax with the epsilon floor, the renormalised
masked policy, the counterfactual baseline on the chain's per-step Q, detached, the loss, autograd, clip, RMSprop).
It shares no hand-derived backward with oracle/coma_np.py or with the kernels (coma_chain.hpp, coma_kernels.hpp); only
`critic_input_dim` / `critic_param_shapes` and the config constants are taken from the oracle's side.

The gate is the one of tests/ref64.py (its `block_errors`, `tolerances`, `ratios`, `failures`, E32_FLOOR, TOL_ROOM,
TOL_CAP), over the blocks of `coma_blocks`: every critic tensor, fc1.weight also by input kind (the one-hot columns are
orders of magnitude smaller than the dense ones), and ref64.grad_blocks' split of the agent tensors. `judge` applies
it to the four quantities a train() leaves behind: the last live step's clipped critic gradient, the critic's
square_avg (every live step's g^2), the critic update p_after - p_before, and the agent's clipped gradient.

The relus cannot be read back from the kernels. `kink_minima` of a step is the smallest |pre-activation| over live
(mask = 1) rows of the critic's two relus, each live step at its own parameter version, and of the agent's fc1 relu;
a row of SHAPES is only valid with a seed that keeps them above the row's margin (DESIGN.md "Parity").
"""
from __future__ import annotations

from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch as th

from tests import ref64
from tests.ref64 import F64

DELTA_CAP = 1e-3   # the critic update: a wrong sign, a dropped row or a missed step moves it by O(1) of its block
CRITIC_Q = ("cgrad_last", "csq", "cdelta")   # the critic-side quantities `judge` gates, then "agrad"


def agent_view(case):
    return ref64.FlatView(case, case.agent_shapes, True, True)


def critic_view(case):
    return ref64.FlatView(case, case.critic_shapes, False, True)


def coma_blocks(case):
    """{"critic": blocks, "agent": blocks}, each {block name: (tensor name, index)} as ref64.grad_blocks gives them."""
    full = slice(None)
    critic = OrderedDict((k, (k, (full,))) for k in case.critic_shapes)
    o = 0
    for kind, w in (("state", case.S), ("obs", case.O), ("actions", case.n * case.A),
                    ("last_actions", case.n * case.A), ("agent_id", case.n)):
        critic["fc1.weight[{}]".format(kind)] = ("fc1.weight", (full, slice(o, o + w)))
        o += w
    assert o == case.K
    return dict(critic=critic, agent=ref64.grad_blocks(agent_view(case)))


def flat_of(named_arrays):   # of any {name: array}; ref64.flat_of is of a case's initial parameters
    return np.concatenate([np.asarray(v).ravel() for v in named_arrays.values()])


def _t64(a):
    return th.tensor(np.asarray(a, np.float64), dtype=F64)


def _critic_inputs(state, obs, onehot, n):
    """COMACritic._build_inputs with t=None: (B, Tp, n, S + O + 2 n A + n)."""
    B, Tp, _, A = onehot.shape
    st = state.unsqueeze(2).expand(B, Tp, n, state.shape[-1])
    own = 1.0 - th.eye(n, dtype=F64).repeat_interleave(A, dim=1)            # (n, n A): 0 on the agent's own block
    joint = onehot.reshape(B, Tp, 1, n * A).expand(B, Tp, n, n * A)
    last = th.cat([th.zeros_like(onehot[:, :1]), onehot[:, :-1]], 1).reshape(B, Tp, 1, n * A).expand(B, Tp, n, n * A)
    eye = th.eye(n, dtype=F64).expand(B, Tp, n, n)
    return th.cat([st, obs, joint * own, last, eye], -1)


def _critic(cp, x):
    z1 = x @ cp["fc1.weight"].T + cp["fc1.bias"]
    z2 = th.relu(z1) @ cp["fc2.weight"].T + cp["fc2.bias"]
    return z1, z2, th.relu(z2) @ cp["fc3.weight"].T + cp["fc3.bias"]


def _rmsprop(p, g, sq, lr, alpha, eps):   # in place on {name: torch tensor}; ref64.rmsprop is on flat numpy vectors
    for k in p:
        sq[k] = alpha * sq[k] + (1.0 - alpha) * g[k] * g[k]
        p[k] = p[k] - lr * g[k] / (sq[k].sqrt() + eps)


def _policy(logits, avail, epsilon, mask_before_softmax):
    """BasicMAC.forward's pi_logits branch (test_mode False), then the learner's renormalised masked policy. A row
    with no available action (an unwritten slot) gets pi = 0 and no gradient."""
    off = avail == 0
    lg = logits.masked_fill(off, -1e10) if mask_before_softmax else logits
    sm = th.softmax(lg, -1)
    if mask_before_softmax:
        nact = avail.sum(-1, keepdim=True).to(F64).clamp(min=1.0)
    else:
        nact = float(logits.shape[-1])
    out = ((1.0 - epsilon) * sm + epsilon / nact).masked_fill(off, 0.0)
    s = out.sum(-1, keepdim=True)
    return (out / th.where(s == 0, th.ones_like(s), s)).masked_fill(off, 0.0)


def coma_ref64_step(case, agent, critic, target_critic, agent_sq, critic_sq, batch, epsilon):
    """One COMALearner.train() in float64.

    agent / critic / target_critic / agent_sq / critic_sq: flat float32 vectors as read from the learner (parameters()
    order); batch: the numpy batch of case.batch(k); epsilon: the MAC's action_selector.epsilon.
    Returns a namespace, every gradient / parameter as {tensor name: float64 numpy}:
    live_steps (t of every critic step taken, in the order taken), critic_grads / critic_norms / mask_sums (per live
    step; the gradients clipped), critic_params, critic_sq, critic_delta (final - initial), q_vals (B,T,n,A; 0 at
    skipped steps), targets (B,T,n), pi (B,T,n,A), agent_grads (clipped), agent_norm, agent_params, agent_sq,
    stats (the nine and critic_steps), kink_minima {critic_fc1, critic_fc2, agent_fc1}, mask (B,T,n), critic_pre (per
    live step: both relus' pre-activations (R,128) and the live rows), agent_pre (B,T,n,64)."""
    cfg = case.cfg()
    n, A = case.n, case.A
    f32 = lambda v: float(np.float32(v))  # noqa: E731  (the reference multiplies fp32 tensors by these scalars)
    gamma, lam = cfg["gamma"], cfg["td_lambda"]
    lg_, og_ = f32(lam * gamma), f32((1.0 - lam) * gamma)
    clip, alpha, eps = cfg["grad_norm_clip"], cfg["optim_alpha"], cfg["optim_eps"]
    av, cv = agent_view(case), critic_view(case)

    obs, onehot, state = _t64(batch["obs"]), _t64(batch["actions_onehot"]), _t64(batch["state"])
    rewards = _t64(batch["reward"][:, :-1])
    terminated = _t64(batch["terminated"][:, :-1])
    actions_all = th.tensor(np.asarray(batch["actions"], np.int64))
    mask = _t64(batch["filled"][:, :-1]).clone()
    mask[:, 1:] = mask[:, 1:] * (1.0 - terminated[:, :-1])
    avail = th.tensor(np.asarray(batch["avail_actions"][:, :-1]))
    B, Tp = obs.shape[:2]
    T = Tp - 1

    # ---- critic prologue: the target critic over every stored step, TD(lambda) (rl_utils.py:4-14)
    X = _critic_inputs(state, obs, onehot, n)
    ctp = {k: _t64(v) for k, v in cv.unflatten(np.asarray(target_critic)).items()}
    tq = th.gather(_critic(ctp, X)[2], 3, actions_all).squeeze(3)           # (B, Tp, n)
    ret = th.zeros_like(tq)
    ret[:, -1] = tq[:, -1] * (1.0 - terminated.sum(1))
    for t in range(T - 1, -1, -1):
        ret[:, t] = lg_ * ret[:, t + 1] + mask[:, t] * (rewards[:, t] + og_ * tq[:, t + 1] * (1.0 - terminated[:, t]))
    targets = ret[:, :-1]

    # ---- the critic's chain: one optimiser step per live t, reversed
    cp = OrderedDict((k, _t64(v)) for k, v in cv.unflatten(np.asarray(critic)).items())
    csq = OrderedDict((k, _t64(v)) for k, v in cv.unflatten(np.asarray(critic_sq)).items())
    cp0 = OrderedDict((k, v.clone()) for k, v in cp.items())
    q_vals = th.zeros(B, T, n, A, dtype=F64)
    live_steps, cgrads, cnorms, msums, cpre = [], [], [], [], []
    log = {k: [] for k in ("critic_loss", "td_error_abs", "q_taken_mean", "target_mean")}
    kink1 = kink2 = float("inf")
    for t in reversed(range(T)):
        mask_t = mask[:, t].expand(B, n)
        msum = float(mask_t.sum())
        if msum == 0:
            continue
        leaf = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in cp.items())
        z1, z2, q = _critic(leaf, X[:, t].reshape(B * n, -1))
        q_vals[:, t] = q.detach().reshape(B, n, A)
        q_taken = th.gather(q.reshape(B, n, A), 2, actions_all[:, t]).squeeze(2)
        mtd = (q_taken - targets[:, t]) * mask_t
        loss = (mtd ** 2).sum() / msum
        loss.backward()
        norm, g = ref64.clip(OrderedDict((k, v.grad.clone()) for k, v in leaf.items()), clip, F64)
        live = (mask_t > 0).reshape(-1)
        kink1 = min(kink1, float(z1.detach()[live].abs().min()))
        kink2 = min(kink2, float(z2.detach()[live].abs().min()))
        cpre.append((z1.detach().numpy(), z2.detach().numpy(), live.numpy()))
        _rmsprop(cp, g, csq, cfg["critic_lr"], alpha, eps)
        live_steps.append(t)
        cgrads.append(OrderedDict((k, v.numpy()) for k, v in g.items()))
        cnorms.append(norm)
        msums.append(msum)
        log["critic_loss"].append(loss.item())
        log["td_error_abs"].append(mtd.detach().abs().sum().item() / msum)
        log["q_taken_mean"].append((q_taken.detach() * mask_t).sum().item() / msum)
        log["target_mean"].append((targets[:, t] * mask_t).sum().item() / msum)

    # ---- the actor
    P = OrderedDict((k, _t64(v).requires_grad_(True)) for k, v in av.unflatten(np.asarray(agent)).items())
    logits, pre, _ = ref64.unroll(P, obs[:, :T], onehot[:, :T], (True, True), F64)
    pi = _policy(logits, avail, float(epsilon), bool(cfg.get("mask_before_softmax", True)))
    actions = actions_all[:, :-1]
    m = mask.expand(B, T, n)
    ms = float(m.sum())
    q_taken = th.gather(q_vals, 3, actions).squeeze(3)
    adv = (q_taken - (pi * q_vals).sum(-1)).detach()
    pi_taken = th.where(m == 0, th.ones_like(m), th.gather(pi, 3, actions).squeeze(3))
    coma_loss = -((adv * th.log(pi_taken)) * m).sum() / ms
    coma_loss.backward()
    anorm, ag = ref64.clip(OrderedDict((k, v.grad.clone()) for k, v in P.items()), clip, F64)
    ap = OrderedDict((k, v.detach().clone()) for k, v in P.items())
    asq = OrderedDict((k, _t64(v)) for k, v in av.unflatten(np.asarray(agent_sq)).items())
    _rmsprop(ap, ag, asq, cfg["lr"], alpha, eps)

    nl = max(len(live_steps), 1)
    stats = {k: sum(v) / nl for k, v in log.items()}
    stats["critic_grad_norm"] = sum(cnorms) / nl
    stats.update(advantage_mean=(adv * m).sum().item() / ms, coma_loss=coma_loss.item(), agent_grad_norm=anorm,
                 pi_max=(pi.detach().max(-1)[0] * m).sum().item() / ms, critic_steps=len(live_steps))
    kinks = dict(critic_fc1=kink1, critic_fc2=kink2, agent_fc1=float(pre.detach()[m > 0].abs().min()))
    npd = lambda d: OrderedDict((k, v.detach().numpy()) for k, v in d.items())  # noqa: E731
    return SimpleNamespace(
        live_steps=live_steps, critic_grads=cgrads, critic_norms=cnorms, mask_sums=msums, critic_params=npd(cp),
        critic_sq=npd(csq), critic_delta=OrderedDict((k, (cp[k] - cp0[k]).numpy()) for k in cp),
        critic_params0=npd(cp0), q_vals=q_vals.numpy(), targets=targets.numpy(), pi=pi.detach().numpy(),
        agent_grads=OrderedDict((k, v.numpy()) for k, v in ag.items()), agent_norm=anorm, agent_params=npd(ap),
        agent_sq=npd(asq), stats=stats, kink_minima=kinks, mask=m.numpy(), critic_pre=cpre,
        agent_pre=pre.detach().numpy())


# ---- the fp32 oracle from the same state, and the gate over both ---------------------------------------------------

def oracle_at(case, agent, critic, target_critic, agent_sq, critic_sq):
    """An OracleCOMALearner holding the given flat float32 state."""
    from oracle.coma_np import OracleCOMALearner
    av, cv = agent_view(case), critic_view(case)
    f = lambda view, flat: OrderedDict(  # noqa: E731
        (k, np.array(v, np.float32)) for k, v in view.unflatten(np.asarray(flat, np.float32)).items())
    o = OracleCOMALearner(f(av, agent), f(cv, critic), case.cfg())
    o.ctp, o.sq, o.csq = f(cv, target_critic), f(av, agent_sq), f(cv, critic_sq)
    return o


def oracle_quantities(o, critic_before):
    """The four gated quantities of an oracle after its train(), flat: as a learner's buffers hold them."""
    return dict(cgrad_last=flat_of(o.last["critic_grads"][-1]), csq=o.flat("critic_sq"),
                cdelta=o.flat("critic").astype(np.float64) - np.asarray(critic_before, np.float64),
                agrad=flat_of(o.last["agent_grads"]))


def reference_quantities(r):
    return dict(cgrad_last=r.critic_grads[-1], csq=r.critic_sq, cdelta=r.critic_delta, agrad=r.agent_grads)


def delta_floor(r, blocks):
    """Per block, what fp32 storage of the parameters leaves of the update: 2^-24 max|p| / max|delta|."""
    out = OrderedDict()
    for name, (k, idx) in blocks.items():
        d = float(np.abs(r.critic_delta[k][idx]).max())
        p = float(max(np.abs(r.critic_params[k][idx]).max(), np.abs(r.critic_params0[k][idx]).max()))
        out[name] = 2.0 ** -24 * p / max(d, 1e-300)
    return out


def judge(case, r, got, orc):
    """The gate on one train(): `got` and `orc` are {quantity: flat vector} of the implementation under test and of
    the fp32 oracle from the same state (oracle_quantities), `r` the reference's step. Returns
    ({quantity: {block: dict(err, e32, tol, ratio)}}, [(quantity, block, err, tol) over tolerance])."""
    blocks = coma_blocks(case)
    ref = reference_quantities(r)
    rec, bad = OrderedDict(), []
    for q in CRITIC_Q + ("agrad",):
        view, bl = (agent_view(case), blocks["agent"]) if q == "agrad" else (critic_view(case), blocks["critic"])
        e32 = ref64.block_errors(orc[q], ref[q], view, bl)
        errs = ref64.block_errors(got[q], ref[q], view, bl)
        if q == "cdelta":
            fl = delta_floor(r, bl)
            tol = OrderedDict((k, min(DELTA_CAP, ref64.TOL_ROOM * max(e32[k], ref64.E32_FLOOR, fl[k]))) for k in e32)
            ratio = OrderedDict((k, errs[k] / max(e32[k], ref64.E32_FLOOR, fl[k])) for k in errs)
        else:
            tol, ratio = ref64.tolerances(e32), ref64.ratios(errs, e32)
        rec[q] = OrderedDict((b, dict(err=errs[b], e32=e32[b], tol=tol[b], ratio=ratio[b])) for b in errs)
        bad += [(q, b, e, t) for b, (e, t) in ref64.failures(errs, tol).items()]
    return rec, bad


def worst(rec):
    """(quantity, block, ratio) of the largest err / max(e32, floor) of a `judge` record."""
    return max(((q, b, v["ratio"]) for q, d in rec.items() for b, v in d.items()), key=lambda x: x[2])


# ---- the shapes of tests/test_gpu_coma_blocks.py ---------------------------------------------------------------------
# (n, A, O, S, B, T), n_episodes = B, ragged with min_len = 1; Kc = S + O + 2 n A + n, R = B n. Each is the smallest
# shape at which its edge exists (DESIGN.md "Parity" has the table with the reasons). mbs alternates: coma_smac.yaml
# uses mask_before_softmax False, the masked path True. The rows with R >= 78 use T = 2.
# `seed` is the outcome of the bounded search of tests/test_coma_ref64_host.py (its __main__; seeds 0..63 in order, only
# those whose batch reaches the full T), `margin` what the GPU test asserts of kink_minima and the CPU test twice:
# * the first seed whose kink_minima of both steps exceed 2 * ref64.KINK_EPS, margin = KINK_EPS: every row but two
#   (r78: 2 seeds of 64 reach it, r81: 2 of 64; the rows with R <= 20: most);
# * a32_r80 (2560 + 10240 critic pre-activations per step, largest minimum of 64 seeds 9.0e-6) and r129 (1.4e-5) do
#   not reach it: the first seed whose minima exceed 3 x rule, rule = max(1e-6, 8 x `pre_err`), pre_err the fp32
#   oracle's largest pre-activation error against this reference over the row's live rows (measured on the CPU, never
#   against the GPU), and margin = 1.25 x rule rounded up.
# Measured minima over both steps at these seeds: r9 4.2e-5, t1 2.8e-5, r9_holes 2.4e-5, r17_k113 2.9e-5,
# k224_a16 2.2e-5, a17_k112 3.8e-5, k63 7.1e-5, k64 5.8e-5, k176 2.4e-5, k177 6.7e-5, r78 2.2e-5, a32_r80 5.1e-6,
# r81 3.1e-5, a33 3.2e-5, r129 1.4e-5.
SHAPES = OrderedDict([
    ("r9", dict(n=3, A=5, O=12, S=20, B=3, T=5, mbs=False, seed=5, margin=1e-5)),
    ("t1", dict(n=3, A=5, O=12, S=20, B=3, T=1, mbs=True, seed=0, margin=1e-5)),
    # T = 5 of the batch that runs: the replay has 8 slots, and the sum(filled) truncation that both the buffer and
    # case.batch apply takes the two unwritten slots off the end, leaving slots 0..5 with filled = 1 0 1 0 1 1
    ("r9_holes", dict(n=3, A=5, O=12, S=20, B=3, T=7, mbs=True, seed=4, margin=1e-5, holes=(1, 3), live=[4, 2, 0])),
    ("r17_k113", dict(n=17, A=2, O=6, S=22, B=1, T=4, mbs=False, seed=6, margin=1e-5)),
    ("k224_a16", dict(n=4, A=16, O=32, S=60, B=5, T=4, mbs=True, seed=4, margin=1e-5)),
    ("a17_k112", dict(n=2, A=17, O=12, S=30, B=3, T=4, mbs=False, seed=1, margin=1e-5)),
    ("k63", dict(n=3, A=5, O=10, S=20, B=3, T=4, mbs=True, seed=0, margin=1e-5)),
    ("k64", dict(n=3, A=5, O=11, S=20, B=3, T=4, mbs=False, seed=1, margin=1e-5)),
    ("k176", dict(n=3, A=5, O=43, S=100, B=3, T=4, mbs=True, seed=0, margin=1e-5)),
    ("k177", dict(n=3, A=5, O=44, S=100, B=3, T=4, mbs=False, seed=14, margin=1e-5)),
    ("r78", dict(n=6, A=5, O=12, S=20, B=13, T=2, mbs=True, seed=26, margin=1e-5)),
    ("a32_r80", dict(n=8, A=32, O=8, S=16, B=10, T=2, mbs=False, seed=5, margin=1.4e-6, pre_err=1.36e-7)),
    ("r81", dict(n=9, A=5, O=12, S=20, B=9, T=2, mbs=True, seed=12, margin=1e-5)),
    ("a33", dict(n=2, A=33, O=12, S=20, B=3, T=4, mbs=False, seed=3, margin=1e-5)),
    ("r129", dict(n=3, A=5, O=12, S=20, B=43, T=2, mbs=True, seed=45, margin=3.7e-6, pre_err=3.62e-7)),
])
KC = dict(r9=65, t1=65, r9_holes=65, r17_k113=113, k224_a16=224, a17_k112=112, k63=63, k64=64, k176=176, k177=177,
          r78=98, a32_r80=544, r81=131, a33=166, r129=65)
CHAIN_ROWS = [k for k in SHAPES if k not in ("r81", "a33", "r129")]   # B n <= 80 and A <= 32: the persistent chain
EPSILON = (0.5, 0.3)   # the MAC's action_selector.epsilon at the two steps


def synth_case(row, seed=None):
    from tests.golden_utils import SynthComaCase
    d = SHAPES[row]
    c = SynthComaCase(row, d["n"], d["A"], d["O"], d["S"], d["T"], d["B"], d["seed"] if seed is None else seed,
                      d["mbs"], epsilon=EPSILON)
    for h in d.get("holes", ()):   # slots left unwritten in every episode: the steps there are skipped
        c.data["filled"][:, h] = 0
        c.data["actions"][:, h] = 0
        c.data["actions_onehot"][:, h] = 0.0
    assert c.K == KC[row], (row, c.K)
    return c
