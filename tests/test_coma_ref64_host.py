"""The float64 COMA reference (tests/coma_ref64.py) and the per-block gate built on it, checked on the CPU.

* the reference is right: chained in float64 over the golden run of the reference COMALearner (coma_tiny.npz), it gives
  the reference's last critic gradient, parameters, square_avg and stats, at tighter bounds than the fp32 oracle's test;
* the fp32 oracle passes the gate at every row of tests/test_gpu_coma_blocks.py, at both steps; its own error e32 per
  block is what the GPU tolerance is built from, so the worst is printed;
* the gate has teeth: four kernel-like faults planted in the oracle's last critic step on a small and a large row are
  named by block, while the checks tests/test_gpu_coma.py had before (the 1e-2 critic band, the flat 1e-4 agent gate)
  pass them;
* the kink condition: with the seed recorded in coma_ref64.SHAPES every relu pre-activation of a live row stays above
  twice the row's margin at both steps, and the margins of the large rows are what their rule says.

`python -m tests.test_coma_ref64_host` runs the bounded seed search (at most 64 seeds per row) and prints the table.
"""
from collections import OrderedDict

import numpy as np
import pytest

from tests import coma_ref64 as C
from tests import ref64
from tests.golden_utils import COMA_STATS, ComaCase, rel_err

F32 = np.float32
MAX_SEEDS = 64
CRITIC_BAND = 5e-4 * 20   # test_coma_teacher_forced: |p_gpu - p_oracle| <= 20 lr on the critic
AGENT_GATE = 1e-4         # and rel(flat agent gradient) < 1e-4


def initial_state(c):
    """(agent, critic, target critic, agent square_avg, critic square_avg) of a fresh learner, flat float32."""
    a, k = C.flat_of(c.agent_params), C.flat_of(c.critic_params)
    return a, k, k.copy(), np.zeros_like(a), np.zeros_like(k)


def oracle_preacts(record):
    """A stand-in for oracle.coma_np.critic_forward that also appends the fp32 pre-activations of both relus."""
    import oracle.coma_np as M
    orig = M.critic_forward

    def fwd(cp, x):
        z1 = (x @ cp["fc1.weight"].T + cp["fc1.bias"]).astype(F32)
        z2 = (np.maximum(z1, F32(0.0)) @ cp["fc2.weight"].T + cp["fc2.bias"]).astype(F32)
        record.append((z1, z2))
        return orig(cp, x)
    return fwd


def two_steps(c, monkeypatch=None):
    """Both train() steps of a row on the CPU: step 0 from the case's weights, step 1 from the oracle's state after
    it. Per step: the state, the batch, the reference's step, the oracle after its step, and (with monkeypatch) the
    oracle's largest pre-activation error against the reference over live rows."""
    import oracle.coma_np as M
    from oracle.qlearner_np import fc1_preacts
    out, state = [], initial_state(c)
    for k in range(2):
        nb, _ = c.batch(k)
        r = C.coma_ref64_step(c, *state, nb, c.epsilon[k])
        o = C.oracle_at(c, *state)
        rec, pre_err = [], None
        if monkeypatch is not None:
            monkeypatch.setattr(M, "critic_forward", oracle_preacts(rec))
        o.train(nb, 1000 * (k + 1), 8 * k, c.epsilon[k])
        if monkeypatch is not None:
            monkeypatch.undo()
            assert len(rec) == 1 + len(r.live_steps)   # the target pass, then the live steps
            pre_err = 0.0
            for (z1, z2), (r1, r2, live) in zip(rec[1:], r.critic_pre):
                pre_err = max(pre_err, np.abs(z1[live] - r1[live]).max(), np.abs(z2[live] - r2[live]).max())
            T = nb["obs"].shape[1] - 1
            ap = fc1_preacts(o_params_before(c, state), nb["obs"][:, :T], nb["actions_onehot"][:, :T], (True, True))
            pre_err = float(max(pre_err, np.abs(ap - r.agent_pre)[r.mask > 0].max()))
        out.append(dict(state=state, nb=nb, ref=r, oracle=o, pre_err=pre_err))
        state = tuple(o.flat(w) for w in ("agent", "critic", "target_critic", "sq", "critic_sq"))
    return out


def o_params_before(c, state):
    return OrderedDict((k, np.asarray(v, F32)) for k, v in C.agent_view(c).unflatten(np.asarray(state[0])).items())


@pytest.fixture(scope="module")
def rows():
    cache = {}

    def get(row):
        if row not in cache:
            cache[row] = (C.synth_case(row), two_steps(C.synth_case(row)))
        return cache[row]
    return get


# ---- the reference is right ------------------------------------------------------------------------------------------

def test_reference_matches_the_golden_run():
    """Chained in float64 over coma_tiny's golden run. tests/test_coma_oracle.py holds the fp32 oracle to 1e-4 on all of
    these; the golden arrays are fp32 results of the reference's own fp32 chain, so 2e-5 of the tensor max (2e-6 on the
    stats) is what a float64 restatement of the same mathematics is held to."""
    c = ComaCase("coma_tiny")
    state = tuple(np.asarray(v, np.float64) for v in initial_state(c))
    steps = last_update = 0
    for k in range(c.steps):
        nb, _ = c.batch(k)
        r = C.coma_ref64_step(c, *state, nb, c.epsilon[k])
        for s in COMA_STATS:
            ref = float(c.z["stat_" + s][k])
            assert abs(r.stats[s] - ref) <= 2e-6 * abs(ref) + 1e-7, (k, s, r.stats[s], ref)
        if k == 0:
            assert rel_err(C.flat_of(r.critic_grads[-1]), c.z["step0_critic_grads_last"]) < 2e-5
            assert rel_err(C.flat_of(r.agent_grads), c.z["step0_agent_grads"]) < 2e-5
            assert r.live_steps == sorted(r.live_steps, reverse=True) and len(r.critic_norms) == len(r.live_steps)
        steps += r.stats["critic_steps"]
        tc = state[2]
        if (steps - last_update) / c.target_update_interval >= 1.0:
            tc, last_update = C.flat_of(r.critic_params), steps
        state = (C.flat_of(r.agent_params), C.flat_of(r.critic_params), tc, C.flat_of(r.agent_sq),
                 C.flat_of(r.critic_sq))
        for got, key in zip(state, ("step_agent", "step_critic", "step_target_critic", "step_sq", "step_critic_sq")):
            assert rel_err(got, c.z[key][k]) < 2e-5, (k, key)
    assert steps == int(c.z["critic_training_steps"])


def test_blocks_cover_and_partition():
    c = C.synth_case("r9")
    b = C.coma_blocks(c)
    assert all(k in b["critic"] for k in c.critic_shapes) and all(k in b["agent"] for k in c.agent_shapes)
    cover = np.zeros(c.critic_shapes["fc1.weight"], np.int32)
    for name, (t, idx) in b["critic"].items():
        if t == "fc1.weight" and name != t:
            cover[idx] += 1
    assert (cover == 1).all()
    assert b["critic"]["fc1.weight[agent_id]"][1][1] == slice(c.K - c.n, c.K)
    assert "fc1.weight[last_action]" in b["agent"] and "rnn.bias_hh[z]" in b["agent"]


# ---- the oracle passes the gate at every row ------------------------------------------------------------------------

@pytest.mark.parametrize("row", list(C.SHAPES))
def test_oracle_passes_the_gate(rows, row):
    c, steps = rows(row)
    for k, s in enumerate(steps):
        r, o = s["ref"], s["oracle"]
        orc = C.oracle_quantities(o, s["state"][1])
        rec, bad = C.judge(c, r, orc, orc)
        w = max(((q, b, v["e32"]) for q, d in rec.items() if q != "cdelta" for b, v in d.items()), key=lambda x: x[2])
        wd = max(rec["cdelta"].items(), key=lambda x: x[1]["e32"])
        print("{} step {}: live steps {}, worst e32 {:.3g} at {} {}; update e32 {:.3g} at {}".format(
            row, k, r.live_steps, w[2], w[0], w[1], wd[1]["e32"], wd[0]))
        assert not bad, (row, k, bad)
        assert r.stats["critic_steps"] == len(o.last["critic_grads"]) >= 1
        for q, ref in (("q_vals", r.q_vals), ("targets", r.targets), ("pi", r.pi)):
            assert rel_err(o.last[q], ref) < 1e-5, (row, k, q)
        for st in COMA_STATS:
            assert abs(o.last["stats"][st] - r.stats[st]) <= 1e-4 * abs(r.stats[st]) + 1e-6, (row, k, st)
        assert abs(o.last["stats"]["agent_grad_norm"] - r.agent_norm) <= 1e-5 * r.agent_norm
    d = C.SHAPES[row]
    if d.get("holes"):   # five steps ran, those at the two unwritten slots were skipped
        assert all(s["nb"]["filled"].shape[1] == 6 and s["ref"].live_steps == d["live"] for s in steps), row


# ---- the gate has teeth ----------------------------------------------------------------------------------------------

def _drop_bias_row(g, row_term, c):
    g["fc1.bias"] = (g["fc1.bias"] - row_term).astype(F32)


def _zero_last_column(g, row_term, c):
    g["fc1.weight"][:, -1] = 0.0


def _scale_fc3(g, row_term, c):
    g["fc3.weight"] = (g["fc3.weight"].astype(np.float64) * (1.0 + 1e-4)).astype(F32)


def _flip_id_column(g, row_term, c):
    g["fc1.weight"][:, c.K - c.n] *= F32(-1.0)


# (name, fault, the blocks that hold the corrupted elements, the narrowest of them, whether the old critic band must
# stay silent)
FAULTS = [
    ("row R-1 dropped from fc1.bias's sum", _drop_bias_row, {"fc1.bias"}, "fc1.bias", True),
    ("last column of fc1.weight zeroed", _zero_last_column, {"fc1.weight", "fc1.weight[agent_id]"},
     "fc1.weight[agent_id]", True),
    ("fc3.weight * (1 + 1e-4)", _scale_fc3, {"fc3.weight"}, "fc3.weight", True),
    ("sign of an agent-id column flipped", _flip_id_column, {"fc1.weight", "fc1.weight[agent_id]"},
     "fc1.weight[agent_id]", False),
]


def faulty_oracle(c, s, fault, monkeypatch):
    """The oracle's train() from step state `s` with `fault` planted in the clipped gradient of its last critic step
    (so the step's RMSprop carries it into square_avg and the parameters, as a faulty kernel would)."""
    import oracle.coma_np as M
    n_live, seen, term = len(s["ref"].live_steps), dict(n=0), {}
    back, clip = M.critic_backward, M.clip_grad_norm

    def backward(cp, x, h1, h2, dq):   # row R-1's term of fc1.bias's gradient, which is a plain sum over the rows
        dh2 = (dq[-1:] @ cp["fc3.weight"]) * (h2[-1:] > 0)
        term["row"] = ((dh2 @ cp["fc2.weight"]) * (h1[-1:] > 0))[0].astype(F32)
        return back(cp, x, h1, h2, dq)

    def clip_then_fault(grads, max_norm):
        gn = clip(grads, max_norm)
        if "fc3.weight" in grads:
            seen["n"] += 1
            if seen["n"] == n_live:
                fault(grads, term["row"] * F32(min(max_norm / (gn + 1e-6), 1.0)), c)
        return gn
    monkeypatch.setattr(M, "critic_backward", backward)
    monkeypatch.setattr(M, "clip_grad_norm", clip_then_fault)
    o = C.oracle_at(c, *s["state"])
    o.train(s["nb"], 1000, 0, c.epsilon[0])
    monkeypatch.undo()
    assert seen["n"] == n_live
    return o


@pytest.mark.parametrize("row", ["t1", "r129"])
@pytest.mark.parametrize("what,fault,blocks,narrowest,blind", FAULTS, ids=[f[0] for f in FAULTS])
def test_gate_names_the_faulty_block(rows, row, what, fault, blocks, narrowest, blind, monkeypatch):
    c, steps = rows(row)
    s = steps[0]
    clean = s["oracle"]
    orc = C.oracle_quantities(clean, s["state"][1])
    o = faulty_oracle(c, s, fault, monkeypatch)
    got = C.oracle_quantities(o, s["state"][1])
    assert not np.array_equal(got["cgrad_last"], orc["cgrad_last"])
    rec, bad = C.judge(c, s["ref"], got, orc)
    named_ = {q: {b for qq, b, _, _ in bad if qq == q} for q in C.CRITIC_Q + ("agrad",)}
    # the last step's gradient: exactly the blocks that hold the corrupted elements, the tensor and its column block
    assert named_["cgrad_last"] == blocks, (row, what, bad)
    # square_avg and the update carry it in the same blocks and nowhere else; the agent's gradient not at all
    assert named_["csq"] <= blocks and named_["cdelta"] <= blocks and not named_["agrad"], (row, what, bad)
    # square_avg is g^2: every fault but the sign flip moves it. The update is lr g / (sqrt(v) + eps) with v made of
    # the same g, all but invariant to g's scale, so the 1 + 1e-4 fault legitimately stays silent there; a dropped
    # row, a zeroed column and a flipped sign move it by O(1) of the block
    if fault is not _flip_id_column:
        assert narrowest in named_["csq"], (row, what, bad)
    if fault is not _scale_fc3:
        assert narrowest in named_["cdelta"], (row, what, bad)
    band = np.abs(o.flat("critic").astype(np.float64) - clean.flat("critic")).max()
    worst_ = max(rec["cgrad_last"][b]["err"] for b in blocks)
    print("{} / {}: block err {:.3g}; old critic band sees {:.3g} of {:g}".format(row, what, worst_, band, CRITIC_BAND))
    if blind:
        assert band <= CRITIC_BAND, (row, what, band)   # the gap this gate closes
        assert rel_err(o.last["q_vals"], clean.last["q_vals"]) == 0.0   # the step's Q values cannot see it,
        flat_agent = lambda x: C.flat_of(x.last["agent_grads"])  # noqa: E731  nor the flat gate of the agent's gradient
        assert rel_err(flat_agent(o), flat_agent(clean)) < AGENT_GATE


@pytest.mark.parametrize("row", ["t1", "r129"])
def test_agent_gate_names_what_the_flat_gate_passes(rows, row):
    """The flat rel < 1e-4 gate of the agent's gradient is always fc2.bias's: fc2.weight scaled by 1 + 1e-4 and an
    agent-id column short of 1/1024 of itself pass it; the per-block gate names each."""
    c, steps = rows(row)
    s = steps[0]
    orc = C.oracle_quantities(s["oracle"], s["state"][1])
    av = C.agent_view(c)
    for what, block in (("fc2", "fc2.weight"), ("id", "fc1.weight[agent_id]")):
        g = orc["agrad"].astype(np.float64).copy()
        d = av.unflatten(g)
        if what == "fc2":
            d["fc2.weight"] *= 1.0 + 1e-4
        else:
            d["fc1.weight"][:, c.O + c.A] *= 1.0 - 1.0 / 1024
        rec, bad = C.judge(c, s["ref"], dict(orc, agrad=g), orc)
        assert {(q, b) for q, b, _, _ in bad} <= {("agrad", block), ("agrad", "fc1.weight")}, (row, what, bad)
        assert ("agrad", block) in {(q, b) for q, b, _, _ in bad}, (row, what, bad)
        assert rel_err(g, orc["agrad"]) < AGENT_GATE, (row, what)


# ---- the kink condition ----------------------------------------------------------------------------------------------

def measure(row, seed, monkeypatch):
    """None if the seed's batch does not reach the row's full T; else (kink minimum over both steps and the three
    relus, the oracle's largest pre-activation error, per-step minima)."""
    c = C.synth_case(row, seed)
    d = C.SHAPES[row]
    if int(c.data["filled"].sum(1).max()) != d["T"] + 1 - len(d.get("holes", ())):
        return None
    steps = two_steps(c, monkeypatch)
    if d.get("holes") and any(s["ref"].live_steps != d["live"] for s in steps):
        return None
    kinks = [s["ref"].kink_minima for s in steps]
    return min(min(k.values()) for k in kinks), max(s["pre_err"] for s in steps), kinks


def fallback_rule(pre_err):
    """The margin of a row no seed of which reaches ref64.KINK_EPS: 8 x the oracle's pre-activation error, >= 1e-6."""
    return max(1e-6, 8.0 * pre_err)


@pytest.mark.parametrize("row", list(C.SHAPES))
def test_kink_condition(row, monkeypatch):
    d = C.SHAPES[row]
    assert 0 <= d["seed"] < MAX_SEEDS
    m = measure(row, d["seed"], monkeypatch)
    assert m is not None, "the recorded seed's batch does not have the row's shape"
    kmin, pre_err, kinks = m
    print(row, "seed", d["seed"], "margin", d["margin"], "pre_err", pre_err, kinks)
    if d["margin"] != ref64.KINK_EPS:   # a row that does not reach KINK_EPS: T = 2 and the measured rule
        assert d["T"] == 2 and fallback_rule(pre_err) <= d["margin"] < ref64.KINK_EPS, (row, d["margin"], pre_err)
        assert d["margin"] <= 1.5 * fallback_rule(d["pre_err"])   # and no looser than the rule with its headroom
    assert kmin > 2.0 * d["margin"], (row, kmin, d["margin"], kinks)


if __name__ == "__main__":   # the bounded seed search behind coma_ref64.SHAPES (the rule is in its comment)
    mp = pytest.MonkeyPatch()
    for row_ in C.SHAPES:
        ms = [(seed_, measure(row_, seed_, mp)) for seed_ in range(MAX_SEEDS)]
        ms = [(seed_, m_) for seed_, m_ in ms if m_ is not None]
        reach = [(seed_, m_) for seed_, m_ in ms if m_[0] > 2.0 * ref64.KINK_EPS]
        if reach:
            seed_, m_ = reach[0]
            print("{}: seed {} margin {:g} ({} of {} seeds reach it); minimum {:.3g}".format(
                row_, seed_, ref64.KINK_EPS, len(reach), MAX_SEEDS, m_[0]))
            continue
        ok = [(seed_, m_) for seed_, m_ in ms if m_[0] > 3.0 * fallback_rule(m_[1])]
        print("{}: largest minimum of {} seeds {:.3g};".format(row_, MAX_SEEDS, max(m_[0] for _, m_ in ms)),
              "seed {} pre_err {:.3g} rule {:.3g} minimum {:.3g}".format(
                  ok[0][0], ok[0][1][1], fallback_rule(ok[0][1][1]), ok[0][1][0]) if ok else "no seed")
