"""The float64 autograd reference (tests/ref64.py) and the per-block gradient gate, checked on the CPU.

* ref64 against the numpy oracle (itself pinned to the reference's goldens): every block of the oracle's fp32 raw
  gradient within 1e-5 of ref64 on the block's own max, loss and the five stats to 1e-6 relative. The two share no
  backward code: the oracle's is derived by hand, ref64's is autograd.
* the comparer has teeth: kernel-like faults planted in a correct gradient fail the per-block gate, and the global
  `rel(flat) < 1e-4` gate of the teacher-forced tests does not see them.
* the mixer-kink preconditions (ref64 module docstring) hold for every QMIX shape of tests/test_gpu_grad_blocks.py.
* ref_step's TD(lambda), Huber and weighted tails against the fp32 oracles of tests/lambda_oracle.py and
  tests/per_oracle.py in the same bands; their defaults change no bit; six faults a tail kernel could have fail the
  gate on a named block; every row of tests/test_gpu_tail_blocks.py holds its preconditions with the fp32 oracle
  standing in for the GPU.
"""
from collections import OrderedDict

import numpy as np
import pytest

from oracle.qlearner_np import OracleQLearner, clip_grad_norm
from tests import ref64
from tests.golden_utils import rel_err

STATS = ["loss", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean"]
SYNTH = ["base", "lds", "gemm", "fast32", "stream", "tiles_r21"]
GOLDEN = ["tiny_qmix", "tiny_vdn", "tiny_iql", "tiny_qmix_nola", "tiny_vdn_noid", "tiny_qmix_nodq"]
QMIX_GPU_SHAPES = SYNTH + ["tiles_kq40", "tiles_kq80"]   # every QMIX shape of the GPU table
OLD_GATE = 1e-4   # run_teacher_forced: rel(flat_grads(learner), oracle_grads) < 1e-4, one max over all tensors


@pytest.fixture(scope="module")
def synth():
    cache = {}

    def get(shape):
        if shape not in cache:
            cache[shape] = ref64.synth_case(shape)
        return cache[shape]
    return get


def oracle_raw(case, nb, **over):
    """The fp32 oracle's unclipped gradient at the case's initial state: (oracle, flat gradient, forward dict)."""
    o = OracleQLearner(case.agent_params, case.mixer_params, case.cfg())
    ag, mg, fw = o.gradients(nb, **over)
    g = OrderedDict(list(ag.items()) + list(mg.items()))
    return o, np.concatenate([v.ravel() for v in g.values()]), fw, g


def check_against_oracle(case, over_fn=None):
    nb, _ = case.batch(0)
    o, _, fw0, _ = oracle_raw(case, nb)
    over = over_fn(case, nb, fw0) if over_fn else {}
    o, flat, fw, g = oracle_raw(case, nb, **over)
    r = ref64.ref_step(case, o.flat("params"), o.flat("targets"), nb, **over)
    errs = ref64.block_errors(flat, r.grads, case)
    print(case.name, "worst block", max(errs, key=errs.get), max(errs.values()))
    for k, e in errs.items():
        assert e <= 1e-5, (case.name, k, e)
    st = dict(loss=fw["loss"], grad_norm=clip_grad_norm(OrderedDict(g), case.cfg()["grad_norm_clip"]))
    m, ms = fw["mask"], float(fw["mask"].sum())
    st["td_error_abs"] = float(np.abs(fw["td"] * m).sum()) / ms
    st["q_taken_mean"] = float((fw["q_tot"] * m).sum()) / (ms * case.n)
    st["target_mean"] = float((fw["targets"] * m).sum()) / (ms * case.n)
    for s in STATS:
        assert abs(st[s] - r.stats[s]) <= 1e-6 * abs(r.stats[s]), (case.name, s, st[s], r.stats[s])
    assert np.array_equal(fw["cur_max_actions"], r.cur_max_actions)
    assert rel_err(fw["mask"], r.mask) == 0.0
    return r


@pytest.mark.parametrize("shape", SYNTH)
def test_ref64_matches_oracle_synth(synth, shape):
    r = check_against_oracle(synth(shape))
    nb, _ = synth(shape).batch(0)
    B, Tp = nb["obs"].shape[:2]
    c = synth(shape)
    assert r.hw1.shape == (B * (Tp - 1), c.n * ref64.E) and r.hwf.shape == r.hv.shape == (B * (Tp - 1), ref64.E)
    assert r.pre.shape == (B, Tp, c.n, ref64.H) and r.masked_q.shape == (B, Tp - 1, c.n, c.A)
    # the clipped gradient is g * min(clip / (norm + 1e-6), 1) with the float64 norm
    coef = min(10.0 / (r.norm + 1e-6), 1.0)
    for k, g in r.grads.items():
        assert np.array_equal(r.clipped[k], g * coef)
    assert abs(r.norm - np.sqrt(sum((g ** 2).sum() for g in r.grads.values()))) <= 1e-12 * r.norm


@pytest.mark.parametrize("name", GOLDEN)
def test_ref64_matches_oracle_golden(golden_cases, name):
    check_against_oracle(golden_cases[name])


def forced_decisions(case, nb, fw):
    """Decisions other than the step's own: action 1 (available everywhere, utils/synthetic.py) as the double-Q
    action and the fc1 relu switched the other way wherever |pre-activation| < 0.02."""
    from oracle.qlearner_np import fc1_preacts
    flags = (case.obs_last_action, case.obs_agent_id)
    pre = fc1_preacts(case.agent_params, nb["obs"], nb["actions_onehot"], flags)
    on = (pre > 0) ^ (np.abs(pre) < 0.02)
    assert (on != (pre > 0)).sum() > 10
    cur = np.ones_like(fw["cur_max_actions"])
    assert (cur != fw["cur_max_actions"]).sum() > 10
    return dict(cur_max_override=cur, relu_override=on)


@pytest.mark.parametrize("shape", ["base", "stream"])
def test_overrides_mean_what_the_oracles_mean(synth, shape):
    """cur_max_override / relu_override change ref64's step exactly as they change the oracle's."""
    c = synth(shape)
    nb, _ = c.batch(0)
    free = check_against_oracle(c)
    forced = check_against_oracle(c, forced_decisions)
    assert abs(forced.loss - free.loss) > 1e-3 * free.loss   # the overrides were taken, not ignored


def test_grad_blocks_cover_and_partition(synth, golden_cases):
    for c in (synth("base"), golden_cases["tiny_qmix_nola"], golden_cases["tiny_vdn_noid"], golden_cases["tiny_iql"]):
        blocks = ref64.grad_blocks(c)
        shapes = OrderedDict(list(c.agent_shapes.items()) + list(c.mixer_shapes.items()))
        assert all(k in blocks for k in shapes)
        for k, s in shapes.items():   # the sub-blocks of a tensor tile it exactly once
            subs = [idx for name, (t, idx) in blocks.items() if t == k and name != k]
            if subs:
                cover = np.zeros(s, np.int32)
                for idx in subs:
                    cover[idx] += 1
                assert (cover == 1).all(), (c.name, k)
        assert ("fc1.weight[last_action]" in blocks) == c.obs_last_action
        assert ("fc1.weight[agent_id]" in blocks) == c.obs_agent_id
        assert ("hyper_w_1.bias[agent{}]".format(c.n - 1) in blocks) == (c.mixer == "qmix")
        assert blocks["fc1.weight[obs]"][1][1] == slice(0, c.O)


def test_zero_reference_block_is_measured_on_its_parent(synth):
    c = synth("base")
    ref = OrderedDict((k, np.zeros(s)) for k, s in list(c.agent_shapes.items()) + list(c.mixer_shapes.items()))
    ref["fc1.weight"][:, :c.O] = 2.0   # the last-action and agent-id blocks of the reference are exactly 0
    got = np.concatenate([v.ravel() for v in ref.values()])
    d = c.unflatten(got)
    d["fc1.weight"][3, c.O + 1] = 0.5
    e = ref64.block_errors(got, ref, c)
    assert e["fc1.weight[last_action]"] == 0.25 and e["fc1.weight"] == 0.25 and e["fc1.weight[obs]"] == 0.0


def test_tolerance_rule():
    tol = ref64.tolerances(dict(lucky=7e-9, usual=4e-7, noisy=3e-6))
    assert tol["lucky"] == 16 * 2e-7 and tol["usual"] == 16 * 4e-7 and tol["noisy"] == 1e-5
    assert max(tol.values()) <= OLD_GATE / 10


# Faults a kernel could have, planted in the oracle's (correct) fp32 gradient of the base case. Each is
# (name, blind, mutate(named views, case, T, ref)); blind: the old global gate is asserted not to see it.
# A whole agent-id column zeroed and the z rows short of a whole timestep are errors of 2.9e-2 and 4.1e-4 of the
# global max at this shape (an agent-id column is 1.7e-2 of it at cfg2's), which the global gate does see, so nothing
# is asserted of it there; their attenuated forms (the column off by 1/1024, one row of a 256-row slab reduction
# missing from one timestep) it does not see, and the block gate catches all of them.
def _v0_small_element(ref):
    """The largest element of V.0.weight under half the old gate's resolution (5e-5 of the global max)."""
    gmax = max(np.abs(v).max() for v in ref.values())
    a = np.abs(ref["V.0.weight"])
    return np.unravel_index(np.where(a < 0.5 * OLD_GATE * gmax, a, 0.0).argmax(), a.shape)


def _mut_hw1b(d, c, T, ref):
    d["hyper_w_1.bias"][ref64.E:2 * ref64.E] *= 1.0 - 1.0 / 256


def _mut_id_col(d, c, T, ref):
    d["fc1.weight"][:, c.O + c.A + 1] = 0.0


def _mut_id_col_1024(d, c, T, ref):
    d["fc1.weight"][:, c.O + c.A + 1] *= 1.0 - 1.0 / 1024


def _mut_bhh_z(d, c, T, ref):
    d["rnn.bias_hh"][ref64.H:2 * ref64.H] *= 1.0 - 1.0 / T


def _mut_bhh_z_row(d, c, T, ref):
    d["rnn.bias_hh"][ref64.H:2 * ref64.H] *= 1.0 - 1.0 / (256 * T)


def _mut_v0(d, c, T, ref):
    d["V.0.weight"][_v0_small_element(ref)] = 0.0


MUTANTS = [
    ("hyper_w_1.bias agent block * (1 - 1/256)", True, _mut_hw1b, "hyper_w_1.bias[agent1]"),
    ("fc1.weight agent-id column zeroed", False, _mut_id_col, "fc1.weight[agent_id]"),
    ("fc1.weight agent-id column * (1 - 1/1024)", True, _mut_id_col_1024, "fc1.weight[agent_id]"),
    ("rnn.bias_hh z rows * (1 - 1/T)", False, _mut_bhh_z, "rnn.bias_hh[z]"),
    ("rnn.bias_hh z rows * (1 - 1/(256 T))", True, _mut_bhh_z_row, "rnn.bias_hh[z]"),
    ("V.0.weight element zeroed", True, _mut_v0, "V.0.weight"),
]


@pytest.fixture(scope="module")
def base_gradients(synth):
    c = synth("base")
    nb, _ = c.batch(0)
    o, flat, fw, _ = oracle_raw(c, nb)
    r = ref64.ref_step(c, o.flat("params"), o.flat("targets"), nb)
    e32 = ref64.block_errors(flat, r.grads, c)
    return c, nb["obs"].shape[1] - 1, flat, r, e32


def test_unmodified_gradient_passes_the_gate(base_gradients):
    c, T, flat, r, e32 = base_gradients
    assert not ref64.failures(e32, ref64.tolerances(e32))
    assert max(e32.values()) < 1e-6   # fp32 noise: the tolerances below are 16 * that, not the 1e-5 cap


@pytest.mark.parametrize("what,blind,mutate,block", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_gate_catches_mutant(base_gradients, what, blind, mutate, block):
    c, T, flat, r, e32 = base_gradients
    got = flat.astype(np.float64).copy()
    mutate(c.unflatten(got), c, T, r.grads)
    assert not np.array_equal(got, flat.astype(np.float64))
    bad = ref64.failures(ref64.block_errors(got, r.grads, c), ref64.tolerances(e32))
    assert block in bad, (what, bad)
    old = rel_err(got, np.concatenate([g.ravel() for g in r.grads.values()]))
    print(what, "per-block", bad[block], "old global rel", old)
    if blind:
        assert old < OLD_GATE, (what, old)   # the gap this gate closes


@pytest.mark.parametrize("shape", QMIX_GPU_SHAPES)
def test_kink_preconditions(synth, shape):
    c = synth(shape)
    nb, _ = c.batch(0)
    o = OracleQLearner(c.agent_params, c.mixer_params, c.cfg())
    r = ref64.ref_step(c, o.flat("params"), o.flat("targets"), nb)
    print(shape, ref64.kink_minima(r))
    ref64.assert_clear_of_kinks(r, c.name)
    assert (r.mask > 0).sum() < r.mask.size   # ragged: dead rows exist and are left out of the minima


# ------------------------------------------------------------------ the TD(lambda), Huber and weighted tails of ref_step
TAIL_CASES = [("base", "qmix"), ("base", "vdn"), ("base", "none"), ("fast32", "qmix"), ("stream", "qmix")]
TAIL_KINDS = ["lam", "huber", "weights", "all"]
LAM = 0.8


@pytest.fixture(scope="module")
def lambda_cases():
    cache = {}

    def get(shape, mixer):
        if (shape, mixer) not in cache:
            cache[shape, mixer] = ref64.lambda_case(shape, mixer)
        return cache[shape, mixer]
    return get


def median_delta(case, nb, lam):
    """Huber's delta as tests/test_gpu_tail_blocks.py chooses it: the median |td mask| of the live transitions at the
    case's initial weights, rounded to a multiple of 1/16."""
    o = OracleQLearner(case.agent_params, case.mixer_params, case.cfg())
    r = ref64.ref_step(case, o.flat("params"), o.flat("targets"), nb, td_lambda=lam)
    return round(float(np.median(np.abs(r.mtd)[r.mask > 0])) * 16) / 16


def skewed(B):
    """Weights as the sampler normalises them: the largest is 1, the smallest 1/4."""
    return np.linspace(0.25, 1.0, B).astype(np.float32)


def tail_settings(case, nb, kind):
    lam = LAM if kind in ("lam", "all") else None
    delta = median_delta(case, nb, lam) if kind in ("huber", "all") else 0.0
    w = skewed(nb["obs"].shape[0]) if kind in ("weights", "all") else None
    return lam, delta, w


def per_oracle_raw(case, nb, lam, delta, w):
    """tests/per_oracle.PEROracleQLearner's unclipped fp32 gradient under the three tails: (oracle, flat, fw, named)."""
    from tests.per_oracle import PEROracleQLearner
    o = PEROracleQLearner(case.agent_params, case.mixer_params,
                          dict(case.cfg(), td_lambda=lam or 0.0, huber_delta=delta))
    o.weights = w
    ag, mg, fw = o.gradients(nb)
    g = OrderedDict(list(ag.items()) + list(mg.items()))
    return o, np.concatenate([v.ravel() for v in g.values()]), fw, g


@pytest.mark.parametrize("kind", TAIL_KINDS)
@pytest.mark.parametrize("shape,mixer", TAIL_CASES, ids=["_".join(c) for c in TAIL_CASES])
def test_ref64_tails_match_the_fp32_oracle(lambda_cases, shape, mixer, kind):
    """ref_step's three tails against the fp32 oracles they share no code with (tests/lambda_oracle.py's recurrence,
    tests/per_oracle.py's Huber and weights, hand-derived dy), in check_against_oracle's bands."""
    case = lambda_cases(shape, mixer)
    nb, _ = case.batch(0)
    lam, delta, w = tail_settings(case, nb, kind)
    o, flat, fw, g = per_oracle_raw(case, nb, lam, delta, w)
    r = ref64.ref_step(case, o.flat("params"), o.flat("targets"), nb, td_lambda=lam, huber_delta=delta, weights=w)
    errs = ref64.block_errors(flat, r.grads, case)
    print(case.name, kind, "delta", delta, "worst block", max(errs, key=errs.get), max(errs.values()))
    for k, e in errs.items():
        assert e <= 1e-5, (case.name, kind, k, e)
    m, ms = fw["mask"], float(fw["mask"].sum())
    st = dict(loss=fw["loss"], grad_norm=clip_grad_norm(OrderedDict(g), case.cfg()["grad_norm_clip"]),
              td_error_abs=float(np.abs(fw["td"] * m).sum()) / ms,
              q_taken_mean=float((fw["q_tot"] * m).sum()) / (ms * case.n),
              target_mean=float((fw["targets"] * m).sum()) / (ms * case.n))
    for s in STATS:
        assert abs(st[s] - r.stats[s]) <= 1e-6 * abs(r.stats[s]), (case.name, kind, s, st[s], r.stats[s])
    live = r.mask > 0
    k = 1 if mixer != "none" else case.n
    assert r.targets.shape == r.y_next.shape == r.mtd.shape == r.mask.shape == live.shape[:2] + (k,)
    assert r.abs_mtd.shape == live.shape[:2] + (1,)
    assert np.array_equal(r.abs_mtd, np.abs(r.mtd).sum(2, keepdims=True))
    assert np.abs(fw["targets"] - r.targets)[live].max() <= 1e-6 * np.abs(r.targets[live]).max()
    if lam:   # the case has what the lambda rows need: a single transition, and a bootstrap that is not zero
        assert int(nb["filled"].sum(1).min()) == 2 and r.bootstrap.shape == (live.shape[0], k)
        assert np.abs(r.bootstrap).max() > 1e-3
    else:
        assert r.bootstrap is None
    if delta:
        below = float((np.abs(r.mtd)[live] <= delta).mean())
        assert 0.4 <= below <= 0.6, (case.name, kind, below)   # delta is the median: both regimes carry the loss
    # the tail was taken, not ignored
    plain = ref64.ref_step(case, o.flat("params"), o.flat("targets"), nb)
    assert rel_err(r.clipped_flat, plain.clipped_flat) > 1e-2


@pytest.mark.parametrize("shape,mixer", [("base", "qmix"), ("base", "none")])
def test_tail_defaults_are_bitwise(synth, shape, mixer):
    """The new keyword arguments at their defaults, and weights == 1, change no bit of the step."""
    c = ref64.synth_case(shape, mixer) if mixer != "qmix" else synth(shape)
    nb, _ = c.batch(0)
    flat = ref64.flat_of(c)
    a = ref64.ref_step(c, flat, flat, nb)
    b = ref64.ref_step(c, flat, flat, nb, td_lambda=None, huber_delta=0.0, weights=None)
    ones = ref64.ref_step(c, flat, flat, nb, weights=np.ones(nb["obs"].shape[0], np.float32))
    for other in (b, ones):
        assert other.loss == a.loss and other.stats == a.stats and other.norm == a.norm
        for k in a.grads:
            assert np.array_equal(other.grads[k], a.grads[k]), k
        assert np.array_equal(other.clipped_flat, a.clipped_flat)


def _shifted_returns(rew, term, mask, y, gamma, lam):
    """lambda_returns reading y'[t + 1] where y'[t] belongs (the last step reads its own)."""
    import torch as th
    L = y.shape[1]
    return _LAMBDA_RETURNS(rew, term, mask, th.cat([y[:, 1:], y[:, L - 1:]], 1), gamma, lam)[0], \
        y[:, L - 1] * (1.0 - term.sum(1))


def _no_bootstrap_returns(rew, term, mask, y, gamma, lam):
    """lambda_returns started from 0 where y'[L-1] (1 - sum term) belongs. The recurrence is linear in its start:
    step t carries (lambda gamma)^(L - t) of it."""
    import torch as th
    full, boot = _LAMBDA_RETURNS(rew, term, mask, y, gamma, lam)
    L = y.shape[1]
    decay = th.tensor([(lam * gamma) ** (L - t) for t in range(L)], dtype=y.dtype).reshape(1, L, 1)
    return full - decay * boot.unsqueeze(1), boot


def _unmasked_huber(td, m, delta):
    """td_loss with Huber on td where td * m belongs: the padded transitions reach the loss and dy."""
    import torch as th
    return _TD_LOSS(td, th.ones_like(m), delta)[0], td * m


_LAMBDA_RETURNS, _TD_LOSS = ref64.lambda_returns, ref64.td_loss

# (name, blind, which reference function is replaced, by what, keyword arguments of the mutant's ref_step that differ
# from the reference's, the block named). The reference runs lambda = 0.8, Huber at the median and skewed weights
# together. blind: the old gate, rel(flat) < 1e-4, is asserted not to see the mutant. None of these six is small on
# the global max once its tail is really on (the figures are printed), so none is blind in that sense; the gap they
# stood in is one of coverage. Off the fast16 shapes the old tests ran PER at beta = 0 only, where W == 1: there the
# two PER mutants leave every bit of the gradient as it is (asserted below), and Huber met a reference on fast16 alone.
TAIL_MUTANTS = [
    ("w on the loss, not on dy", False, None, None, dict(weights=None), "V.0.weight"),
    ("w[b] of the neighbouring episode", False, None, None, dict(weights="roll"), "hyper_w_1.bias[agent1]"),
    ("lambda recurrence reads y'[t+1]", False, "lambda_returns", _shifted_returns, {}, "fc1.weight[agent_id]"),
    ("bootstrap term dropped", False, "lambda_returns", _no_bootstrap_returns, {}, "rnn.bias_hh[z]"),
    ("Huber clamps at 2 delta", False, None, None, dict(huber_delta="double"), "hyper_w_final.bias"),
    ("Huber's dy without the mask", False, "td_loss", _unmasked_huber, {}, "fc2.bias"),
]


@pytest.fixture(scope="module")
def tail_gradients(lambda_cases):
    c = lambda_cases("base", "qmix")
    nb, _ = c.batch(0)
    lam, delta, w = tail_settings(c, nb, "all")
    o, flat, fw, _ = per_oracle_raw(c, nb, lam, delta, w)
    r = ref64.ref_step(c, o.flat("params"), o.flat("targets"), nb, td_lambda=lam, huber_delta=delta, weights=w)
    return c, nb, o, dict(td_lambda=lam, huber_delta=delta, weights=w), r, ref64.block_errors(flat, r.grads, c)


def test_unmodified_tail_gradient_passes_the_gate(tail_gradients):
    c, nb, o, kw, r, e32 = tail_gradients
    assert not ref64.failures(e32, ref64.tolerances(e32))
    assert max(e32.values()) < 1e-6


@pytest.mark.parametrize("what,blind,target,repl,diff,block", TAIL_MUTANTS, ids=[m[0] for m in TAIL_MUTANTS])
def test_gate_catches_tail_mutant(tail_gradients, monkeypatch, what, blind, target, repl, diff, block):
    c, nb, o, kw, r, e32 = tail_gradients
    kw2 = dict(kw)
    for k, v in diff.items():
        kw2[k] = np.roll(kw[k], 1) if v == "roll" else 2.0 * kw[k] if v == "double" else v
    if target:
        monkeypatch.setattr(ref64, target, repl)
    mut = ref64.ref_step(c, o.flat("params"), o.flat("targets"), nb, **kw2)
    monkeypatch.undo()
    got = np.concatenate([g.ravel() for g in mut.grads.values()])
    bad = ref64.failures(ref64.block_errors(got, r.grads, c), ref64.tolerances(e32))
    assert block in bad, (what, bad)
    old = rel_err(got, np.concatenate([g.ravel() for g in r.grads.values()]))
    print(what, "per-block", bad[block], "blocks over", len(bad), "of", len(e32), "old global rel", old)
    assert (old < OLD_GATE) == blind, (what, old)
    if "weights" in diff:   # what the old tests gave every kernel but fast16: W == 1, and the mutant is the reference
        one = dict(kw, weights=np.ones_like(kw["weights"]))
        a = ref64.ref_step(c, o.flat("params"), o.flat("targets"), nb, **one)
        b = ref64.ref_step(c, o.flat("params"), o.flat("targets"), nb, **dict(one, weights=None))
        assert rel_err(b.clipped_flat, a.clipped_flat) == 0.0 < OLD_GATE


def test_tail_rows_hold_their_preconditions():
    """Every row of tests/test_gpu_tail_blocks.py on the CPU, the fp32 oracle standing in for the GPU over both steps:
    the draw of a PER row has its two weights and the episodes a lambda row needs; delta is the step-0 median; both
    Huber regimes are live; the bootstrap is not zero; the QMIX rows keep clear of the mixer's kinks."""
    from tests import reward_norm_ref as RN
    from tests import test_gpu_tail_blocks as TB
    from tests.per_oracle import PEROracleQLearner
    from tests.test_gpu_epymarl_keys import with_rewards
    from tests.test_gpu_per import numpy_batch
    assert len(TB.ROWS) == 28 and set(TB.HUBER_DELTA) == {r for r, v in TB.ROWS.items() if TB.TAILS[v[3]][2]}
    cases = {}
    for row, (shape, mixer, switches, tail, mix) in TB.ROWS.items():
        lam, per, hub, rs, want = TB.TAILS[tail]
        case = cases.setdefault(TB.case_key(row), TB.tail_case(row))
        assert case.n_episodes == case.B and case.T == ref64.SHAPES[shape]["T"]
        delta = TB.HUBER_DELTA[row] if hub else 0.0
        if hub:
            assert delta == median_delta(case, case.batch(0)[0], LAM if lam else None), row
            assert np.float32(delta) == delta
        o = PEROracleQLearner(case.agent_params, case.mixer_params,
                              dict(case.cfg(), td_lambda=TB.LAM if lam else 0.0, huber_delta=delta))
        need = TB.lambda_needs(case) if lam else ()
        state = RN.INIT
        for k in range(2):
            w = None
            if per:
                prio, u, ids, w = TB.per_draw(case, k, need)
                assert prio.max() >= 0.5 * prio.sum() and len(set(w.tolist())) >= 2 and set(need) <= set(ids)
                assert np.array_equal(u * 256, np.round(u * 256))
                nb = numpy_batch(case, ids, int(case.data["filled"].sum(1).max()))
            else:
                nb, _ = case.batch(k)
            if rs:
                state, r8 = RN.standardise(state, nb["reward"][:, :-1])
                nb = with_rewards(nb, r8.astype(np.float32))
            o.weights = w
            ref = ref64.ref_step(case, o.flat("params"), o.flat("targets"), nb, weights=w,
                                 td_lambda=TB.LAM if lam else None, huber_delta=delta)
            if mixer == "qmix":
                ref64.assert_clear_of_kinks(ref, "{} step {}".format(row, k))
            TB.preconditions(ref, nb, lam, delta, "{} step {}".format(row, k))
            o.train(nb, 1000 * k, case.episodes[k])
