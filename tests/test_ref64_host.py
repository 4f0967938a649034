"""The float64 autograd reference (tests/ref64.py) and the per-block gradient gate, checked on the CPU.

* ref64 against the numpy oracle (itself pinned to the reference's goldens): every block of the oracle's fp32 raw
  gradient within 1e-5 of ref64 on the block's own max, loss and the five stats to 1e-6 relative. The two share no
  backward code: the oracle's is derived by hand, ref64's is autograd.
* the comparer has teeth: kernel-like faults planted in a correct gradient fail the per-block gate, and the global
  `rel(flat) < 1e-4` gate of the teacher-forced tests does not see them.
* the mixer-kink preconditions (ref64 module docstring) hold for every QMIX shape of tests/test_gpu_grad_blocks.py.
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
