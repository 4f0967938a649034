"""GPU parity of the HIP learner against the golden vectors of the reference learner (and the oracle).

Runs through the product path: QLearner.train -> libmq_learner.so (C ABI) on an MI355X.

Two kinds of check (DESIGN.md "Parity"):
* free-running trajectory vs the reference's golden run. north_star asks for the loss trajectory to 1e-4 relative.
  Two discrete decisions sit on fp32 rounding: the double-Q target gathers the TARGET net's Q at the ONLINE net's
  argmax (q_learner.py:75-76), and the fc1 relu (rnn_agent.py:28) switches at 0. A near-tie that rounds the other
  way changes a target by O(1) or a gradient row, and RMSprop's per-parameter normalisation carries it into the
  next step's parameters at O(lr): from the first such event on, the GPU and the reference follow different,
  equally valid trajectories (the oracle and the reference themselves part after 12 cfg2 steps). So at every step
  the oracle is run from the GPU's own state and every decision is classified: a near-tie (top-2 margin
  <= MARGIN_EPS * max(1, |Q|), or |fc1 pre-activation| <= RELU_EPS) is exempt, and a flip (the GPU deciding a
  near-tie the other way, either from the oracle reset to the GPU's state or from a free-running shadow oracle at its
  own state) is counted. The loss must hold 1e-4 against the reference for HOLD_STEPS steps, or up to
  a step at or after the first counted flip. The per-step errors and counts are written to $MQ_PARITY_DIR.
* teacher-forced steps (the per-step parity proper): the GPU learner and the numpy oracle (itself pinned to the
  reference at ~1e-7) start every step from the SAME parameters / optimiser state; the GPU's double-Q argmax
  must equal the oracle's wherever the top-2 margin exceeds MARGIN_EPS and its fc1 relu decisions wherever
  |pre-activation| > RELU_EPS; the oracle then follows the GPU's decisions on the near-ties, and loss / stats
  must agree to 1e-5 relative, gradients and updated parameters to 1e-4 / 1e-5 of the tensor max. The exempted
  near-ties and the flips among them are counted per step and written out.
"""
import json
import os

import numpy as np
import pytest
import torch as th

from tests.golden_utils import Case
from tests.gpu_helpers import set_switch
from tests.ref64 import MARGIN_EPS, RELU_EPS, near_ties

pytestmark = pytest.mark.gpu

STATS = ["loss", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean"]
HOLD_STEPS = 12     # the oracle itself holds the reference's cfg2 loss trajectory to 1e-4 for 12 steps
LOSS_RTOL = 1e-4    # north_star: "loss trajectory to 1e-4 rel on a fixed seed"


def write_record(kind, name, rec):
    out = os.environ.get("MQ_PARITY_DIR")
    if not out:
        return
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "parity_{}_{}.json".format(kind, name)), "w") as f:
        json.dump(rec, f, indent=1)


def per_tensor_err(case, got_flat, ref_flat):
    """{tensor: max|got - ref| / max|ref|}, each tensor on its own max (recorded, not asserted: at cfg2 / cfg3 sizes
    some of the 1e5 hypernet pre-activations sit on the mixer's abs / relu kinks, so a tight per-tensor gate would be
    flaky by construction; tests/test_gpu_grad_blocks.py gates per block on shapes that keep clear of them)."""
    from tests.gpu_helpers import rel
    got, ref = case.unflatten(np.asarray(got_flat)), case.unflatten(np.asarray(ref_flat))
    return {k: rel(got[k], ref[k]) for k in ref}


def classify_decisions(learner, o, nb, fw):
    """Compare the GPU's double-Q argmax and fc1 relu decisions with the oracle's at the same state.
    Returns (record, dq_flip_mask_ok, relu_flip_ok): the counts of decisions, near-ties and flips."""
    from oracle.qlearner_np import fc1_preacts
    if o.cfg.get("double_q", True):   # the online net's masked argmax (q_learner.py:71-76)
        q = fw["mac_out"].copy()
        q[nb["avail_actions"] == 0] = -9999999.0
        q = q[:, 1:]
    else:                             # target_mac_out.max(dim=3) (q_learner.py:77-78), masked at :68
        q = fw["target_mac_out"]
    # live transitions (q_learner.py:39-44 mask): padded slots (every action masked) are ties by construction but
    # never reach the loss, so they are counted separately
    tie, live = near_ties(q, fw["mask"])
    got = learner.last_cur_max_actions().cpu().numpy()
    dq_flip = got != fw["cur_max_actions"]
    on_gpu = learner.last_intermediate(3).cpu().numpy() > 0
    pre = fc1_preacts(o.p, nb["obs"], nb["actions_onehot"], o.input_flags)
    relu_tie = np.abs(pre) <= RELU_EPS
    relu_flip = on_gpu != (pre > 0)
    rec = dict(dq_decisions=int(live.sum()), dq_ties=int((tie & live).sum()), dq_masked_slots=int((~live).sum()),
               dq_flips=int(dq_flip.sum()), dq_flips_live=int((dq_flip & live).sum()),
               dq_flips_outside_ties=int((dq_flip & ~tie).sum()), relu_decisions=int(relu_tie.size),
               relu_ties=int(relu_tie.sum()), relu_flips=int(relu_flip.sum()),
               relu_flips_outside_ties=int((relu_flip & ~relu_tie).sum()),
               max_flip_pre=float(np.abs(pre[relu_flip]).max()) if relu_flip.any() else 0.0)
    return rec, got, on_gpu


def oracle_from_learner(o, case, learner):
    """Put the GPU learner's params / targets / RMSprop state into the oracle (for decisions at the GPU's state)."""
    from tests.gpu_helpers import flat_params, flat_targets
    for which, flat in (("p", flat_params(learner)), ("t", flat_targets(learner)),
                        ("sq", learner._sq.detach().cpu().numpy().copy())):
        d = case.unflatten(flat)
        for k, v in d.items():
            if which == "sq":
                o.sq[k] = v.astype(np.float32).copy()
            elif k in o.p or k in o.tp:
                (o.p if which == "p" else o.tp)[k] = v.astype(np.float32).copy()
            else:
                (o.mp if which == "p" else o.tmp)[k] = v.astype(np.float32).copy()


@pytest.fixture(scope="module")
def cases():
    return {}


def get_case(cases, name):
    if name not in cases:
        cases[name] = Case(name)
    return cases[name]


def run_case(case, check_full, plan=None):
    """Free run of the GPU learner against the reference's golden run (module doc). Beside it run two oracles: `o`
    is reset to the GPU's state every step and classifies the GPU's decisions (near-ties, flips); the shadow `o2`
    runs free from the same start but takes the GPU's decisions (allowed only where they are near-ties at its own
    state), so GPU vs shadow measures the arithmetic alone, with the near-tie branch choices factored out."""
    from oracle.qlearner_np import OracleQLearner
    from tests.gpu_helpers import build, flat_grads, flat_params, flat_targets, rel
    args, buf, mac, learner, logger = build(case)
    o = OracleQLearner(case.agent_params, case.mixer_params, case.cfg())
    o2 = OracleQLearner(case.agent_params, case.mixer_params, case.cfg())
    np.random.seed(case.sampler_seed)
    rec = []
    for k in range(case.steps):
        batch = buf.sample(case.B)
        assert np.array_equal(batch.ep_ids_np, case.z["ids"][k]), "sampler ids diverged from the reference"
        max_t = batch.max_t_filled()
        batch = batch[:, :max_t]
        nb, _ = case.batch(k)
        oracle_from_learner(o, case, learner)   # the oracle's decisions at the GPU's own state
        fw = o.forward(nb)
        fw2 = o2.forward(nb)
        learner.train(batch, 1000 * k, case.episodes[k])
        if plan is not None and k == 0:
            got_plan = learner.last_plan()
            for key, v in plan.items():
                assert got_plan[key] == v, (case.name, key, got_plan)
        st = learner.last_stats()
        r, got, on_gpu = classify_decisions(learner, o, nb, fw)
        r2, _, _ = classify_decisions(learner, o2, nb, fw2)
        st2 = o2.train(nb, 1000 * k, case.episodes[k], cur_max_override=got, relu_override=on_gpu)
        r["step"] = k
        r["loss"] = st["loss"]
        r["ref_loss"] = float(case.z["stat_loss"][k])
        r["shadow_loss"] = st2["loss"]
        r["shadow_flips_outside_ties"] = r2["dq_flips_outside_ties"] + r2["relu_flips_outside_ties"]
        # near-ties the GPU decided against the free-running oracle's own decision at the oracle's own state: from
        # such a step on, the GPU (and the shadow, which took its choices) leave the trajectory the oracle and the
        # reference share, even where the oracle reset to the GPU's state agrees with the GPU
        r["shadow_flips"] = r2["dq_flips"] + r2["relu_flips"]
        for s_ in STATS:
            ref = float(case.z["stat_" + s_][k])
            assert np.isfinite(st[s_]), (case.name, k, s_)
            r["rel_err_" + s_] = abs(st[s_] - ref) / max(abs(ref), 1e-12)
            r["shadow_rel_err_" + s_] = abs(st[s_] - st2[s_]) / max(abs(st2[s_]), 1e-12)
        # against the shadow oracle's gradient (its own free-running state, the GPU's decisions)
        r["grad_err_per_tensor"] = per_tensor_err(
            case, flat_grads(learner), np.concatenate([v.ravel() for v in o2.last["grads"].values()]))
        if "cur_max_actions" in case.z and k < case.z["cur_max_actions"].shape[0]:
            Tk = got.shape[1]   # ragged fixtures pad the time axis
            ref = case.z["cur_max_actions"][k][:, :Tk].astype(np.int64)
            # the decision's own Q: the online net under double-Q, else the target net (q_learner.py:71-78)
            mo = learner.last_intermediate(0 if case.double_q else 1).cpu().numpy()[:, 1:max_t]
            mo = np.where(nb["avail_actions"][:, 1:] == 0, np.float32(-9999999.0), mo)
            clear = case.z["margin"][k][:, :Tk] > MARGIN_EPS * np.maximum(1.0, np.abs(mo.max(axis=3)))
            r["ref_dq_mismatch_clear"] = int((got != ref)[clear].sum())
            r["ref_dq_mismatch_ties"] = int((got != ref)[~clear].sum())
        rec.append(r)
        if check_full and k == 0:
            mo = learner.last_intermediate(0).cpu().numpy()
            assert rel(mo, case.z["step0_mac_out"]) < 2e-5
            tmo = learner.last_intermediate(1).cpu().numpy()[:, 1:]
            avail = case.data["avail_actions"][case.z["ids"][0]][:, 1:max_t]
            tmo = np.where(avail == 0, np.float32(-9999999.0), tmo)
            assert rel(tmo, case.z["step0_target_mac_out"]) < 2e-5
            assert rel(flat_grads(learner), case.z["step0_grads_clipped"]) < 1e-4
        if "step_params" in case.z:
            assert rel(flat_params(learner), case.z["step_params"][k]) < 1e-4, (case.name, k)
    write_record("freerun", case.name, rec)
    # every decision the GPU takes differently from the oracle at its own state is a near-tie
    for r in rec:
        assert r["dq_flips_outside_ties"] == 0 and r["relu_flips_outside_ties"] == 0, (case.name, r)
    flip_steps = [r["step"] for r in rec if r["dq_flips"] + r["relu_flips"] + r["shadow_flips"] > 0]
    first_flip = flip_steps[0] if flip_steps else case.steps
    # against the reference's recorded actions: exact on clear margins until a flip can have moved the parameters
    for r in rec[:first_flip + 1]:
        assert r.get("ref_dq_mismatch_clear", 0) == 0, (case.name, r)
    # the loss trajectory holds LOSS_RTOL against the reference for HOLD_STEPS steps, or up to a counted flip
    errs = [r["rel_err_loss"] for r in rec]
    hold = next((k for k, e in enumerate(errs) if e > LOSS_RTOL), len(errs))
    for s_ in STATS:
        ref0 = abs(float(case.z["stat_" + s_][0]))
        assert rec[0]["rel_err_" + s_] <= LOSS_RTOL + 1e-6 / max(ref0, 1e-6), (case.name, s_, rec[0])
    if hold < min(HOLD_STEPS, case.steps):
        assert first_flip <= hold, (case.name, "loss left 1e-4 at step {} before any counted flip".format(hold), errs)
    # with the GPU's near-tie choices factored out (shadow oracle), the loss holds LOSS_RTOL as long as the oracle
    # holds the reference's own trajectory (HOLD_STEPS) and the shadow's decisions stay clear of forced flips
    for r in rec[:HOLD_STEPS]:
        if r["shadow_flips_outside_ties"]:
            break
        assert r["shadow_rel_err_loss"] <= LOSS_RTOL, (case.name, r["step"], [x["shadow_rel_err_loss"] for x in rec])
    for k in range(hold, case.steps):   # a different valid trajectory after a near-tie flip: sanity bound only
        ref = case.z["stat_loss"][k]
        assert 0.5 * ref <= rec[k]["loss"] <= 2.0 * ref, (case.name, k, errs)
    if "targets_final" in case.z:
        # RMSprop's per-element 1/(sqrt(v)+eps) turns fp32 noise in a cancelling (near-zero) gradient element into
        # an O(lr) step difference, so parameters agree per element only to an O(lr) band per step taken
        # (the loss above, a global statistic, is the tight check)
        d = np.abs(flat_targets(learner).astype(np.float64) - case.z["targets_final"])
        assert d.max() <= 20 * 5e-4 * case.steps, (case.name, float(d.max()))
    if "sqavg_final" in case.z:
        assert rel(learner._sq.cpu().numpy(), case.z["sqavg_final"]) < 1e-4
    return learner


@pytest.mark.parametrize("name", ["tiny_qmix_full", "tiny_qmix", "tiny_vdn", "tiny_iql", "tiny_qmix_nodq",
                                  "tiny_qmix_nola", "tiny_vdn_noid", "tiny_qmix_bare"])
def test_tiny_full(cases, name):
    run_case(get_case(cases, name), check_full=True)


@pytest.mark.parametrize("name", ["cfg2_qmix", "cfg2_vdn", "cfg2_qmix_ragged", "cfg2_iql", "cfg3_vdn", "cfg3_qmix",
                                  "cfg4_qmix", "cfg2_qmix_nodq", "cfg1_qmix", "cfg1_vdn"])
def test_cfg2_trajectory(cases, name):
    run_case(get_case(cases, name), check_full=False)


# Kernel variants past the fused kernels' limits, each pinned to a reference golden run (tests/golden/make_golden.py)
# and to the oracle teacher-forced: R = B * n rows selects gru_fwd_kernel<RW> (RW = 2 / 4 / 8 rows per workgroup)
# and gru_bwd_kernel<2> (R > 512); B > 256 sends the episode ids through the device vector; cfg3_vdn_b128 is BASELINE
# configs[2] itself (the bench's cfg3 path).
WIDE_PLANS = {
    # past the one-row fused kernels (R > 512): the row-tile MFMA forward / BPTT (gru_tiles.hpp)
    "rw2_qmix": dict(rows=576, tiles=1, fused_fwd=0, fused_bwd=0, inline_ids=1, hyper="ws"),
    "rw4_vdn": dict(rows=1280, tiles=1, fused_fwd=0, fused_bwd=0, inline_ids=1, mix="fast16"),
    "wide_qmix": dict(rows=2400, tiles=1, fused_fwd=0, fused_bwd=0, inline_ids=0),
    "cfg3_vdn_b128": dict(rows=3456, tiles=1, fused_fwd=0, fused_bwd=0, inline_ids=1, mix="stream"),
    "cfg2_iql": dict(rows=256, fused_fwd=2, fused_bwd=1, hyper="none"),
    # configs[3]'s per-GPU shard: R = 320 rows, past the CU count, still on the fused BPTT (a second wave of rows)
    "cfg4_qmix": dict(rows=320, fused_fwd=1, fused_bwd=1, hyper="ws"),
}


@pytest.mark.parametrize("name", sorted(WIDE_PLANS))
def test_wide_batch_paths_vs_reference(cases, name):
    run_case(get_case(cases, name), check_full=False, plan=WIDE_PLANS[name])


# The row-batched GEMM + recurrence path the row tiles replaced (MQ_PLAN row_tiles=0): gru_fwd_kernel<RW>
# (RW = 2 / 4 / 8 rows per workgroup) and gru_bwd_kernel<2>, still the path for shapes past the tiles' limits, pinned to the same
# reference goldens.
RW_PLANS = {
    "rw2_qmix": dict(rows=576, tiles=0, fused_fwd=0, rw_fwd=2, fused_bwd=0, rw_bwd=2, inline_ids=1, hyper="ws"),
    "rw4_vdn": dict(rows=1280, tiles=0, fused_fwd=0, rw_fwd=4, fused_bwd=0, rw_bwd=2, inline_ids=1),
    "wide_qmix": dict(rows=2400, tiles=0, fused_fwd=0, rw_fwd=8, fused_bwd=0, rw_bwd=2, inline_ids=0),
}


@pytest.mark.parametrize("name", sorted(RW_PLANS))
def test_row_batched_paths_vs_reference(cases, name, monkeypatch):
    set_switch(monkeypatch, "row_tiles", "0")
    run_case(get_case(cases, name), check_full=False, plan=RW_PLANS[name])


# The row-tile path forced onto every shape it takes (MQ_PLAN row_tiles=1), teacher-forced against the oracle: partial
# tiles (R not a multiple of 16 / 32), ragged episodes, VDN / QMIX / IQL, the obs_last_action / obs_agent_id = False
# branches, configs[2]'s shape at B = 4 and configs[3]'s shard.
@pytest.mark.parametrize("name,steps", [
    ("tiny_qmix", 4), ("tiny_vdn", 4), ("tiny_iql", 3), ("tiny_qmix_bare", 3), ("tiny_qmix_nola", 3),
    ("tiny_vdn_noid", 3), ("cfg2_qmix", 3), ("cfg2_qmix_ragged", 3), ("cfg3_vdn", 3), ("cfg3_qmix", 2),
    ("cfg4_qmix", 2), ("cfg1_qmix", 3)])
def test_row_tiles_teacher_forced(cases, name, steps, monkeypatch):
    set_switch(monkeypatch, "row_tiles", "1")
    learner = run_teacher_forced(get_case(cases, name), steps, False, monkeypatch)
    assert learner.last_plan()["tiles"] == 1


@pytest.mark.parametrize("name", ["tiny_qmix", "tiny_vdn"])
def test_train_from_reference_checkpoint(cases, name):
    """Load the checkpoint the REFERENCE wrote after golden step 2 (weights_only), train golden step 3 on the GPU
    and match the reference's step-3 stats, parameters and RMSprop state (row f4, q_learner.py:131-143)."""
    import os
    from pymarl_amd.components.episode_buffer import SampledBatch
    from tests.golden_utils import GOLDEN
    from tests.gpu_helpers import CKPT, build, flat_params, rel
    case = get_case(cases, name)
    args, buf, mac, learner, logger = build(case)
    learner.load_models(os.path.join(GOLDEN, CKPT[name]))
    if learner.mixer is not None:
        # load_models restores the target agent only (q_learner.py:137-142); in the reference's run the target
        # mixer equals the online one after the step-2 target update (episode 200), so the test sets it so
        learner.target_mixer.load_state_dict(learner.mixer.state_dict())
    learner.last_target_update_episode = case.episodes[2]
    batch = SampledBatch(buf, case.z["ids"][3])
    batch = batch[:, :batch.max_t_filled()]
    learner.train(batch, 3000, case.episodes[3])
    st = learner.last_stats()
    for s_ in STATS:
        ref = float(case.z["stat_" + s_][3])
        assert abs(st[s_] - ref) <= 1e-4 * abs(ref) + 1e-6, (name, s_, st[s_], ref)
    assert rel(flat_params(learner), case.z["step_params"][3]) < 1e-4
    assert rel(learner._sq.cpu().numpy(), case.z["sqavg_final"]) < 1e-4


def test_greedy_select_actions(cases):
    """BasicMAC.select_actions(test_mode=True) (HIP mac step + greedy kernel) vs the reference's."""
    from tests.gpu_helpers import build
    case = get_case(cases, "tiny_qmix")
    args, buf, mac, learner, logger = build(case)
    ids = case.z["ids"][0]
    from pymarl_amd.components.episode_buffer import SampledBatch
    batch = SampledBatch(buf, ids)
    ref = case.z["greedy_actions"]
    mac.init_hidden(case.B)
    got = [mac.select_actions(batch, t_ep=t, t_env=0, test_mode=True).cpu().numpy() for t in range(ref.shape[1])]
    got = np.stack(got, 1)
    assert np.array_equal(got, ref)


def test_mac_forward_matches_learner_unroll(cases):
    """BasicMAC.forward stepped over t reproduces the learner's fused mac_out (same params)."""
    from tests.gpu_helpers import build, rel
    case = get_case(cases, "tiny_qmix_full")
    args, buf, mac, learner, logger = build(case)
    from pymarl_amd.components.episode_buffer import SampledBatch
    batch = SampledBatch(buf, case.z["ids"][0])
    mac.init_hidden(case.B)
    outs = [mac.forward(batch, t).cpu().numpy() for t in range(batch.max_t_filled())]
    mo = np.stack(outs, 1)
    assert rel(mo, case.z["step0_mac_out"]) < 2e-5


def set_state_from_oracle(learner, o):
    """Load the oracle's params / target params / RMSprop state into the GPU learner's flat buffers."""
    with th.no_grad():
        learner._online[:learner.n_params].copy_(th.from_numpy(o.flat("params")))
        learner._target[:learner.n_params].copy_(th.from_numpy(o.flat("targets")))
        learner._sq.copy_(th.from_numpy(o.flat("sq")))


UNFUSED_KEYS = ("unfused_fwd", "unfused_bwd")   # MQ_PLAN items (pymarl_amd/csrc/switches.hpp)


@pytest.mark.parametrize("name,steps,unfused", [
    ("cfg2_qmix", 20, False), ("cfg2_vdn", 10, False), ("cfg2_qmix_ragged", 5, False), ("tiny_qmix", 4, False),
    ("tiny_vdn", 4, False),
    # BASELINE configs[2] / configs[3] shapes: the row-batched (unfused) recurrences and the GEMM path run here
    ("cfg3_vdn", 4, False), ("cfg3_qmix", 3, False), ("cfg4_qmix", 4, False),
    # IQL (mixer None) and the kernel variants past the fused limits (WIDE_PLANS), reference-pinned cases
    ("tiny_iql", 4, False), ("cfg2_iql", 4, False), ("rw2_qmix", 3, False), ("rw4_vdn", 3, False),
    ("wide_qmix", 3, False), ("cfg3_vdn_b128", 2, False),
    # the A/B switches: the unfused kernel sequence on the shapes the fused kernels normally take
    ("cfg2_qmix", 4, True), ("cfg2_qmix_ragged", 3, True), ("tiny_vdn", 2, True), ("tiny_qmix_bare", 2, True),
    # reference branches no shipped config takes (double_q / obs_last_action / obs_agent_id = False) and BASELINE
    # configs[0]'s learner shape (3m: n = 3, A = 9, O = 30, S = 48, T = 60, B = 8)
    ("tiny_qmix_nodq", 4, False), ("tiny_qmix_nola", 4, False), ("tiny_vdn_noid", 4, False),
    ("tiny_qmix_bare", 4, False), ("cfg2_qmix_nodq", 5, False), ("cfg1_qmix", 10, False), ("cfg1_vdn", 5, False)])
def test_teacher_forced_steps(cases, name, steps, unfused, monkeypatch):
    learner = run_teacher_forced(get_case(cases, name), steps, unfused, monkeypatch)
    if name == "cfg3_vdn_b128":   # BASELINE configs[2] itself: the bench's plan (row tiles, no fused kernels)
        plan = learner.last_plan()
        assert plan["tiles"] == 1 and plan["fused_fwd"] == 0 and plan["fused_bwd"] == 0, plan


@pytest.mark.parametrize("name,steps", [("cfg2_qmix", 3), ("cfg2_qmix_ragged", 3), ("tiny_vdn", 3),
                                        ("tiny_qmix_bare", 3), ("cfg1_qmix", 3)])
@pytest.mark.parametrize("pair", ["0", "1"])
def test_forward_pair_switch_teacher_forced(cases, name, steps, pair, monkeypatch):
    """Both one-wave agent forwards teacher-forced against the oracle: the row-pair kernel (gru_fwd_pair.hpp, both nets
    of a row per workgroup; the default when the rows fit the CUs) and the one-row-net kernel it replaced there
    (MQ_PLAN fwd_pair=0; still the forward past one wave of rows, e.g. configs[3]'s shard)."""
    set_switch(monkeypatch, "fwd_pair", pair)
    learner = run_teacher_forced(get_case(cases, name), steps, False, monkeypatch)
    assert learner.last_plan()["fused_fwd"] == (2 if pair == "1" else 1)


@pytest.mark.parametrize("name,steps,flow", [
    ("tiny_qmix", 4, "cpu_to"), ("cfg2_qmix", 3, "cpu_to"), ("cfg2_qmix_ragged", 3, "cpu_to"), ("cfg1_qmix", 4, "cpu_to"),
    ("tiny_vdn", 3, "cpu_to"), ("tiny_qmix", 4, "dense_slice"), ("cfg1_qmix", 4, "dense_slice")])
def test_reference_replay_flows(cases, name, steps, flow, monkeypatch):
    """The learner fed the way the reference's run loop feeds it, teacher-forced against the oracle with step 0 also
    against the reference's own golden stats:
    * cpu_to: buffer_cpu_only (run.py:137-139) — a host ReplayBuffer, then sample -> max_t_filled -> [:, :max_t] ->
      `.to(args.device)` in place (run.py:208-215) -> train; the moved batch is dense (no episode ids) and the
      learner takes the dense kernel path;
    * dense_slice: a dense device EpisodeBatch of the full T + 1 steps sliced to [:, :max_t] (the reference's own
      buffer kept on the GPU), so the kernels read it with t_stride = T + 1 > t_len."""
    run_teacher_forced(get_case(cases, name), steps, False, monkeypatch, flow=flow)


def sample_like_reference(buf, case, args, flow):
    """One batch as run.py:207-215 builds it (flow "view": this repo's HBM replay view, ids gathered in-kernel)."""
    batch = buf.sample(case.B)
    if flow == "dense_slice":
        full = batch.materialize()   # a dense [B][T+1] device EpisodeBatch, as the reference's __getitem__ returns
        return full[:, :batch.max_t_filled()]
    max_ep_t = batch.max_t_filled()
    batch = batch[:, :max_ep_t]
    if flow == "cpu_to" and batch.device != args.device:
        batch.to(args.device)
        assert batch.dense and batch["obs"].is_cuda
    return batch


def run_teacher_forced(case, steps, unfused, monkeypatch, flow="view", huber=0.0):
    """Every step from the oracle's state; decisions, stats, gradients and the RMSprop step checked (see module doc).
    huber > 0: the opt-in masked Huber TD loss with that delta on both sides (no reference golden for it)."""
    from oracle.qlearner_np import OracleQLearner
    from tests.gpu_helpers import build, flat_grads, flat_params, rel
    name = case.name
    for k in UNFUSED_KEYS:   # read once, at handle creation (mq_create)
        set_switch(monkeypatch, k, True if unfused else None)
    over = {"td_loss": "huber", "huber_delta": huber} if huber else {}
    args, buf, mac, learner, logger = build(case, buffer_device="cpu" if flow == "cpu_to" else None, **over)
    o = OracleQLearner(case.agent_params, case.mixer_params, dict(case.cfg(), huber_delta=huber))
    np.random.seed(case.sampler_seed)
    rec = []
    strided = truncated = 0
    regimes = set()
    for k in range(steps):
        batch = sample_like_reference(buf, case, args, flow)
        if flow == "dense_slice":
            strided += int(batch["obs"].stride(0) != batch.max_seq_length * case.n * case.O)
            truncated += int(batch.max_seq_length < case.T + 1)
        nb, _ = case.batch(k)
        set_state_from_oracle(learner, o)
        p_prev, sq_prev = o.flat("params").astype(np.float64), o.flat("sq").astype(np.float64)
        fw = o.forward(nb)
        learner.train(batch, 1000 * k, case.episodes[k])
        st = learner.last_stats()
        if flow != "view":
            assert learner.last_plan()["inline_ids"] == 0, "a dense batch must not take the episode-id path"
        if huber:
            ax = np.abs(fw["td"] * fw["mask"])[fw["mask"] > 0]
            regimes |= {"quadratic"} if (ax <= huber).any() else set()
            regimes |= {"linear"} if (ax > huber).any() else set()
        if k == 0 and "stat_loss" in case.z and not huber:   # the reference golden run's start: its stats
            for s_ in STATS:
                ref = float(case.z["stat_" + s_][0])
                assert abs(st[s_] - ref) <= 1e-4 * abs(ref) + 1e-6, (name, flow, s_, st[s_], ref)
        r, got, on_gpu = classify_decisions(learner, o, nb, fw)
        r["step"] = k
        rec.append(r)
        # double-Q argmax exact wherever the top-2 margin > MARGIN_EPS * max(1, |Q|); relu decisions exact wherever
        # |pre-activation| > RELU_EPS
        assert r["dq_flips_outside_ties"] == 0, (name, k, r)
        assert r["relu_flips_outside_ties"] == 0, (name, k, r)
        # on the near-ties the GPU may pick the other (equally valid in fp32 noise) branch: the oracle follows it
        st_o = o.train(nb, 1000 * k, case.episodes[k], cur_max_override=got, relu_override=on_gpu)
        for s_ in STATS:
            assert abs(st[s_] - st_o[s_]) <= 1e-5 * abs(st_o[s_]) + 1e-6, (name, k, s_, st[s_], st_o[s_])
        g_or = np.concatenate([v.ravel() for v in o.last["grads"].values()])
        g_gpu = flat_grads(learner)
        assert rel(g_gpu, g_or) < 1e-4, (name, k)
        r["grad_err_per_tensor"] = per_tensor_err(case, g_gpu, g_or)
        # RMSprop (q_learner.py:30, torch.optim.RMSprop) on the GPU's own clipped gradient: exact up to rounding.
        # Against the oracle's parameters only an O(lr) band holds: the per-element 1/(sqrt(v)+eps) normalisation
        # turns a 1e-4-of-max gradient difference on a tiny-|g| element into an O(lr) step difference.
        g64 = g_gpu.astype(np.float64)
        sq_exp = 0.99 * sq_prev + 0.01 * g64 * g64
        p_exp = p_prev - 5e-4 * g64 / (np.sqrt(sq_exp) + 1e-5)
        assert rel(learner._sq.cpu().numpy(), sq_exp) < 1e-5, (name, k)
        assert rel(flat_params(learner), p_exp) < 1e-6, (name, k)
        assert np.abs(flat_params(learner) - o.flat("params")).max() <= 20 * 5e-4, (name, k)
    if huber:
        assert regimes == {"quadratic", "linear"}, (name, regimes)   # both branches of the loss exercised
    if flow == "dense_slice":   # every truncated batch is read in place with t_stride = T + 1 > t_len
        assert strided == truncated, (strided, truncated)
        assert case.name != "cfg1_qmix" or strided == steps
    tag = "_tiles" if "row_tiles=1" in os.environ.get("MQ_PLAN", "").split(",") else ""
    write_record("teacher" + ("_unfused" if unfused else "") + tag + ("_huber" if huber else "")
                 + ("" if flow == "view" else "_" + flow), name, rec)
    return learner


@pytest.mark.parametrize("name", ["tiny_qmix", "tiny_vdn", "tiny_iql", "cfg2_qmix"])
def test_huber_teacher_forced(cases, name, monkeypatch):
    """The opt-in masked Huber TD loss (mq_config.huber_delta; north_star names it, the reference has L2 only, so
    parity is against the oracle's Huber branch, unpinned by any reference golden): stats, gradients and the
    RMSprop step from the oracle's state, with deltas that put transitions in both the quadratic and linear
    regimes."""
    case = get_case(cases, name)
    run_teacher_forced(case, 3, False, monkeypatch, huber=1.0)


def test_data_parallel_norm_path_single_rank(cases):
    """The data-parallel apply path (norm recomputed after the all-reduce) on one rank equals the local path."""
    from tests.gpu_helpers import build, flat_params, rel
    case = get_case(cases, "tiny_qmix")
    outs = []
    for force in (False, True):
        args, buf, mac, learner, logger = build(case)
        learner.force_dp_norm = force
        np.random.seed(case.sampler_seed)
        for k in range(2):
            batch = buf.sample(case.B)
            learner.train(batch[:, :batch.max_t_filled()], 1000 * k, case.episodes[k])
        outs.append((flat_params(learner), learner.last_stats()["grad_norm"]))
    assert rel(outs[1][0], outs[0][0]) < 1e-6
    assert abs(outs[1][1] - outs[0][1]) <= 1e-5 * abs(outs[0][1])


@pytest.mark.parametrize("name", ["cfg2_qmix", "cfg4_qmix", "cfg1_qmix", "tiny_qmix_full", "cfg2_qmix_ragged"])
def test_hyper_in_forward_grid_bitwise(cases, name, monkeypatch):
    """The QMIX hypernet as workgroups appended to the fused forward's grid (MQ_PLAN hyp_in_fwd=1; the default for
    shards past two row-nets per CU, e.g. cfg4) equals hyper_ws_kernel launched after the forward (MQ_PLAN
    hyp_in_fwd=0) bitwise:
    parameters, gradients, square_avg and stats over up to four steps, ragged M (cfg1: M = 480, tiny) and the
    two-wave forward of configs[3]'s shard (cfg4) included."""
    from tests.gpu_helpers import build, flat_grads, flat_params
    case = get_case(cases, name)
    outs = []
    set_switch(monkeypatch, "fwd_pair", "0")   # both arms on the one-row-net forward (the pair kernel has no HYP grid)
    for inf in ("1", "0"):
        set_switch(monkeypatch, "hyp_in_fwd", inf)
        args, buf, mac, learner, logger = build(case)
        np.random.seed(case.sampler_seed)
        for k in range(min(4, len(case.episodes))):
            batch = buf.sample(case.B)
            learner.train(batch[:, :batch.max_t_filled()], 1000 * k, case.episodes[k])
        th.cuda.synchronize()
        assert learner.last_plan()["hyper"] == "ws" and learner.last_plan()["fused_fwd"] == 1
        outs.append((flat_params(learner), flat_grads(learner), learner._sq.cpu().numpy(), learner.last_stats()))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][2], outs[1][2])
    assert outs[0][3] == outs[1][3]


@pytest.mark.parametrize("name", ["cfg2_qmix", "cfg1_qmix", "tiny_qmix_full", "cfg2_qmix_ragged"])
def test_pair_hyper_epilogue_bitwise(cases, name, monkeypatch):
    """The QMIX hypernet inside the row-pair forward — on waves 4 / 5 during the T loop (the default when every
    hypernet block has a workgroup) or as the kernel's epilogue (MQ_PLAN pair_hyp_epi, and the default otherwise) —
    equals hyper_ws_kernel launched after the forward (MQ_PLAN hyp_in_fwd=0) bitwise: parameters, gradients, square_avg
    and stats over up to four steps, ragged M included."""
    from tests.gpu_helpers import build, flat_grads, flat_params
    case = get_case(cases, name)
    outs = []
    set_switch(monkeypatch, "fwd_pair", "1")
    for inf, epi in ((None, False), (None, True), ("0", False)):
        if epi:
            set_switch(monkeypatch, "pair_hyp_epi")
        else:
            set_switch(monkeypatch, "pair_hyp_epi", None)
        if inf is None:
            set_switch(monkeypatch, "hyp_in_fwd", None)
        else:
            set_switch(monkeypatch, "hyp_in_fwd", inf)
        args, buf, mac, learner, logger = build(case)
        np.random.seed(case.sampler_seed)
        for k in range(min(4, len(case.episodes))):
            batch = buf.sample(case.B)
            learner.train(batch[:, :batch.max_t_filled()], 1000 * k, case.episodes[k])
        th.cuda.synchronize()
        assert learner.last_plan()["hyper"] == "ws" and learner.last_plan()["fused_fwd"] == 2
        outs.append((flat_params(learner), flat_grads(learner), learner._sq.cpu().numpy(), learner.last_stats()))
    for o in outs[1:]:
        assert np.array_equal(outs[0][0], o[0])
        assert np.array_equal(outs[0][1], o[1])
        assert np.array_equal(outs[0][2], o[2])
        assert outs[0][3] == o[3]


@pytest.mark.parametrize("name", ["cfg3_vdn", "cfg3_qmix", "cfg3_vdn_b128"])
def test_mix_stream_bitwise(cases, name, monkeypatch):
    """configs[2]'s mixer with the selection rows staged by the workgroup (mix_kernel<true>, the default where
    n * A <= 1024) equals the per-lane generic form (MQ_PLAN mix_generic) bitwise, double-Q argmax included."""
    from tests.gpu_helpers import build, flat_grads, flat_params
    case = get_case(cases, name)
    outs = []
    for gen in ("0", "1"):
        if gen == "1":
            set_switch(monkeypatch, "mix_generic")
        else:
            set_switch(monkeypatch, "mix_generic", None)
        args, buf, mac, learner, logger = build(case)
        np.random.seed(case.sampler_seed)
        for k in range(min(2, len(case.episodes))):
            batch = buf.sample(case.B)
            learner.train(batch[:, :batch.max_t_filled()], 1000 * k, case.episodes[k])
        th.cuda.synchronize()
        assert learner.last_plan()["mix"] == ("generic" if gen == "1" else "stream")
        outs.append((flat_params(learner), flat_grads(learner), learner.last_stats()))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][2] == outs[1][2]


@pytest.mark.parametrize("name,generic", [("cfg3_vdn_b128", False), ("cfg3_vdn_b128", True), ("cfg2_qmix", False),
                                          ("tiny_qmix_full", False), ("cfg3_qmix", True)])
def test_avail_bits_bitwise(cases, name, generic, monkeypatch):
    """The mixer's double-Q selection reading the replay buffer's avail bitmask (mq_replay.avail_bits, the default
    for buffer views) equals it reading avail_actions (learner.use_avail_bits = False) bitwise, in the staged
    (stream), per-lane (MQ_PLAN mix_generic) and fast mixers; the chosen argmax actions too."""
    from tests.gpu_helpers import build, flat_grads, flat_params
    case = get_case(cases, name)
    if generic:
        set_switch(monkeypatch, "mix_generic")
    outs = []
    for bits in (True, False):
        args, buf, mac, learner, logger = build(case)
        learner.use_avail_bits = bits
        assert buf.avail_bits is not None
        np.random.seed(case.sampler_seed)
        acts = []
        for k in range(min(2, len(case.episodes))):
            batch = buf.sample(case.B)
            learner.train(batch[:, :batch.max_t_filled()], 1000 * k, case.episodes[k])
            acts.append(learner.last_cur_max_actions().cpu().numpy())
        th.cuda.synchronize()
        outs.append((flat_params(learner), flat_grads(learner), learner.last_stats(), acts))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])
    assert outs[0][2] == outs[1][2]
    for a, b in zip(outs[0][3], outs[1][3]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["cfg2_qmix", "cfg4_qmix", "cfg1_qmix", "tiny_qmix_full"])
def test_dwh_in_bptt_grid_bitwise(cases, name, monkeypatch):
    """dW_hyper's tiles appended to the fused BPTT's grid (MQ_PLAN dwh_in_bwd=1; the default for shards past the CU
    count, e.g. cfg4) equal dW_hyper in the reduction's launch (MQ_PLAN dwh_in_bwd=0) bitwise: parameters,
    gradients, square_avg and stats over up to four steps; the plan reports where it ran."""
    from tests.gpu_helpers import build, flat_grads, flat_params
    case = get_case(cases, name)
    outs = []
    for inb in ("1", "0"):
        set_switch(monkeypatch, "dwh_in_bwd", inb)
        args, buf, mac, learner, logger = build(case)
        np.random.seed(case.sampler_seed)
        for k in range(min(4, len(case.episodes))):
            batch = buf.sample(case.B)
            learner.train(batch[:, :batch.max_t_filled()], 1000 * k, case.episodes[k])
        th.cuda.synchronize()
        plan = learner.last_plan()
        assert plan["fused_bwd"] == 1 and plan["dwh"] == ("bptt_grid" if inb == "1" else "red1"), plan
        outs.append((flat_params(learner), flat_grads(learner), learner._sq.cpu().numpy(), learner.last_stats()))
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])
    assert np.array_equal(outs[0][2], outs[1][2])
    assert outs[0][3] == outs[1][3]


