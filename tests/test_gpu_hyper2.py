"""The two-layer QMIX hypernetwork (hypernet_layers: 2) on the GPU, against tests/ref64.py on hyper2_ref.py's cases.

* QMixer.forward (mq_qmix_forward2) against the restated upstream module in float64: the GPU's error is at most
  16 * max(error of the same module in fp32 on the CPU, 2e-7 * max|ref|).
* Every gradient block of two train() steps against the float64 reference, by tests/test_gpu_grad_blocks.py's
  procedure and ref64's tolerance rule with e32 from the reference's float32 run: step 1 starts from the GPU's own
  parameters; the GPU's double-Q argmax, fc1 relu and hypernet layer-1 relu (intermediate 7) decisions differ from
  the reference's on near-ties only and are followed; the second-layer outputs and V.0 keep clear of their kinks.
  The measured err / max(e32, 2e-7) of every block goes to $MQ_PARITY_DIR/parity_grad64_h2_<row>.json.
* The optimiser and target update reach the new tensors; two runs are bitwise equal; a PER step at beta = 0 is the
  uniform step bitwise; a checkpoint round trip changes nothing; two data-parallel ranks equal one process.
* The reference's own CPU QLearner with the restated two-layer mixer (tests/golden/tiny_qmix_h2.npz,
  make_golden_hyper2.py): the loss trajectory, step-0 intermediates and gradient, parameters, targets and square_avg.
"""
import copy
import os
import socket
from collections import OrderedDict
from types import SimpleNamespace as SN

import numpy as np
import pytest
import torch as th

from tests import hyper2_ref as R
from tests import ref64
from tests import test_gpu_parity as P
from tests.gpu_helpers import build, flat_grads, flat_params, flat_targets, rel, set_switch

pytestmark = pytest.mark.gpu

NEW = [k for k in R.mixer2_shapes(1, 1, 1) if k.startswith(("hyper_w_1.", "hyper_w_final."))]


# ---------------------------------------------------------------------------------------------- standalone forward
# (n, S, He, rows): one row; a partial row group; K padding; S % 4 != 0 with the branch boundary at column 64; 576
# second-layer columns; S > 192
FWD = [(3, 48, 64, 1), (3, 48, 64, 33), (3, 48, 20, 33), (2, 30, 64, 33), (17, 40, 64, 5), (2, 200, 64, 7)]


@pytest.mark.parametrize("n,S,He,rows", FWD)
def test_standalone_forward(n, S, He, rows):
    from pymarl_amd.modules.mixers.qmix import QMixer
    th.manual_seed(1000 * n + S + He + rows)
    ref32 = R.RefQMixer2(n, S, 32, He)
    ref64_ = copy.deepcopy(ref32).double()
    m = QMixer(SN(n_agents=n, state_shape=S, mixing_embed_dim=32, hypernet_layers=2, hypernet_embed=He)).cuda()
    m.load_state_dict(ref32.state_dict())
    qs, st = th.randn(rows, 1, n), th.randn(rows, 1, S)
    with th.no_grad():
        y64 = ref64_(qs.double(), st.double())
        y32 = ref32(qs, st).double()
    got = m(qs.cuda(), st.cuda())
    assert got.shape == (rows, 1, 1)
    scale = float(y64.abs().max())
    e32 = float((y32 - y64).abs().max())
    err = float((got.cpu().double() - y64).abs().max())
    print("forward n={} S={} He={} rows={}: err {:.3g}, fp32 module {:.3g}, max|ref| {:.3g}".format(
        n, S, He, rows, err, e32, scale))
    assert err <= 16 * max(e32, 2e-7 * scale), (err, e32, scale)


def test_forward_of_a_one_layer_mixer_is_unchanged_beside_it():
    """The one-layer module still goes through mq_qmix_forward (same values as before for the same weights)."""
    from pymarl_amd.modules.mixers.qmix import QMixer
    th.manual_seed(2)
    m = QMixer(SN(n_agents=3, state_shape=48, mixing_embed_dim=32)).cuda()
    qs, st = th.randn(5, 2, 3).cuda(), th.randn(5, 2, 48).cuda()
    assert th.equal(m(qs, st), m(qs, st)) and m(qs, st).shape == (5, 2, 1)


# ---------------------------------------------------------------------------------------------- gradient blocks
BASE = dict(fused_fwd=2, fused_bwd=1, bwd_lean=1, mix="fast16", tiles=0, rows=12, hyper="gemm", dwh="red1")
# row id: (hyper2_ref.ROW_SHAPES row, MQ_PLAN switches, the plan items the row must report)
ROWS = OrderedDict([
    ("base", ("base", {}, BASE)),
    ("base_he20", ("base_he20", {}, BASE)),
    ("gemm", ("gemm", {}, dict(hyper="gemm", fused_fwd=2, fused_bwd=1))),
    ("stream", ("stream", {}, dict(mix="stream"))),
    ("tiles_r21", ("tiles_r21", {"row_tiles": 1}, dict(tiles=1, rows=21))),
    ("one", ("one", {}, dict(rows=3))),
    # td_lambda = 0 through the TD(lambda) passes: the one-step target, so the same reference applies
    ("base_lambda0", ("base", {"lambda_path": 1}, dict(BASE, td_lambda=1))),
])


@pytest.fixture(scope="module")
def cases():
    return {}


def get_case(cases, row):
    if row not in cases:
        cases[row] = R.synth_case2(row)
    return cases[row]


def decisions(learner):
    return (learner.last_cur_max_actions().cpu().numpy(), learner.last_intermediate(3).cpu().numpy() > 0,
            learner.last_intermediate(7).cpu().numpy() > 0)


@pytest.mark.parametrize("row", list(ROWS))
def test_grad_blocks_vs_ref64(cases, row, monkeypatch):
    shape, switches, want = ROWS[row]
    case = get_case(cases, shape)
    for key, v in switches.items():   # read once, at handle creation
        set_switch(monkeypatch, key, v)
    args, buf, mac, learner, logger = build(case, **case.over())
    np.random.seed(case.sampler_seed)
    rec, bad = [], []
    for k in range(2):
        batch = buf.sample(case.B)
        batch = batch[:, :batch.max_t_filled()]
        nb, _ = case.batch(k)
        params, targets = flat_params(learner), flat_targets(learner)   # step 1: the GPU's own after step 0
        learner.train(batch, 1000 * k, case.episodes[k])
        g_gpu = flat_grads(learner)
        plan = learner.last_plan()
        norm_gpu = learner.last_stats()["grad_norm"]
        assert np.isfinite(g_gpu).all(), (row, k)
        assert plan["hyper_layers"] == 2, plan
        got, on_gpu, hyp_on = decisions(learner)
        assert hyp_on.shape == (case.B, nb["obs"].shape[1] - 1, 2 * case.He)
        own = ref64.ref_step(case, params, targets, nb)   # the reference's own decisions at this state
        r = ref64.classify(own, got, on_gpu, got_hyp_relu=hyp_on)
        assert r["dq_flips_outside_ties"] == 0, (row, k, r)
        assert r["relu_flips_outside_ties"] == 0, (row, k, r)
        assert r["hyp_relu_flips_outside_ties"] == 0, (row, k, r)
        over = dict(cur_max_override=got, relu_override=on_gpu, hyp_relu_override=hyp_on)
        ref = ref64.ref_step(case, params, targets, nb, **over)
        ref64.assert_clear_of_kinks(ref, "{} step {}".format(row, k))
        e32 = ref64.block_errors(ref64.ref_step(case, params, targets, nb, dtype=th.float32, **over).clipped_flat,
                                 ref.clipped, case)
        errs = ref64.block_errors(g_gpu, ref.clipped, case)
        tol = ref64.tolerances(e32)
        ratio = ref64.ratios(errs, e32)
        worst = max(ratio, key=ratio.get)
        norm_err = abs(norm_gpu - ref.norm) / ref.norm
        print("{} step {}: worst ratio {:.2f} at {} (err {:.3g}, e32 {:.3g}, tol {:.3g}); grad_norm rel {:.3g}; "
              "dq ties/flips {}/{}, relu ties/flips {}/{}, hyp relu ties/flips {}/{}".format(
                  row, k, ratio[worst], worst, errs[worst], e32[worst], tol[worst], norm_err, r["dq_ties"],
                  r["dq_flips"], r["relu_ties"], r["relu_flips"], r["hyp_relu_ties"], r["hyp_relu_flips"]))
        rec.append(dict(step=k, plan=plan, decisions=r, grad_norm=norm_gpu, ref_grad_norm=ref.norm,
                        worst_block=worst, worst_ratio=ratio[worst], kinks=ref64.kink_minima(ref),
                        blocks={b: dict(err=errs[b], e32=e32[b], tol=tol[b], ratio=ratio[b]) for b in errs}))
        bad += [(k, b, e, t) for b, (e, t) in ref64.failures(errs, tol).items()]
        for key, v in want.items():
            assert plan[key] == v, (row, key, plan)
        assert norm_err <= 1e-5, (row, k, norm_gpu, ref.norm)
        for key in ("loss", "td_error_abs", "q_taken_mean", "target_mean"):
            got_s = learner.last_stats()[key]
            assert abs(got_s - ref.stats[key]) <= 1e-5 * abs(ref.stats[key]) + 1e-6, (row, k, key)
    P.write_record("grad64_h2", row, rec)
    assert not bad, (row, bad)


# ---------------------------------------------------------------------------------------------- further cases
def run_steps(case, steps, **over):
    args, buf, mac, learner, logger = build(case, **dict(case.over(), **over))
    np.random.seed(case.sampler_seed)
    for k in range(steps):
        batch = buf.sample(case.B)
        learner.train(batch[:, :batch.max_t_filled()], 1000 * k, case.episodes[k])
    th.cuda.synchronize()
    return buf, learner


def test_optimiser_and_target_update_reach_the_new_tensors(cases):
    case = get_case(cases, "base")
    p0 = case.unflatten(ref64.flat_of(case))
    buf, learner = run_steps(case, 1)
    p1, t1 = case.unflatten(flat_params(learner)), case.unflatten(flat_targets(learner))
    g = case.unflatten(flat_grads(learner))
    sq = case.unflatten(learner._sq.cpu().numpy())
    one_minus_alpha = np.float32(1.0) - np.float32(0.99)   # the kernel's (1 - alpha), two fp32 multiplies follow
    for k in NEW:
        assert np.abs(g[k]).max() > 0, k
        moved = p1[k] != p0[k]
        assert moved[g[k] != 0].all(), k   # lr |g| / (sqrt((1 - alpha) g^2) + eps) ~ 5e-3: far above an ulp
        exp = one_minus_alpha * (g[k] * g[k])
        assert (np.abs(sq[k] - exp) <= 4 * np.spacing(np.abs(exp)) + 1e-37).all(), k
        assert np.array_equal(t1[k], p0[k]), k   # the target has not been updated yet
    learner._update_targets()
    th.cuda.synchronize()
    t2 = case.unflatten(flat_targets(learner))
    for k in t2:
        assert np.array_equal(t2[k], p1[k]), k
    assert dict(learner.mixer.state_dict()).keys() == p1.keys() - set(case.agent_shapes)
    for k, v in learner.target_mixer.state_dict().items():   # the module views see it too
        assert np.array_equal(v.cpu().numpy(), p1[k]), k


def test_two_runs_are_bitwise_equal(cases):
    case = get_case(cases, "base")
    outs = []
    for _ in range(2):
        buf, learner = run_steps(case, 2)
        outs.append((flat_grads(learner), flat_params(learner), learner._sq.cpu().numpy(),
                     learner._stats.cpu().numpy()))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_per_step_at_beta_zero_is_the_uniform_step_bitwise(cases):
    from pymarl_amd.components.episode_buffer import SampledBatch
    from tests.test_gpu_per import make_per_buffer, step_outputs
    case = get_case(cases, "base")
    args, buf, mac, learner, logger = build(case, **case.over())
    pbuf = make_per_buffer(case, per_alpha=0.6, per_beta=0.0, per_eps=1e-6, seed=5)
    pbuf.load_arrays(case.data)
    pb = pbuf.sample(case.B)
    learner.train(pb, 0, case.episodes[0])
    got = step_outputs(learner)
    plan = learner.last_plan()
    assert plan["per"] == 1 and plan["hyper_layers"] == 2, plan
    assert np.array_equal(pb.weights.cpu().numpy(), np.ones(case.B, np.float32))
    ids = pb.ep_ids.cpu().numpy()
    _, buf2, _, uniform, _ = build(case, **case.over())
    uniform.train(SampledBatch(buf2, ids, pb.t_len), 0, case.episodes[0])
    ref = step_outputs(uniform)
    assert uniform.last_plan()["per"] == 0
    assert np.abs(ref["grads"]).max() > 0
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k


def test_checkpoint_round_trip_changes_nothing(cases, tmp_path):
    """Step, target update, [save, load into a fresh learner,] step: bitwise the same with and without the bracket.
    (load_models restores the target agent from agent.th, as the reference does, so both arms update the targets
    first.)"""
    from pymarl_amd.components.episode_buffer import SampledBatch
    case = get_case(cases, "base_he20")
    ids = case.z["ids"]

    def step(learner, buf, k):
        b = SampledBatch(buf, ids[k])
        learner.train(b[:, :b.max_t_filled()], 1000 * k, case.episodes[k])

    args, buf, mac, a, logger = build(case, **case.over())
    step(a, buf, 0)
    a._update_targets()
    th.cuda.synchronize()
    a.save_models(str(tmp_path))
    sd = th.load(str(tmp_path / "mixer.th"), weights_only=True)
    assert list(sd) == list(case.mixer_shapes)   # upstream's keys in the file
    step(a, buf, 1)
    th.cuda.synchronize()

    over = dict(case.over())
    _, buf2, mac2, b, _ = build(case, **over)
    b.load_models(str(tmp_path))
    b.target_mixer.load_state_dict(b.mixer.state_dict())
    b.last_target_update_episode = a.last_target_update_episode
    step(b, buf2, 1)
    th.cuda.synchronize()
    assert b.last_plan()["hyper_layers"] == 2
    assert np.array_equal(flat_grads(b), flat_grads(a))
    assert np.array_equal(flat_params(b), flat_params(a))
    assert np.array_equal(b._sq.cpu().numpy(), a._sq.cpu().numpy())


# ---------------------------------------------------------------------------------------------- data parallel
DP_STEPS = 2
STATS = ["loss", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean"]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_train(learner, buf, case, record):
    from pymarl_amd.components.episode_buffer import SampledBatch
    for k in range(DP_STEPS):
        gb = SampledBatch(buf, case.z["ids"][k])
        gb = gb[:, :gb.max_t_filled()]
        learner.train(gb, 1000 * k, case.episodes[k])
        st = learner.last_stats()
        record["stats"].append([st[s] for s in STATS])
        record["grads"].append(flat_grads(learner))
        record["params"].append(flat_params(learner))
        record["layers"].append(learner.last_plan()["hyper_layers"])


def _dp_worker(rank, world, port, out_path):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    th.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        case = R.synth_case2("base")
        args, buf, mac, learner, logger = build(case, learner_dp=True, **case.over())
        rec = {"stats": [], "grads": [], "params": [], "layers": []}
        _dp_train(learner, buf, case, rec)
        th.cuda.synchronize()
        if rank == 0:
            np.savez(out_path, **{k: np.asarray(v) for k, v in rec.items()})
    finally:
        dist.destroy_process_group()


def test_two_rank_dp_equals_single_process(cases, tmp_path):
    """tests/test_gpu_dp.py's two ranks on one GPU (gloo on device tensors) with the two-layer mixer on the base
    shape: no new code, the gradient buffer is simply longer."""
    import torch.multiprocessing as mp
    out = str(tmp_path / "dp.npz")
    mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    dp = np.load(out)
    case = get_case(cases, "base")
    args, buf, mac, learner, logger = build(case, **case.over())
    ref = {"stats": [], "grads": [], "params": [], "layers": []}
    _dp_train(learner, buf, case, ref)
    assert list(dp["layers"]) == ref["layers"] == [2] * DP_STEPS
    # step 0 from identical state: only the order the two shards' partial sums are added in differs
    assert rel(dp["grads"][0], ref["grads"][0]) < 1e-5
    assert rel(dp["stats"][0], ref["stats"][0]) < 1e-5
    g = case.unflatten(dp["grads"][0].astype(np.float64))
    gr = case.unflatten(np.asarray(ref["grads"][0], np.float64))
    for k in NEW:   # and each new tensor on its own scale
        assert np.abs(g[k] - gr[k]).max() <= 1e-5 * np.abs(gr[k]).max(), k
    for k in range(DP_STEPS):
        assert rel(dp["stats"][k], ref["stats"][k]) < 1e-3, (k, dp["stats"][k], ref["stats"][k])
    g0 = dp["grads"][0].astype(np.float64)
    assert rel(dp["params"][0], ref64.flat_of(case) - 5e-4 * g0 / (np.sqrt(0.01 * g0 * g0) + 1e-5)) < 1e-6
    assert np.abs(dp["params"][-1] - ref["params"][-1]).max() <= 20 * 5e-4


# ---------------------------------------------------------------------------------------------- the reference's golden
def test_golden_run_of_the_reference_learner():
    """tests/golden/tiny_qmix_h2.npz held to what tests/test_gpu_parity.run_case(check_full=True) holds tiny_qmix to,
    less the numpy oracle (oracle/ has no two-layer mixer): the sampler's ids; at step 0 the five stats to LOSS_RTOL,
    mac_out / target_mac_out to 2e-5 and the clipped gradient to 1e-4; the double-Q actions exact on clear margins;
    the loss and the parameters of every step to 1e-4; the targets after the update within the O(lr) band and
    square_avg to 1e-4."""
    case = R.GoldenCase2()
    z = case.z
    args, buf, mac, learner, logger = build(case, **case.over())
    np.random.seed(case.sampler_seed)
    for k in range(case.steps):
        batch = buf.sample(case.B)
        assert np.array_equal(batch.ep_ids_np, z["ids"][k]), "sampler ids diverged from the reference"
        max_t = batch.max_t_filled()
        batch = batch[:, :max_t]
        nb, _ = case.batch(k)
        learner.train(batch, 1000 * k, case.episodes[k])
        st = learner.last_stats()
        assert learner.last_plan()["hyper_layers"] == 2
        got = learner.last_cur_max_actions().cpu().numpy()
        ref_a = z["cur_max_actions"][k][:, :got.shape[1]].astype(np.int64)
        mo = learner.last_intermediate(0).cpu().numpy()[:, 1:max_t]
        mo = np.where(nb["avail_actions"][:, 1:] == 0, np.float32(-9999999.0), mo)
        clear = z["margin"][k][:, :got.shape[1]] > P.MARGIN_EPS * np.maximum(1.0, np.abs(mo.max(axis=3)))
        assert int((got != ref_a)[clear].sum()) == 0, k
        for s_ in P.STATS:
            ref = float(z["stat_" + s_][k])
            err = abs(st[s_] - ref) / max(abs(ref), 1e-12)
            print("golden step {} {}: {:.7g} vs {:.7g} (rel {:.3g})".format(k, s_, st[s_], ref, err))
            if k == 0 or s_ == "loss":
                assert err <= P.LOSS_RTOL + 1e-6 / max(abs(ref), 1e-6), (k, s_, st[s_], ref)
        if k == 0:
            assert rel(learner.last_intermediate(0).cpu().numpy(), z["step0_mac_out"]) < 2e-5
            tmo = learner.last_intermediate(1).cpu().numpy()[:, 1:]
            avail = case.data["avail_actions"][z["ids"][0]][:, 1:max_t]
            assert rel(np.where(avail == 0, np.float32(-9999999.0), tmo), z["step0_target_mac_out"]) < 2e-5
            assert rel(flat_grads(learner), z["step0_grads_clipped"]) < 1e-4
            g = case.unflatten(flat_grads(learner).astype(np.float64))
            gr = case.unflatten(z["step0_grads_clipped"].astype(np.float64))
            for name in NEW:   # the new tensors on their own scale, at the global gate's figure
                assert np.abs(g[name] - gr[name]).max() <= 1e-4 * np.abs(gr[name]).max(), name
        assert rel(flat_params(learner), z["step_params"][k]) < 1e-4, k
    d = np.abs(flat_targets(learner).astype(np.float64) - z["targets_final"])
    assert d.max() <= 20 * 5e-4 * case.steps, float(d.max())
    assert np.array_equal(flat_targets(learner), flat_params(learner))   # the update of step 1 (episode 200) ran
    assert rel(learner._sq.cpu().numpy(), z["sqavg_final"]) < 1e-4
