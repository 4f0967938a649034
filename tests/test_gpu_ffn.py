"""The feed-forward agent (use_rnn: False, epymarl's key) on the GPU, against tests/ref64.py on ffn_ref.py's cases.

* Every gradient block of two train() steps against the float64 reference, by tests/test_gpu_hyper2.py's procedure and
  ref64's tolerance rule with e32 from the reference's float32 run: step 1 starts from the GPU's own parameters; the
  GPU's double-Q argmax and both relus (intermediates 3 and 9) differ from the reference's on near-ties only and are
  followed. Rows: tests/ffn_ref.ROW_SHAPES under QMIX, `part` also under VDN and mixer: None, with the four input-flag
  combinations, through the TD(lambda) passes at td_lambda = 0 and beside the two-layer hypernet; and the chain's own
  partitions: `tiles` with ffn_dp2_kernel capped at two workgroups (19 rounds each, the last partial), `split` (two
  split-K slices of both weight-gradient GEMMs) and `walk` (16 slices, two rounds per workgroup; VDN). The measured
  err / max(e32, 2e-7) of every block goes to $MQ_PARITY_DIR/parity_grad64_ffn_<row>.json.
* The forward: Q of both nets, relu(fc1) and relu(rnn) of every row (padded steps included) against float64 under
  err <= 16 max(e32, 2e-7 max|ref|); mq_last_agent and the plan report the path.
* Acting: RNNAgent.forward and BasicMAC.forward per step against RefFFAgent in float64 under the same rule; the greedy
  actions are the learner's double-Q choices on the same parameters; a NaN hidden state reaches neither output.
* The rest of the step: RMSprop / Adam on the GPU's own clipped gradient, two runs bitwise equal, a PER step at beta = 0
  bitwise the uniform step, a checkpoint round trip, two data-parallel ranks against one process.
* Beside it a learner without the key reports the plan it always did, mq_last_agent() == 0 and no intermediate 9.

The step runs the GEMM chain (ffn_kernels.hpp) on every row: there is no fused kernel, and mq_last_agent() is 1.
"""
import copy
import os
import socket
from collections import OrderedDict
from types import SimpleNamespace as SN

import numpy as np
import pytest
import torch as th

from tests import act_ref64 as A64
from tests import ffn_ref as R
from tests import ref64
from tests import test_gpu_parity as P
from tests.gpu_helpers import build, flat_grads, flat_params, flat_targets, rel, set_switch

pytestmark = pytest.mark.gpu

NEW = ["rnn.weight", "rnn.bias"]
ZERO_ITEMS = ("fused_fwd", "rw_fwd", "fused_bwd", "rw_bwd", "tiles", "bwd_lean")
STATS = ["loss", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean"]


@pytest.fixture(scope="module")
def cases():
    return {}


def get_case(cases, row, mixer=None, flags=(True, True)):
    mixer = mixer or R.ROW_SHAPES[row].get("mixer", "qmix")
    key = (row, mixer, flags)
    if key not in cases:
        cases[key] = R.synth_case(row, mixer, flags=flags)
    return cases[key]


def check_path(learner, case):
    """The step ran the feed-forward agent's chain and says so."""
    plan = learner.last_plan()
    assert learner.last_agent() == 1, learner.last_agent()
    for k in ZERO_ITEMS:
        assert plan[k] == 0, (k, plan)
    assert plan["dwh"] == "red1" and plan["rows"] == case.B * case.n, plan
    assert plan["hyper_layers"] == (0 if case.mixer != "qmix" else 2 if case.He else 1), plan
    return plan


# ---------------------------------------------------------------------------------------------- gradient blocks
# row id: (ffn_ref row, mixer, (obs_last_action, obs_agent_id), MQ_PLAN switches, plan items the row must report)
ROWS = OrderedDict([
    ("one", ("one", "qmix", (True, True), {}, dict(rows=1))),
    ("part", ("part", "qmix", (True, True), {}, dict(mix="fast16", rows=9))),
    ("part_vdn", ("part", "vdn", (True, True), {}, dict(hyper="none"))),
    ("part_iql", ("part", "none", (True, True), {}, dict(hyper="none"))),
    ("tiles", ("tiles", "qmix", (True, True), {}, dict(rows=21))),
    ("wideI", ("wideI", "qmix", (True, True), {}, {})),
    ("A33", ("A33", "qmix", (True, True), {"mix_generic": True}, dict(mix="generic"))),
    ("n17", ("n17", "qmix", (True, True), {}, dict(mix="stream"))),
    ("ragged", ("ragged", "qmix", (True, True), {}, {})),
    ("part_la", ("part", "qmix", (True, False), {}, {})),
    ("part_id", ("part", "qmix", (False, True), {}, {})),
    ("part_bare", ("part", "qmix", (False, False), {}, {})),
    # td_lambda = 0 through the TD(lambda) passes: the one-step target, so the same reference applies
    ("part_lambda0", ("part", "qmix", (True, True), {"lambda_path": 1}, dict(td_lambda=1))),
    ("part_h2", ("part_h2", "qmix", (True, True), {}, dict(hyper="gemm"))),
    # the chain's partitions (tests/test_ffn_host.py asserts each from the plan): two ffn_dp2_kernel workgroups of 19
    # rounds, the second partial; two split-K slices; 16 slices and two rounds per workgroup
    ("tiles_dp2", ("tiles", "qmix", (True, True), {"ffn_dp2_blocks": 2}, dict(rows=21))),
    ("split", ("split", "qmix", (True, True), {}, dict(rows=36))),
    ("walk", ("walk", "vdn", (True, True), {}, dict(rows=128, hyper="none"))),
])


def decisions(learner, case):
    out = [learner.last_cur_max_actions().cpu().numpy(), learner.last_intermediate(3).cpu().numpy() > 0,
           learner.last_intermediate(9).cpu().numpy() > 0]
    if case.He:
        out.append(learner.last_intermediate(7).cpu().numpy() > 0)
    return out


@pytest.mark.parametrize("row", list(ROWS))
def test_grad_blocks_vs_ref64(cases, row, monkeypatch):
    shape, mixer, flags, switches, want = ROWS[row]
    case = get_case(cases, shape, mixer, flags)
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
        plan = check_path(learner, case)
        norm_gpu = learner.last_stats()["grad_norm"]
        assert np.isfinite(g_gpu).all(), (row, k)
        dec = decisions(learner, case)
        assert dec[2].shape == (case.B, nb["obs"].shape[1], case.n, 64)
        own = ref64.ref_step(case, params, targets, nb)   # the reference's own decisions at this state
        r = ref64.classify(own, dec[0], dec[1], dec[2])
        assert r["dq_flips_outside_ties"] == 0, (row, k, r)
        assert r["relu_flips_outside_ties"] == 0, (row, k, r)
        assert r["hid_relu_flips_outside_ties"] == 0, (row, k, r)
        over = dict(cur_max_override=dec[0], relu_override=dec[1], hid_relu_override=dec[2])
        if case.He:
            hyp_tie = np.abs(own.a1) <= ref64.RELU_EPS
            assert int(((dec[3] != (own.a1 > 0)) & ~hyp_tie).sum()) == 0, (row, k)
            over["hyp_relu_override"] = dec[3]
        ref = ref64.ref_step(case, params, targets, nb, **over)
        if case.mixer == "qmix":
            ref64.assert_clear_of_kinks(ref, "{} step {}".format(row, k))
        e32 = ref64.block_errors(ref64.ref_step(case, params, targets, nb, dtype=th.float32, **over).clipped_flat,
                                 ref.clipped, case)
        errs = ref64.block_errors(g_gpu, ref.clipped, case)
        tol = ref64.tolerances(e32)
        ratio = ref64.ratios(errs, e32)
        worst = max(ratio, key=ratio.get)
        norm_err = abs(norm_gpu - ref.norm) / ref.norm
        print("{} step {}: worst ratio {:.2f} at {} (err {:.3g}, e32 {:.3g}, tol {:.3g}); grad_norm rel {:.3g}; "
              "dq ties/flips {}/{}, relu ties/flips {}/{}, hid relu ties/flips {}/{}".format(
                  row, k, ratio[worst], worst, errs[worst], e32[worst], tol[worst], norm_err, r["dq_ties"],
                  r["dq_flips"], r["relu_ties"], r["relu_flips"], r["hid_relu_ties"], r["hid_relu_flips"]))
        rec.append(dict(step=k, plan=plan, agent=learner.last_agent(), decisions=r, grad_norm=norm_gpu,
                        ref_grad_norm=ref.norm, worst_block=worst, worst_ratio=ratio[worst],
                        kinks=ref64.kink_minima(ref) if case.mixer == "qmix" else None,
                        blocks={b: dict(err=errs[b], e32=e32[b], tol=tol[b], ratio=ratio[b]) for b in errs}))
        bad += [(k, b, e, t) for b, (e, t) in ref64.failures(errs, tol).items()]
        for key, v in want.items():
            assert plan[key] == v, (row, key, plan)
        assert norm_err <= 1e-5, (row, k, norm_gpu, ref.norm)
        for key in ("loss", "td_error_abs", "q_taken_mean", "target_mean"):
            got_s = learner.last_stats()[key]
            assert abs(got_s - ref.stats[key]) <= 1e-5 * abs(ref.stats[key]) + 1e-6, (row, k, key)
    P.write_record("grad64_ffn", row, rec)
    assert not bad, (row, bad)


# ---------------------------------------------------------------------------------------------- the forward
def judge(bad, name, got, ref, c32):
    r, err, e32, scale = A64.ratio(got, ref, c32)
    print("{}: ratio {:.3g} (err {:.3g}, e32 {:.3g}, max|ref| {:.3g})".format(name, r, err, e32, scale))
    if not A64.passes(r):
        bad.append((name, r, err, e32, scale))
    return r


@pytest.mark.parametrize("row", list(R.ROW_SHAPES))
def test_forward_vs_ref64(cases, row):
    case = get_case(cases, row)
    args, buf, mac, learner, logger = build(case, **case.over())
    np.random.seed(case.sampler_seed)
    batch = buf.sample(case.B)
    batch = batch[:, :batch.max_t_filled()]
    nb, _ = case.batch(0)
    p = flat_params(learner)
    learner.train(batch, 0, case.episodes[0])
    check_path(learner, case)
    r64 = ref64.ref_step(case, p, p, nb)
    r32 = ref64.ref_step(case, p, p, nb, dtype=th.float32)
    bad, rec = [], {}
    for which, name in ((0, "mac_out"), (1, "target_mac_out_full"), (3, "x1"), (9, "hid")):
        got = learner.last_intermediate(which).cpu().numpy()
        ref = getattr(r64, name)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)   # every row of every step, padded ones included
        rec[name] = judge(bad, "{} {}".format(row, name), got, ref, getattr(r32, name))
    P.write_record("fwd64_ffn", row, rec)
    assert not bad, (row, bad)
    if row == "ragged":   # a padded step's row: the storage's zeros in, fc2(relu(rnn(relu(fc1(one-hot id))))) out
        filled = nb["filled"][:, :, 0]
        b, t = np.argwhere(filled == 0)[0]
        got = learner.last_intermediate(0).cpu().numpy()[b, t]
        assert np.abs(got - r64.mac_out[b, t]).max() <= 1e-5 * np.abs(r64.mac_out).max()


def test_param_offsets_follow_the_flat_buffer(cases):
    from pymarl_amd import _lib
    case = get_case(cases, "part")
    args, buf, mac, learner, logger = build(case, **case.over())
    np.random.seed(case.sampler_seed)
    batch = buf.sample(case.B)
    learner.train(batch[:, :batch.max_t_filled()], 0, 0)
    offs = dict(zip(_lib.PARAM_NAMES, learner._handle.offsets))
    total = learner._handle.offsets[-1]
    assert total == learner.n_params
    o = 0
    for k, s in list(case.agent_shapes.items()) + list(case.mixer_shapes.items()):
        assert offs[k] == o, (k, offs[k], o)
        o += int(np.prod(s))
    for k in ("rnn.weight_ih", "rnn.weight_hh", "rnn.bias_ih", "rnn.bias_hh", "hyper_w_1.2.weight"):
        assert offs[k] == total, k   # absent: zero floats at the end of the buffer
    assert _lib.PARAM_NAMES.index("rnn.weight") == 22   # behind MQ_P_HWF_B2: the earlier entries keep their numbers


# ---------------------------------------------------------------------------------------------- acting
@pytest.mark.parametrize("rows", [1, 33, 257])
def test_agent_forward_vs_ref64(rows):
    from pymarl_amd.modules.agents.rnn_agent import RNNAgent
    I, A = 42, 9
    th.manual_seed(100 + rows)
    mod = R.RefFFAgent(I, A)
    m64 = copy.deepcopy(mod).double()
    agent = RNNAgent(I, SN(hidden_dim=64, n_actions=A, n_agents=1, obs_last_action=False, obs_agent_id=False,
                           use_rnn=False)).cuda()
    agent.load_state_dict(mod.state_dict())
    x = 3.0 * th.randn(rows, I)
    x[-1] = 0.0
    with th.no_grad():
        q64, h64 = m64(x.double())
        q32, h32 = mod(x)
    garbage = th.full((rows, 64), float("nan"), device="cuda")   # h_in does not reach q or h_out
    q, h = agent(x.cuda(), garbage)
    assert q.shape == (rows, A) and h.shape == (rows, 64)
    assert th.isfinite(q).all() and th.isfinite(h).all() and (h >= 0).all()
    bad = []
    judge(bad, "agent q rows={}".format(rows), q.cpu().numpy(), q64.numpy(), q32.numpy())
    judge(bad, "agent h rows={}".format(rows), h.cpu().numpy(), h64.numpy(), h32.numpy())
    assert not bad, bad
    q2, h2 = agent(x.cuda(), None)   # any hidden_state
    assert th.equal(q2, q) and th.equal(h2, h)


def test_mac_forward_per_step_and_greedy_actions_are_the_learners(cases):
    from pymarl_amd.components.action_selectors import greedy_actions
    case = get_case(cases, "ragged")
    args, buf, mac, learner, logger = build(case, **case.over())
    flags = (True, True)
    N, n, Tp = case.n_episodes, case.n, case.T + 1
    p64 = A64.named64(case.agent_params)
    mod = R.RefFFAgent(case.I, case.A)
    mod.load_state_dict({k: th.from_numpy(v) for k, v in case.agent_params.items()})
    m64 = copy.deepcopy(mod).double()
    m64.load_state_dict(p64)
    full = buf[0:N]
    mac.init_hidden(N)
    mac.hidden_states = th.full((N, n, 64), float("nan"), device="cuda")   # garbage in: not read
    bad, qs = [], []
    for t in range(Tp):
        q = mac.forward(full, t)
        assert q.shape == (N, n, case.A) and mac.hidden_states.shape == (N, n, 64)
        x64 = A64.build_inputs(case.data["obs"], case.data["actions"], case.data["filled"], t, case.A, flags)
        with th.no_grad():
            q64, h64 = m64(x64)
            q32, h32 = mod(x64.float())
        judge(bad, "mac q[{}]".format(t), q.reshape(N * n, -1).cpu().numpy(), q64.numpy(), q32.numpy())
        judge(bad, "mac h[{}]".format(t), mac.hidden_states.reshape(N * n, 64).cpu().numpy(), h64.numpy(), h32.numpy())
        qs.append(q.clone())
    assert not bad, bad
    # the same parameters through the learner: its double-Q greedy choice at t + 1 is the MAC's greedy action there
    np.random.seed(case.sampler_seed)
    batch = buf.sample(case.B)
    ids = batch.ep_ids_np
    batch = batch[:, :batch.max_t_filled()]
    nb, _ = case.batch(0)
    learner.train(batch, 0, 0)
    cur = learner.last_cur_max_actions().cpu().numpy()   # (B, T, n)
    mo = learner.last_intermediate(0).cpu().numpy()
    T = cur.shape[1]
    checked = 0
    for t in range(T):
        qt = qs[t + 1][th.as_tensor(ids, device="cuda")]
        assert np.abs(qt.cpu().numpy() - mo[:, t + 1]).max() <= 1e-5 * np.abs(mo).max()
        avail = th.as_tensor(nb["avail_actions"][:, t + 1], device="cuda").int()
        act = greedy_actions(qt, avail).cpu().numpy()
        masked = np.where(nb["avail_actions"][:, t + 1] == 0, -9999999.0, mo[:, t + 1].astype(np.float64))
        top2 = -np.sort(-masked, axis=2)[..., :2]
        clear = (top2[..., 0] - top2[..., 1]) > ref64.MARGIN_EPS * np.maximum(1.0, np.abs(top2[..., 0]))
        clear &= nb["avail_actions"][:, t + 1].sum(-1) > 0
        assert (act[clear] == cur[:, t][clear]).all(), t
        checked += int(clear.sum())
    assert checked > 0


# ---------------------------------------------------------------------------------------------- the rest of the step
def run_steps(case, steps, **over):
    args, buf, mac, learner, logger = build(case, **dict(case.over(), **over))
    np.random.seed(case.sampler_seed)
    for k in range(steps):
        batch = buf.sample(case.B)
        learner.train(batch[:, :batch.max_t_filled()], 1000 * k, case.episodes[k])
    th.cuda.synchronize()
    return buf, learner


def torch_rmsprop(p, g, sq, dtype, lr=5e-4, alpha=0.99, eps=1e-5):
    """torch.optim.RMSprop's step on the CPU in `dtype` from float32 inputs: (p, square_avg) float64."""
    t = lambda a: th.tensor(np.asarray(a, np.float32), dtype=dtype)  # noqa: E731
    w = th.nn.Parameter(t(p))
    opt = th.optim.RMSprop([w], lr=lr, alpha=alpha, eps=eps, foreach=False)
    opt.state[w]["step"] = th.tensor(0.0)
    opt.state[w]["square_avg"] = t(sq)
    w.grad = t(g)
    opt.step()
    return w.detach().double().numpy(), opt.state[w]["square_avg"].double().numpy()


def test_rmsprop_step_on_the_gpus_own_gradient_and_target_update(cases):
    case = get_case(cases, "part")
    args, buf, mac, learner, logger = build(case, **case.over())
    np.random.seed(case.sampler_seed)
    for k in range(2):
        p0, sq0, t0 = flat_params(learner), learner._sq.cpu().numpy().copy(), flat_targets(learner)
        batch = buf.sample(case.B)
        learner.train(batch[:, :batch.max_t_filled()], 1000 * k, case.episodes[k])
        g = flat_grads(learner)
        assert np.abs(g).max() > 0
        r64, r32 = torch_rmsprop(p0, g, sq0, th.float64), torch_rmsprop(p0, g, sq0, th.float32)
        bad = []
        for name, got, b64, b32 in zip(("p", "square_avg"), (flat_params(learner), learner._sq.cpu().numpy()), r64, r32):
            judge(bad, "rmsprop step {} {}".format(k, name), got, b64, b32)
        assert not bad, bad
        assert np.array_equal(flat_targets(learner), t0)   # the target has not been updated yet
    gn = case.unflatten(flat_grads(learner))
    p1 = case.unflatten(flat_params(learner))
    for name in NEW:   # the optimiser reaches the new tensors
        assert np.abs(gn[name]).max() > 0 and not np.array_equal(p1[name], case.agent_params[name]), name
    learner._update_targets()
    th.cuda.synchronize()
    assert np.array_equal(flat_targets(learner), flat_params(learner))
    for k, v in learner.target_mac.agent.state_dict().items():   # the module views see it too
        assert np.array_equal(v.cpu().numpy(), p1[k]), k


def test_adam_steps_are_torch_adam_steps(cases):
    from tests.test_gpu_adam import train_checked
    case = get_case(cases, "part")
    args, buf, mac, learner, logger = build(case, optimizer="adam", **case.over())
    assert type(learner.optimiser) is th.optim.Adam
    np.random.seed(case.sampler_seed)
    for k in range(2):
        batch = buf.sample(case.B)
        train_checked(learner, batch[:, :batch.max_t_filled()], 1000 * k, case.episodes[k], k, "ffn adam step {}".format(k))
        assert learner.last_agent() == 1


def test_two_runs_are_bitwise_equal(cases):
    case = get_case(cases, "tiles")
    outs = []
    for _ in range(2):
        buf, learner = run_steps(case, 2)
        outs.append((flat_grads(learner), flat_params(learner), learner._sq.cpu().numpy(),
                     learner._stats.cpu().numpy(), learner.last_intermediate(9).cpu().numpy()))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_per_step_at_beta_zero_is_the_uniform_step_bitwise(cases):
    from pymarl_amd.components.episode_buffer import SampledBatch
    from tests.test_gpu_per import make_per_buffer, step_outputs
    case = get_case(cases, "part")
    args, buf, mac, learner, logger = build(case, **case.over())
    pbuf = make_per_buffer(case, per_alpha=0.6, per_beta=0.0, per_eps=1e-6, seed=5)
    pbuf.load_arrays(case.data)
    pb = pbuf.sample(case.B)
    learner.train(pb, 0, case.episodes[0])
    got = step_outputs(learner)
    assert learner.last_plan()["per"] == 1 and learner.last_agent() == 1
    assert np.array_equal(pb.weights.cpu().numpy(), np.ones(case.B, np.float32))
    ids = pb.ep_ids.cpu().numpy()
    _, buf2, _, uniform, _ = build(case, **case.over())
    uniform.train(SampledBatch(buf2, ids, pb.t_len), 0, case.episodes[0])
    ref = step_outputs(uniform)
    assert uniform.last_plan()["per"] == 0
    assert np.abs(ref["grads"]).max() > 0
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k


@pytest.mark.parametrize("opt", ["rmsprop", "adam"])
def test_checkpoint_round_trip_changes_nothing(cases, tmp_path, opt):
    """Step, target update, [save, load into a fresh learner,] step: bitwise the same with and without the bracket."""
    from pymarl_amd.components.episode_buffer import SampledBatch
    case = get_case(cases, "part")
    ids = case.z["ids"]
    over = dict(case.over(), **({"optimizer": "adam"} if opt == "adam" else {}))

    def step(learner, buf, k):
        b = SampledBatch(buf, ids[k])
        learner.train(b[:, :b.max_t_filled()], 1000 * k, case.episodes[k])

    args, buf, mac, a, logger = build(case, **over)
    step(a, buf, 0)
    a._update_targets()
    th.cuda.synchronize()
    a.save_models(str(tmp_path))
    sd = th.load(str(tmp_path / "agent.th"), weights_only=True)
    assert list(sd) == list(case.agent_shapes)   # epymarl's keys in the file
    step(a, buf, 1)
    th.cuda.synchronize()

    _, buf2, mac2, b, _ = build(case, **over)
    b.load_models(str(tmp_path))
    b.target_mixer.load_state_dict(b.mixer.state_dict())
    b.last_target_update_episode = a.last_target_update_episode
    step(b, buf2, 1)
    th.cuda.synchronize()
    assert b.last_agent() == 1
    assert np.array_equal(flat_grads(b), flat_grads(a))
    assert np.array_equal(flat_params(b), flat_params(a))
    assert np.array_equal(b._sq.cpu().numpy(), a._sq.cpu().numpy())
    if opt == "adam":
        assert np.array_equal(b._m.cpu().numpy(), a._m.cpu().numpy())


def test_plain_epymarl_state_dict_loads_into_the_learners_agent(cases, tmp_path):
    case = get_case(cases, "part")
    th.manual_seed(9)
    mod = R.RefFFAgent(case.I, case.A)
    th.save(mod.state_dict(), str(tmp_path / "agent.th"))
    args, buf, mac, learner, logger = build(case, **case.over())
    mac.load_models(str(tmp_path))
    flat = th.cat([p.detach().reshape(-1) for p in mod.parameters()])
    assert th.equal(learner._online[:flat.numel()].cpu(), flat)   # the kernels' buffer holds it
    x = th.randn(5, case.I)
    with th.no_grad():
        q32, h32 = mod(x)
    q, h = mac.agent(x.cuda(), None)
    assert (q.cpu() - q32).abs().max() <= 1e-5 * q32.abs().max()


# ---------------------------------------------------------------------------------------------- data parallel
DP_STEPS = 2


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
        record["agent"].append(learner.last_agent())


def _dp_worker(rank, world, port, out_path):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    th.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        case = R.synth_case("ragged")
        args, buf, mac, learner, logger = build(case, learner_dp=True, **case.over())
        rec = {"stats": [], "grads": [], "params": [], "agent": []}
        _dp_train(learner, buf, case, rec)
        th.cuda.synchronize()
        if rank == 0:
            np.savez(out_path, **{k: np.asarray(v) for k, v in rec.items()})
    finally:
        dist.destroy_process_group()


def test_two_rank_dp_equals_single_process(cases, tmp_path):
    """tests/test_gpu_dp.py's two ranks on one GPU (gloo on device tensors) with the feed-forward agent on the ragged
    row (3 episodes: shards of 2 and 1 with unequal mask sums)."""
    import torch.multiprocessing as mp
    out = str(tmp_path / "dp.npz")
    mp.spawn(_dp_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    dp = np.load(out)
    case = get_case(cases, "ragged")
    args, buf, mac, learner, logger = build(case, **case.over())
    ref = {"stats": [], "grads": [], "params": [], "agent": []}
    _dp_train(learner, buf, case, ref)
    assert list(dp["agent"]) == ref["agent"] == [1] * DP_STEPS
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


# ---------------------------------------------------------------------------------------------- unchanged beside it
@pytest.mark.parametrize("kw", [{}, dict(use_rnn=True)])
def test_without_the_key_the_gru_step_is_the_one_it_was(kw):
    from pymarl_amd import _lib
    from tests.test_plan_host import PARENT
    case = ref64.synth_case("base")
    args, buf, mac, learner, logger = build(case, **kw)
    np.random.seed(case.sampler_seed)
    batch = buf.sample(case.B)
    batch = batch[:, :batch.max_t_filled()]
    learner.train(batch, 0, case.episodes[0])
    rec = PARENT["rows"]["base"]
    assert batch.max_seq_length == rec["t_len"]
    plan = learner.last_plan()
    assert {k: plan[k] for k in rec["plan"]} == rec["plan"], plan
    assert learner.last_agent() == 0
    with pytest.raises(_lib.MQError, match="feed-forward"):
        learner.last_intermediate(9)
    offs = dict(zip(_lib.PARAM_NAMES, learner._handle.offsets))
    assert offs["rnn.weight"] == offs["rnn.bias"] == learner.n_params   # absent: zero floats at the end
    assert offs["rnn.weight_ih"] == 64 * case.I + 64
    assert list(mac.agent.state_dict())[2] == "rnn.weight_ih"


def test_with_the_key_the_same_shape_runs_another_step():
    """The same data and shape with use_rnn: False: another parameter count, another loss, the chain's report."""
    d = ref64.SHAPES["base"]
    case = R.SynthCaseF("ffn_base", n_episodes=d["B"], steps=1, mixer="qmix", ragged=True, min_len=1, **d)
    gcase = ref64.synth_case("base")
    _, buf, _, ffn, _ = build(case, **case.over())
    _, gbuf, _, gru, _ = build(gcase)
    for c, b, l in ((case, buf, ffn), (gcase, gbuf, gru)):
        np.random.seed(c.sampler_seed)
        batch = b.sample(c.B)
        l.train(batch[:, :batch.max_t_filled()], 0, 0)
    assert ffn.n_params == gru.n_params - 6 * 64 * 64 - 6 * 64 + 64 * 64 + 64
    assert ffn.last_agent() == 1 and gru.last_agent() == 0
    assert abs(ffn.last_stats()["loss"] - gru.last_stats()["loss"]) > 1e-3 * gru.last_stats()["loss"]
