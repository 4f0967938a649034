"""ActorCriticLearner.train() on the GPU against the independent restatement tests/a2c_ref.py.

Per row of a2c_ref.ROWS two train() calls (step 0 from the case's weights and zero optimiser state, step 1 from the
GPU's own state after step 0, read back and given to the float64 and the float32 reference alike), and per step:

1. the reference's kink_minima are above the row's margin, before train() runs;
2. the returns (ma_copy_intermediate 2) are bitwise the float32 per-element restatement fed the GPU's own V' (and, under
   reward standardisation, the GPU's own running statistics);
3. both clipped gradients and both optimisers' moments per block under ref64's rule min(1e-5, 16 max(e32, 2e-7)); both
   parameter updates per block against a float64 torch.optim step on the GPU's own gradient (a2c_ref.judge_updates);
4. V', V and pi to 1e-5, the nine stats to 1e-4 |ref| + 1e-6, both grad norms to 1e-5 relative, everything finite;
and each row asserts its edge from ma_last_plan. The other tests: an all-empty batch changes nothing, two runs are
bitwise equal, the three target-update modes against torch, checkpoints, BasicMAC.forward with soft_policies, and the
standalone critic forward against float64. Per-block figures go to $MQ_PARITY_DIR/parity_a2c_<row>.json.
"""
import os

import numpy as np
import pytest
import torch as th

from tests import a2c_ref as R
from tests import test_gpu_parity as P
from tests.a2c_helpers import all_buffers, build_a2c, learner_state
from tests.gpu_helpers import rel

pytestmark = pytest.mark.gpu

# what each row's plan must show: the edge exists in what was launched, not in the shape alone
EDGES = {
    "one": lambda p, c: p["rows"] == 2 and p["policy_blocks"] == 1 and p["fwd_tiles"] == 1 and p["dv_blocks"] == 1 and
    p["ns_cw1"] == p["ns_cw2"] == p["ns_aw1"] == p["ns_aw2"] == 1,
    "part": lambda p, c: p["k"] % 4 != 0 and p["vec16"] == 0 and p["kp"] == p["k"] + 3 and p["rows"] % 64 != 0,
    "rows9": lambda p, c: p["rows"] == 9 and p["policy_tail"] == 1 and p["policy_blocks"] == 3,
    "A33": lambda p, c: p["policy_lanes"] == 33 and p["ap"] == 36,   # lanes past one half-wave, three pad columns
    "A64": lambda p, c: p["policy_lanes"] == 64 == p["ap"],   # every lane live, no pad column
    "split": lambda p, c: p["rows"] == 544 and p["ns_cw1"] >= 2 and p["ns_cw2"] >= 2 and p["ns_aw1"] >= 2 and
    p["dv_blocks"] > 1,
    "wide": lambda p, c: p["hidden"] == 128,
    "part_ac": lambda p, c: p["k"] == c.O + c.n and p["reward_norm"] == 1 and p["adam"] == 0,
    "part_n10": lambda p, c: p["k"] == c.S + c.n and p["reward_norm"] == 1 and p["adam"] == 0,
    "part_ac_adam": lambda p, c: p["k"] == c.O + c.n and p["reward_norm"] == 0 and p["adam"] == 1,
}


def sample(buf, c):
    batch = buf.sample(c.B)
    return batch[:, :batch.max_t_filled()]


def rewards32(c, nb, learner):
    """The rewards the n-step pass read, float32: the storage's, or standardised with the GPU's own statistics."""
    x = np.asarray(nb["reward"][:, :-1], np.float32)
    if not c.keys["standardise_rewards"]:
        return x
    mean, var, _ = learner.rew_ms.tolist()
    return ((x - np.float32(mean)) / np.sqrt(np.float32(var))).astype(np.float32)


@pytest.mark.parametrize("row", list(R.ROWS))
def test_a2c_vs_ref(row):
    c = R.A2CCase(row)
    args, buf, mac, learner, logger = build_a2c(c)
    nb = c.batch()
    records, bad = [], []
    for k in range(2):
        batch = sample(buf, c)
        assert batch.max_seq_length == nb["filled"].shape[1] == R.ROWS[row]["t_len"]
        state = learner_state(learner)
        r64, r32 = R.a2c_ref_step(c, state, nb, R.F64), R.a2c_ref_step(c, state, nb, R.F32)
        for relu, v in r64.kink_minima.items():   # 1, before the GPU runs
            assert v > R.MARGIN, "{} step {}: min|{}| = {:.3g} over live rows is within the margin {:g} of the " \
                "kink; choose another seed for this row".format(row, k, relu, v, R.MARGIN)
        learner.train(batch, 1000 * (k + 1), 8 * k)
        plan, st = learner.last_plan(), learner.last_stats()
        assert EDGES[row](plan, c), (row, plan)
        after = learner_state(learner)
        Pa, Pc = learner.n_agent_params, learner.n_critic_params
        agrad, cgrad = learner._agrad.detach().cpu().numpy(), learner._cgrad.detach().cpu().numpy()
        got = dict(cgrad=cgrad[:Pc], agrad=agrad[:Pa], c_v=after["c_v"], a_v=after["a_v"], c_m=after["c_m"],
                   a_m=after["a_m"])
        for q, v in got.items():
            assert np.isfinite(v).all(), (row, k, q)
        assert all(np.isfinite(st[s]) for s in R.STATS), (row, k, st)
        assert cgrad[Pc + 1] == agrad[Pa + 1] == r64.M == st["mask_elems"], (row, k, cgrad[Pc + 1], r64.M)
        assert after["step"] == state["step"] + 1 and learner.critic_training_steps == k + 1
        # 2: the returns, bitwise
        inter = {i: learner.last_intermediate(i).cpu().numpy() for i in range(5)}
        ret32 = R.nstep_elem(inter[0], rewards32(c, nb, learner), r32.mask, c.gpow, c.keys["q_nstep"],
                             c.keys["add_value_last_step"])
        assert np.array_equal(ret32, inter[2]), (row, k, np.abs(ret32 - inter[2]).max())
        # 3: gradients and moments per block against float64; updates against the optimiser on the GPU's own gradient
        rec, bad_k = R.judge(c, r64, r32, got)
        rec_u, bad_u = R.judge_updates(c, state, dict(agent=got["agrad"], critic=got["cgrad"]), after)
        rec.update(rec_u)
        bad += [(k,) + b for b in bad_k + bad_u]
        w = R.worst(rec)
        # 4: outputs, stats, norms
        qerr = dict(Vt=rel(inter[0], r64.Vt), V=rel(inter[1], r64.V), pi=rel(inter[3], r64.pi),
                    ret=rel(inter[2], r64.ret), dlogits=rel(inter[4] / r64.M, r64.dlogits))
        norm_err = dict(critic=abs(st["critic_grad_norm"] - r64.critic_norm) / r64.critic_norm,
                        agent=abs(st["agent_grad_norm"] - r64.agent_norm) / r64.agent_norm)
        print("{} step {}: M {}, worst ratio {:.2f} at {} {} (err {:.3g}, e32 {:.3g}, tol {:.3g}); norms rel {:.2g} / "
              "{:.2g}; V' / V / pi / ret / dlogits {:.2g} / {:.2g} / {:.2g} / {:.2g} / {:.2g}; kinks {}".format(
                  row, k, r64.M, w[2], w[0], w[1], rec[w[0]][w[1]]["err"], rec[w[0]][w[1]]["e32"],
                  rec[w[0]][w[1]]["tol"], norm_err["critic"], norm_err["agent"], qerr["Vt"], qerr["V"], qerr["pi"],
                  qerr["ret"], qerr["dlogits"], {a: "{:.3g}".format(b) for a, b in r64.kink_minima.items()}))
        records.append(dict(step=k, plan=plan, kink_minima=r64.kink_minima, margin=R.MARGIN,
                            worst=dict(quantity=w[0], block=w[1], ratio=w[2]), norm_err=norm_err, errors=qerr,
                            stats={s: (st[s], r64.stats[s]) for s in R.STATS}, blocks=rec))
        for name in ("Vt", "V", "pi"):
            assert qerr[name] < 1e-5, (row, k, name, qerr[name])
        for s in R.STATS:
            assert abs(st[s] - r64.stats[s]) <= 1e-4 * abs(r64.stats[s]) + 1e-6, (row, k, s, st[s], r64.stats[s])
        assert norm_err["critic"] <= 1e-5 and norm_err["agent"] <= 1e-5, (row, k, norm_err)
        if c.keys["standardise_rewards"]:
            ms = learner.reward_stats()
            for name, ref in zip(("mean", "var", "count"), r64.new["rew_ms"]):
                assert abs(ms[name] - ref) <= 1e-12 * max(1.0, abs(ref)), (row, k, name, ms[name], ref)
    P.write_record("a2c", row, records)
    assert not bad, (row, bad)


@pytest.mark.parametrize("row", ["part", "part_n10"])
def test_empty_batch_changes_nothing(row):
    """Gate 5: a batch whose mask is empty leaves every buffer (the running reward statistics included: part_n10
    standardises its rewards), both optimisers' step counts and critic_training_steps as they were, after a first live
    step has filled the moments."""
    c = R.A2CCase(row)
    args, buf, mac, learner, logger = build_a2c(c)
    learner.train(sample(buf, c), 1000, 0)
    empty = {k: v.copy() for k, v in c.data.items()}
    empty["filled"][:] = 0
    _, ebuf, _, _, _ = build_a2c(c, data=empty)
    before, steps = all_buffers(learner), (learner._opt_steps, float(learner._step_t), learner.critic_training_steps,
                                           learner.last_target_update_step)
    learner.train(ebuf.sample(c.B)[:, :c.T + 1], 2000, 8)
    after = all_buffers(learner)
    assert learner.last_stats()["mask_elems"] == 0.0
    assert ("rew_ms" in before) == c.keys["standardise_rewards"] and learner.last_plan()["reward_norm"] == int(
        c.keys["standardise_rewards"])
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert steps == (learner._opt_steps, float(learner._step_t), learner.critic_training_steps,
                     learner.last_target_update_step)
    for opt in (learner.agent_optimiser, learner.critic_optimiser):
        assert all(float(s["step"]) == 1.0 for s in opt.state.values())


def test_two_runs_bitwise_equal():
    """Gate 6."""
    c = R.A2CCase("split")
    runs = []
    for _ in range(2):
        args, buf, mac, learner, logger = build_a2c(c)
        for k in range(2):
            learner.train(sample(buf, c), 1000 * (k + 1), 8 * k)
        runs.append((all_buffers(learner), learner._stats.cpu().numpy().copy()))
    for k in runs[0][0]:
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), k
    assert np.array_equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("mode,value", [("soft", 0.01), ("hard", 2.0), ("absent", None)])
def test_target_updates(mode, value):
    """Gate 7: soft bitwise torch's fp32 t * (1.0 - tau) + p * tau on the read-back parameters; hard every `value`
    critic training steps; the key absent: hard every target_update_interval critic training steps."""
    c = R.A2CCase("part")
    over = dict(target_update_interval=3) if mode == "absent" else dict(target_update_interval_or_tau=value)
    args, buf, mac, learner, logger = build_a2c(c, **over)
    every = {"hard": 2, "absent": 3}.get(mode)
    tgt = learner._tcritic.cpu().clone()
    for k in range(4):
        learner.train(sample(buf, c), 1000 * (k + 1), 8 * k)
        on = learner._critic.cpu().clone()
        if mode == "soft":
            tgt = tgt * (1.0 - value) + on * value
        elif (k + 1) % every == 0:
            tgt = on
        assert th.equal(learner._tcritic.cpu(), tgt), (mode, k)
    assert learner.critic_training_steps == 4


def test_checkpoints_round_trip(tmp_path):
    """Gate 8: bitwise through save_models / load_models; a plain-torch critic_opt.th loads."""
    for row in ("part", "part_n10"):
        c = R.A2CCase(row)
        args, buf, mac, learner, logger = build_a2c(c)
        for k in range(2):
            learner.train(sample(buf, c), 1000 * (k + 1), 8 * k)
        d = tmp_path / row
        os.makedirs(d)
        learner.save_models(str(d))
        for f in ("agent.th", "critic.th", "agent_opt.th", "critic_opt.th"):
            th.load(str(d / f), weights_only=True)
        _, buf2, _, fresh, _ = build_a2c(c)
        fresh.load_models(str(d))
        a, b = all_buffers(learner), all_buffers(fresh)
        for k in a:
            if k in ("_agrad", "_cgrad", "_tcritic"):   # not saved: gradients; the target restarts from the critic
                continue
            assert np.array_equal(a[k], b[k]), (row, k)
        assert fresh._opt_steps == learner._opt_steps == 2
        if fresh.rew_ms is not None:
            assert th.equal(fresh.rew_ms.cpu(), learner.rew_ms.cpu())
        # the same next step from both
        fresh._tcritic.copy_(learner._tcritic)
        learner.train(sample(buf, c), 3000, 16)
        fresh.train(sample(buf2, c), 3000, 16)
        a, b = all_buffers(learner), all_buffers(fresh)
        for k in a:
            assert np.array_equal(a[k], b[k]), (row, k)
        # a critic_opt.th written by plain torch over the same parameter shapes
        ps = [th.nn.Parameter(th.zeros(s)) for s in c.critic_shapes.values()]
        opt = th.optim.Adam(ps, lr=c.keys["lr"]) if c.keys["optimizer"] == "adam" else \
            th.optim.RMSprop(ps, lr=c.keys["lr"], alpha=c.keys["optim_alpha"], eps=c.keys["optim_eps"])
        for p in ps:
            p.grad = th.full_like(p, 0.25)
        opt.step()
        th.save(opt.state_dict(), str(d / "critic_opt.th"))
        fresh.load_models(str(d))
        key = "exp_avg_sq" if c.keys["optimizer"] == "adam" else "square_avg"
        want = np.concatenate([opt.state[p][key].numpy().ravel() for p in ps])
        assert np.array_equal(fresh._csq.cpu().numpy(), want), row


@pytest.mark.parametrize("mbs", [True, False])
def test_basic_mac_soft_policies(mbs):
    """Gate 9: BasicMAC.forward with soft_policies over a ragged episode batch against torch's softmax of the same
    logits; test_mode changes nothing; select_actions never returns an unavailable action under the mask.
    Under the mask the rows compared are those with an available action: a slot the runner never wrote has none, and
    mc_policy (unchanged, the COMA learner's) then returns zeros outside test_mode (its floor divides by the number of
    available actions and every action is zeroed as unavailable) and the uniform softmax of equal logits inside it.
    No rollout step reads such a row."""
    c = R.A2CCase("part")
    args, buf, mac, learner, logger = build_a2c(c, mask_before_softmax=mbs)
    batch = sample(buf, c)
    mac.init_hidden(c.B)
    th.manual_seed(5)
    for t in range(batch.max_seq_length):
        h_in = mac.hidden_states.clone()
        out = mac.forward(batch, t, test_mode=False)
        mac.hidden_states = h_in
        out_test = mac.forward(batch, t, test_mode=True)
        avail_t = batch["avail_actions"][:, t]
        rows = (avail_t.sum(-1) > 0) if mbs else th.ones_like(avail_t[..., 0], dtype=th.bool)
        assert th.equal(out[rows], out_test[rows]), t
        # the logits of the same step from the agent module, then torch's softmax
        from pymarl_amd.learners.q_learner import replay_view
        avail = batch["avail_actions"][:, t]
        hd = mac.agent.handle()
        logits = th.empty(c.B * c.n, c.A, device=out.device)
        h_out = th.empty_like(h_in.reshape(c.B * c.n, -1))
        rep, keep = replay_view(batch)
        from pymarl_amd import _lib
        _lib.check(hd.lib.mq_mac_forward(hd.h, rep, t, _lib.ptr(h_in.reshape(c.B * c.n, -1).contiguous()),
                                         _lib.ptr(h_out), _lib.ptr(logits), 0, _lib.stream_ptr()))
        lg = logits.view(c.B, c.n, c.A).double()
        if mbs:
            lg = lg.masked_fill(avail == 0, -1e10)
        ref = th.softmax(lg, -1)
        assert (out.double() - ref)[rows].abs().max().item() <= 1e-6, t
        eps_ok = th.nonzero(rows.all(-1)).reshape(-1)   # the episodes a runner would still be stepping at t
        if mbs and len(eps_ok):
            for test_mode in (False, True):
                mac.hidden_states = h_in
                a = mac.select_actions(batch, t, 0, bs=eps_ok, test_mode=test_mode)
                assert tuple(a.shape) == (len(eps_ok), c.n)
                assert bool((th.gather(avail[eps_ok], 2, a.unsqueeze(-1)) != 0).all()), (t, test_mode)


@pytest.mark.parametrize("row", ["part", "part_ac", "wide", "part_n10"])
def test_standalone_critic_forward(row):
    """Gate 10: the module's forward(batch) and forward(batch, t) against float64, both kinds, both widths; and the
    module's torch input builder against the reference's dense construction."""
    c = R.A2CCase(row)
    args, buf, mac, learner, logger = build_a2c(c)
    batch = sample(buf, c)
    nb = c.batch()
    X = R.critic_inputs(c, nb, R.F64)
    assert th.equal(learner.critic.build_inputs(batch).double().cpu(), X)
    P64 = {k: th.tensor(np.asarray(v, np.float64)) for k, v in c.critic_params.items()}
    h = th.relu(th.relu(X @ P64["fc1.weight"].T + P64["fc1.bias"]) @ P64["fc2.weight"].T + P64["fc2.bias"])
    ref = (h @ P64["fc3.weight"].T + P64["fc3.bias"]).numpy()
    v = learner.critic.forward(batch)
    assert tuple(v.shape) == (c.B, nb["filled"].shape[1], c.n, 1)
    assert rel(v.cpu().numpy(), ref) < 1e-5
    for t in (0, 2, nb["filled"].shape[1] - 1):
        vt = learner.critic.forward(batch, t)
        assert tuple(vt.shape) == (c.B, 1, c.n, 1)
        assert rel(vt[:, 0].cpu().numpy(), ref[:, t]) < 1e-5, t
        assert rel(vt[:, 0].cpu().numpy(), v[:, t].cpu().numpy()) < 1e-6, t
    with pytest.raises(IndexError):
        learner.critic.forward(batch, nb["filled"].shape[1])
