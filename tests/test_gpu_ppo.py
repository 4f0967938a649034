"""PPOLearner.train() on the GPU against the independent restatement tests/ppo_ref.py.

Per row of ppo_ref.ROWS and for k = 1..E a fresh learner is built from the row's initial state with `epochs: k` and
runs one train(). Its last epoch, epoch k, is judged against the reference epoch (float64, and float32 for e32) run
from the GPU's own state after k - 1 epochs, which is the previous build's read-back; the old log-probabilities and
the returns the reference epoch is given are its own from the initial state. The gates are test_gpu_a2c.py's:

1. the reference's kink minima and its ratios' distance to the clip bounds are above the margin, before train() runs;
2. the returns are bitwise the float32 per-element restatement fed the GPU's own V' and reward statistics;
3. both clipped gradients and both optimisers' moments per block under min(1e-5, 16 max(e32, 2e-7)); both parameter
   updates per block against a float64 torch.optim step on the GPU's own gradient (a2c_ref.judge_updates);
4. V', V, pi and old to 1e-5, the epoch's nine stats to 1e-4 |ref| + 1e-6, both grad norms to 1e-5 relative, the
   reward statistics to 1e-12 and merged exactly once per train();
5. the number of live rows whose surrogate gradient is cut equals the reference's, as an integer;
6. `_opt_steps` and both optimisers' step tensors are k, `critic_training_steps` is 1.
The other tests: `epochs: 1` against ActorCriticLearner bitwise, an empty batch changes nothing, two runs are bitwise
equal, one target update per train() whatever E, checkpoints, and epymarl's mappo.yaml / ippo.yaml keys. Per-block
figures go to $MQ_PARITY_DIR/parity_ppo_<row>.json.
"""
import os

import numpy as np
import pytest
import torch as th

from tests import a2c_ref as R
from tests import ppo_ref as PR
from tests import test_gpu_parity as P
from tests.a2c_helpers import all_buffers, learner_state
from tests.gpu_helpers import rel
from tests.ppo_helpers import build_a2c_on, build_ppo
from tests.test_gpu_a2c import EDGES, rewards32, sample

pytestmark = pytest.mark.gpu


def counters(learner):
    return (learner._opt_steps, float(learner._step_t), learner.critic_training_steps,
            learner.last_target_update_step)


@pytest.mark.parametrize("row", list(PR.ROWS))
def test_ppo_epochs_vs_ref(row):
    c = PR.PPOCase(row)
    nb = c.batch()
    state = first64 = first32 = None
    records, bad, refs = [], [], []
    for k in range(1, c.epochs + 1):
        args, buf, mac, learner, logger = build_ppo(c, epochs=k)
        batch = sample(buf, c)
        assert batch.max_seq_length == nb["filled"].shape[1]
        init = learner_state(learner)
        if k == 1:
            state = init
            first64 = r64 = PR.ppo_ref_epoch(c, state, nb, None, None, PR.F64)
            first32 = r32 = PR.ppo_ref_epoch(c, state, nb, None, None, PR.F32)
        else:   # from the GPU's own state after k - 1 epochs: the previous build's read-back
            assert state["step"] == k - 1 and np.array_equal(state["target"], init["target"])
            r64 = PR.ppo_ref_epoch(c, state, nb, first64.old, first64.ret, PR.F64)
            r32 = PR.ppo_ref_epoch(c, state, nb, first32.old, first32.ret, PR.F32)
        refs.append(r64)
        for relu, v in r64.kink_minima.items():   # 1, before the GPU runs
            assert v > R.MARGIN, "{} epoch {}: min|{}| = {:.3g} over live rows is within the margin {:g} of the " \
                "kink; choose another seed for this row".format(row, k, relu, v, R.MARGIN)
        assert min(r64.bound_dist, r32.bound_dist) > R.MARGIN and np.array_equal(r64.w[r64.live], r32.w[r32.live]), \
            "{} epoch {}: a ratio within {:g} of a clip bound; choose another seed".format(row, k, R.MARGIN)
        learner.train(batch, 1000, 0)
        plan, st = learner.last_plan(), learner.last_stats()
        rn = int(c.keys["standardise_rewards"])
        assert EDGES[c.base](plan, c) and plan["epochs"] == k and plan["hoisted"] == 7 + 2 * rn, (row, plan)
        after = learner_state(learner)
        Pa, Pc = learner.n_agent_params, learner.n_critic_params
        agrad, cgrad = learner._agrad.detach().cpu().numpy(), learner._cgrad.detach().cpu().numpy()
        got = dict(cgrad=cgrad[:Pc], agrad=agrad[:Pa], c_v=after["c_v"], a_v=after["a_v"], c_m=after["c_m"],
                   a_m=after["a_m"])
        for q, v in got.items():
            assert np.isfinite(v).all(), (row, k, q)
        ep = st["epochs"]
        assert len(ep) == k and all(np.isfinite(e[s]) for e in ep for s in R.STATS), (row, k, st)
        assert cgrad[Pc + 1] == agrad[Pa + 1] == r64.M == st["mask_elems"], (row, k, cgrad[Pc + 1], r64.M)
        # 6: the counters
        assert counters(learner) == (k, float(k), 1, 0), (row, k, counters(learner))
        for opt in (learner.agent_optimiser, learner.critic_optimiser):
            assert all(float(s["step"]) == float(k) for s in opt.state.values())
        # 2: the returns, bitwise, from the GPU's own V' and the statistics merged once
        inter = {i: learner.last_intermediate(i).cpu().numpy() for i in range(7)}
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
        qerr = dict(Vt=rel(inter[0], first64.Vt), V=rel(inter[1], r64.V), pi=rel(inter[3], r64.pi),
                    ret=rel(inter[2], r64.ret), dlogits=rel(inter[4] / r64.M, r64.dlogits),
                    old=float(np.abs(inter[5] - first64.old).max()), ratio=float(np.abs(inter[6] - r64.ratio).max()))
        last = ep[-1]
        norm_err = dict(critic=abs(last["critic_grad_norm"] - r64.critic_norm) / r64.critic_norm,
                        agent=abs(last["agent_grad_norm"] - r64.agent_norm) / r64.agent_norm)
        print("{} epochs {}: M {}, cut {} (ref {}), worst ratio {:.2f} at {} {} (err {:.3g}, e32 {:.3g}, tol {:.3g}); "
              "norms rel {:.2g} / {:.2g}; V' / V / pi / ret / dlogits / old / ratio {:.2g} / {:.2g} / {:.2g} / {:.2g} / "
              "{:.2g} / {:.2g} / {:.2g}; bound distance {:.3g}; kinks {}".format(
                  row, k, r64.M, last["clipped"], r64.clipped, w[2], w[0], w[1], rec[w[0]][w[1]]["err"],
                  rec[w[0]][w[1]]["e32"], rec[w[0]][w[1]]["tol"], norm_err["critic"], norm_err["agent"], qerr["Vt"],
                  qerr["V"], qerr["pi"], qerr["ret"], qerr["dlogits"], qerr["old"], qerr["ratio"], r64.bound_dist,
                  {a: "{:.3g}".format(b) for a, b in r64.kink_minima.items()}))
        records.append(dict(epochs=k, plan=plan, kink_minima=r64.kink_minima, margin=R.MARGIN,
                            bound_dist=r64.bound_dist, clipped=(last["clipped"], r64.clipped),
                            outside_kept=r64.outside_kept,
                            worst=dict(quantity=w[0], block=w[1], ratio=w[2]), norm_err=norm_err, errors=qerr,
                            stats={s: (last[s], r64.stats[s]) for s in R.STATS}, blocks=rec))
        for name in ("Vt", "V", "pi", "old"):
            assert qerr[name] < 1e-5, (row, k, name, qerr[name])
        for s in R.STATS:   # the epoch's own, then what train() reports: critic means over the epochs, actor's last
            assert abs(last[s] - r64.stats[s]) <= 1e-4 * abs(r64.stats[s]) + 1e-6, (row, k, s, last[s], r64.stats[s])
            want = np.mean([r.stats[s] for r in refs]) if s in R.STATS[:5] else r64.stats[s]
            assert abs(st[s] - want) <= 1e-4 * abs(want) + 1e-6, (row, k, s, st[s], want)
        assert norm_err["critic"] <= 1e-5 and norm_err["agent"] <= 1e-5, (row, k, norm_err)
        # 5: the rows whose gradient is cut, as an integer
        assert last["clipped"] == r64.clipped == r32.clipped, (row, k, last["clipped"], r64.clipped, r32.clipped)
        assert st["clip_frac"] == r64.clipped / r64.M
        if k == 1:
            assert last["clipped"] == 0 and np.all(inter[6][r64.live] == 1.0)   # ratio = exp(0)
        if row == "default":
            assert st["clip_frac"] == 0.0 and r64.clipped == 0 and bool(r64.w[r64.live].all())
        if c.keys["standardise_rewards"]:   # merged once per train(), whatever k
            ms = learner.reward_stats()
            for name, ref in zip(("mean", "var", "count"), first64.new["rew_ms"]):
                assert abs(ms[name] - ref) <= 1e-12 * max(1.0, abs(ref)), (row, k, name, ms[name], ref)
            assert abs(ms["count"] - (R.REW_MS_INIT[2] + nb["reward"][:, :-1].size)) < 1e-9
        state = after
    P.write_record("ppo", row, records)
    assert not bad, (row, bad)
    if row != "default":
        assert records[-1]["clipped"][0] > 0, "the clipped branch did not run"


@pytest.mark.parametrize("row", ["part", "split", "part_n10"])
def test_one_epoch_is_the_actor_critic_learner_bitwise(row):
    """`epochs: 1`: ratio = 1 and w = 1 give c = adv bit for bit, the hoisted launches compute what the two-net launches
    compute, so every buffer is bitwise ActorCriticLearner's after one train() from the same state, and every stat but
    pg_loss (-(adv + ec H), not -(adv log pi_u + ec H)) is equal. The one word excepted is the sum behind that stat:
    the loss sum the policy kernel leaves at the head of the agent gradient buffer's tail."""
    c = PR.PPOCase(row)
    _, buf, _, ppo, _ = build_ppo(c, epochs=1)
    _, abuf, _, a2c, _ = build_a2c_on(c)
    ppo.train(sample(buf, c), 1000, 0)
    a2c.train(sample(abuf, c), 1000, 0)
    a, b = all_buffers(ppo), all_buffers(a2c)
    Pa = ppo.n_agent_params
    assert set(a) == set(b)
    for k in a:
        if k == "_agrad":
            keep = np.arange(a[k].size) != Pa
            assert np.array_equal(a[k][keep], b[k][keep]), (row, k)
            assert a[k][Pa] != b[k][Pa]   # the surrogate's loss sum is not the policy gradient's
        else:
            assert np.array_equal(a[k], b[k]), (row, k)
    sa, sb = ppo.last_stats(), a2c.last_stats()
    for s in R.STATS + ["mask_elems"]:
        if s != "pg_loss":
            assert sa[s] == sb[s], (row, s, sa[s], sb[s])
    assert sa["pg_loss"] != sb["pg_loss"] and sa["clip_frac"] == 0.0
    assert counters(ppo) == counters(a2c) == (1, 1.0, 1, 0)
    for i in range(5):
        assert th.equal(ppo.last_intermediate(i), a2c.last_intermediate(i)), (row, i)


@pytest.mark.parametrize("row", ["part", "part_n10"])
def test_empty_batch_changes_nothing(row):
    """A batch whose mask is empty leaves every buffer (the running reward statistics included: part_n10 standardises
    its rewards) and every counter as they were, with three epochs, after a first live train()."""
    c = PR.PPOCase(row)
    args, buf, mac, learner, logger = build_ppo(c)
    learner.train(sample(buf, c), 1000, 0)
    empty = {k: v.copy() for k, v in c.data.items()}
    empty["filled"][:] = 0
    _, ebuf, _, _, _ = build_ppo(c, data=empty)
    before, steps = all_buffers(learner), counters(learner)
    assert steps == (3, 3.0, 1, 0)
    learner.train(ebuf.sample(c.B)[:, :c.T + 1], 2000, 8)
    after, st = all_buffers(learner), learner.last_stats()
    assert st["mask_elems"] == 0.0 and st["clip_frac"] == 0.0 and len(st["epochs"]) == 3
    assert all(e[s] == 0.0 for e in st["epochs"] for s in R.STATS) and all(e["clipped"] == 0 for e in st["epochs"])
    assert ("rew_ms" in before) == c.keys["standardise_rewards"] and learner.last_plan()["reward_norm"] == int(
        c.keys["standardise_rewards"]) and learner.last_plan()["epochs"] == 3
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    assert steps == counters(learner)
    for opt in (learner.agent_optimiser, learner.critic_optimiser):
        assert all(float(s["step"]) == 3.0 for s in opt.state.values())


def test_two_runs_bitwise_equal():
    c = PR.PPOCase("split")
    runs = []
    for _ in range(2):
        args, buf, mac, learner, logger = build_ppo(c)
        for k in range(2):
            learner.train(sample(buf, c), 1000 * (k + 1), 8 * k)
        assert counters(learner)[:3] == (6, 6.0, 2)
        runs.append((all_buffers(learner), learner._estats.cpu().numpy().copy(),
                     learner.last_intermediate(5).cpu().numpy(), learner.last_intermediate(6).cpu().numpy()))
    for k in runs[0][0]:
        assert np.array_equal(runs[0][0][k], runs[1][0][k]), k
    for i in (1, 2, 3):
        assert np.array_equal(runs[0][i], runs[1][i]), i


@pytest.mark.parametrize("mode,value", [("soft", 0.01), ("hard", 2.0), ("absent", None)])
@pytest.mark.parametrize("epochs", [1, 3])
def test_one_target_update_per_train(mode, value, epochs):
    """Soft: bitwise torch's fp32 t * (1.0 - tau) + p * tau once per train(), after the last epoch; hard every `value`
    train() calls; the key absent: hard every target_update_interval train() calls. Whatever E."""
    c = PR.PPOCase("part")
    over = dict(target_update_interval=3) if mode == "absent" else dict(target_update_interval_or_tau=value)
    args, buf, mac, learner, logger = build_ppo(c, epochs=epochs, **over)
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
    assert learner.critic_training_steps == 4 and learner._opt_steps == 4 * epochs


def test_checkpoints_round_trip(tmp_path):
    """Save, load into a fresh learner, and the next train() is bitwise equal (the actor-critic learner's files)."""
    for row in ("part", "part_n10"):
        c = PR.PPOCase(row)
        args, buf, mac, learner, logger = build_ppo(c)
        learner.train(sample(buf, c), 1000, 0)
        d = tmp_path / row
        os.makedirs(d)
        learner.save_models(str(d))
        assert set(os.listdir(d)) == {"agent.th", "critic.th", "agent_opt.th", "critic_opt.th"} | (
            {"rew_ms.th"} if learner.rew_ms is not None else set())
        _, buf2, _, fresh, _ = build_ppo(c)
        fresh.load_models(str(d))
        assert fresh._opt_steps == learner._opt_steps == 3
        fresh._tcritic.copy_(learner._tcritic)   # not saved: the target restarts from the critic
        learner.train(sample(buf, c), 2000, 8)
        fresh.train(sample(buf2, c), 2000, 8)
        a, b = all_buffers(learner), all_buffers(fresh)
        for k in a:   # the gradient buffers too: not saved, but the step overwrites them whole
            assert np.array_equal(a[k], b[k]), (row, k)
        assert np.array_equal(learner._estats.cpu().numpy(), fresh._estats.cpu().numpy())
        assert fresh._opt_steps == 6


@pytest.mark.parametrize("row,critic", [("default", "cv_critic"), ("part_ac", "ac_critic")])
def test_mappo_and_ippo_keys_train(row, critic):
    """epymarl's mappo.yaml (cv_critic) and ippo.yaml (ac_critic) keys construct and train, on a row whose weights have
    that critic's shapes: four epochs, nothing cut at eps_clip 0.2, one soft target update, rewards standardised
    once."""
    c = PR.PPOCase(row)
    assert c.keys["critic_type"] == critic
    args, buf, mac, learner, logger = build_ppo(c, epochs=4, eps_clip=0.2, q_nstep=5, entropy_coef=0.001,
                                                optimizer="adam", add_value_last_step=True, mask_before_softmax=True,
                                                target_update_interval_or_tau=0.01, standardise_rewards=True)
    tgt = learner._tcritic.cpu().clone()
    for k in range(2):
        learner.train(sample(buf, c), 1000 * (k + 1), 8 * k)
        st = learner.last_stats()
        assert all(np.isfinite(st[s]) for s in R.STATS) and st["clip_frac"] == 0.0 and len(st["epochs"]) == 4
        tgt = tgt * (1.0 - 0.01) + learner._critic.cpu() * 0.01
        assert th.equal(learner._tcritic.cpu(), tgt)
    assert counters(learner)[:3] == (8, 8.0, 2)
    assert abs(learner.reward_stats()["count"] - (R.REW_MS_INIT[2] + 2 * c.batch()["reward"][:, :-1].size)) < 1e-9
    assert all(np.isfinite(v).all() for v in all_buffers(learner).values())
