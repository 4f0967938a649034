"""The feed-forward actor (use_rnn: False) of ActorCriticLearner and PPOLearner on the GPU against
tests/a2c_ref.py / tests/ppo_ref.py on tests/a2c_ffn_ref.py's cases, under tests/test_gpu_a2c.py's and test_gpu_ppo.py's
procedures and gates (the project's rule, not set anew); each row's edge is asserted from ma_last_plan."""
import numpy as np
import pytest
import torch as th

from tests import a2c_ffn_ref as F
from tests import a2c_ref as R
from tests import ppo_ref as PR
from tests.a2c_helpers import all_buffers, build_a2c, learner_state
from tests.ffn_ref import RefFFAgent
from tests.gpu_helpers import rel
from tests.ppo_helpers import build_a2c_on, build_ppo
from tests.test_gpu_a2c import rewards32, sample

pytestmark = pytest.mark.gpu
FF = dict(use_rnn=False)
STREAMED = 5 * 64 * 68 * 4   # ffn_actor_fwd_kernel's LDS with W1 streamed
EDGES = {
    "one": lambda p, c: p["rows"] == 2 and p["policy_lanes"] == 2 and p["ffn_tiles"] == 1,
    "part": lambda p, c: p["rows"] == 54 and p["ffn_tiles"] == 1 and c.I == 13,
    "part_n10": lambda p, c: p["rows"] == 54 and c.I == 8 and p["reward_norm"] == 1 and p["adam"] == 0,
    "tile64": lambda p, c: p["rows"] == 64 and p["ffn_tiles"] == 1,
    "A33": lambda p, c: p["policy_lanes"] == 33 and p["ap"] == 36,
    "A64": lambda p, c: p["policy_lanes"] == 64 == p["ap"],
    "split": lambda p, c: p["rows"] == 544 and p["ffn_tiles"] == 9 == p["ffn_blocks"] and p["ns_aw1"] >= 2,
    "split/2": lambda p, c: p["ffn_tiles"] == 9 and p["ffn_blocks"] == 2 and p["ffn_tiles_per_block"] == 5,
    "wideI": lambda p, c: c.I == 264 and p["ffn_fwd_lds"] == STREAMED,
}


def gates(c, tag, learner, state, r64, r32, nb, plan, st, Vt64):
    """Gates 2-4 on one train() from `state`; returns the per-block misses."""
    assert plan["agent"] == 1 and plan["bwd_blocks"] == plan["ffn_blocks"] and plan["ns_aw2"] == 0, plan
    after = learner_state(learner)
    Pa, Pc = learner.n_agent_params, learner.n_critic_params
    agrad, cgrad = learner._agrad.detach().cpu().numpy(), learner._cgrad.detach().cpu().numpy()
    got = dict(cgrad=cgrad[:Pc], agrad=agrad[:Pa], c_v=after["c_v"], a_v=after["a_v"], c_m=after["c_m"], a_m=after["a_m"])
    assert all(np.isfinite(v).all() for v in got.values()) and cgrad[Pc + 1] == agrad[Pa + 1] == r64.M, tag
    inter = {i: learner.last_intermediate(i).cpu().numpy() for i in range(5)}
    ret32 = R.nstep_elem(inter[0], rewards32(c, nb, learner), r32.mask, c.gpow, c.keys["q_nstep"],
                         c.keys["add_value_last_step"])
    assert np.array_equal(ret32, inter[2]), tag
    rec, bad = R.judge(c, r64, r32, got)
    rec_u, bad_u = R.judge_updates(c, state, dict(agent=got["agrad"], critic=got["cgrad"]), after)
    rec.update(rec_u)
    w = R.worst(rec)
    qerr = dict(Vt=rel(inter[0], Vt64), V=rel(inter[1], r64.V), pi=rel(inter[3], r64.pi))
    nerr = (abs(st["critic_grad_norm"] - r64.critic_norm) / r64.critic_norm,
            abs(st["agent_grad_norm"] - r64.agent_norm) / r64.agent_norm)
    print(tag, "worst ratio {:.2f} at {} {}".format(w[2], w[0], w[1]), rec[w[0]][w[1]], qerr, nerr)
    assert max(qerr.values()) < 1e-5 and max(nerr) <= 1e-5, (tag, qerr, nerr)
    for s in R.STATS:
        assert abs(st[s] - r64.stats[s]) <= 1e-4 * abs(r64.stats[s]) + 1e-6, (tag, s, st[s], r64.stats[s])
    return after, [(tag,) + b for b in bad + bad_u]


@pytest.mark.parametrize("row,plan_env", [(r, None) for r in F.ROWS] + [("split", "ffn_actor_blocks=2")])
def test_a2c_ffn_vs_ref(row, plan_env, monkeypatch):
    if plan_env:   # read once per handle, at the first train()
        monkeypatch.setenv("MQ_PLAN", plan_env)
    c = F.A2CFFCase(row)
    args, buf, mac, learner, logger = build_a2c(c, **FF)
    nb, bad = c.batch(), []
    for k in range(2):   # the second step from the GPU's own state
        batch = sample(buf, c)
        state = learner_state(learner)
        r64, r32 = R.a2c_ref_step(c, state, nb, R.F64), R.a2c_ref_step(c, state, nb, R.F32)
        kinks = F.kinks(c, state, nb, r64)
        assert min(kinks.values()) > R.MARGIN, (row, k, kinks)
        learner.train(batch, 1000 * (k + 1), 8 * k)
        plan = learner.last_plan()
        assert EDGES[row + "/2" if plan_env else row](plan, c), (row, plan)
        bad += gates(c, (row, plan_env, k), learner, state, r64, r32, nb, plan, learner.last_stats(), r64.Vt)[1]
        assert learner._opt_steps == k + 1
    assert not bad, bad


@pytest.mark.parametrize("row", list(F.PPO_SEEDS))
def test_ppo_ffn_epochs_vs_ref(row):
    """A fresh learner with `epochs: k` is judged on epoch k, from the previous build's read-back."""
    c = F.PPOFFCase(row)
    nb, bad, state, first = c.batch(), [], None, None
    for k in range(1, c.epochs + 1):
        args, buf, mac, learner, logger = build_ppo(c, epochs=k, **FF)
        if k == 1:
            state = learner_state(learner)
            first = r64, r32 = [PR.ppo_ref_epoch(c, state, nb, None, None, dt) for dt in (PR.F64, PR.F32)]
        else:
            r64, r32 = [PR.ppo_ref_epoch(c, state, nb, f.old, f.ret, dt) for f, dt in zip(first, (PR.F64, PR.F32))]
        kinks = F.kinks(c, state, nb, r64)
        assert min(kinks.values()) > R.MARGIN, (row, k, kinks)
        assert min(r64.bound_dist, r32.bound_dist) > R.MARGIN and np.array_equal(r64.w[r64.live], r32.w[r32.live])
        learner.train(sample(buf, c), 1000, 0)
        plan, st = learner.last_plan(), learner.last_stats()
        assert plan["epochs"] == k and learner._opt_steps == k
        last = st["epochs"][-1]
        state, bad_k = gates(c, (row, k), learner, state, r64, r32, nb, plan, last, first[0].Vt)
        bad += bad_k
        assert last["clipped"] == r64.clipped == r32.clipped, (row, k, last["clipped"], r64.clipped)   # as integers
    assert not bad, bad
    assert last["clipped"] > 0, "the clipped branch did not run"


def test_ppo_one_epoch_is_the_actor_critic_learner_bitwise():
    """§3l's `epochs: 1` gate with the feed-forward actor: every buffer but pg_loss's one word."""
    c = F.PPOFFCase("part")
    _, buf, _, ppo, _ = build_ppo(c, epochs=1, **FF)
    _, abuf, _, a2c, _ = build_a2c_on(c, **FF)
    ppo.train(sample(buf, c), 1000, 0)
    a2c.train(sample(abuf, c), 1000, 0)
    a, b = all_buffers(ppo), all_buffers(a2c)
    keep = np.arange(a["_agrad"].size) != ppo.n_agent_params
    assert a["_agrad"][ppo.n_agent_params] != b["_agrad"][ppo.n_agent_params]
    a["_agrad"], b["_agrad"] = a["_agrad"][keep], b["_agrad"][keep]
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert all(ppo.last_stats()[s] == a2c.last_stats()[s] for s in R.STATS if s != "pg_loss")


def test_two_runs_bitwise_equal():
    c, runs = F.A2CFFCase("split"), []
    for _ in range(2):
        args, buf, mac, learner, logger = build_a2c(c, **FF)
        for k in range(2):
            learner.train(sample(buf, c), 1000 * (k + 1), 8 * k)
        runs.append(dict(all_buffers(learner), stats=learner._stats.cpu().numpy().copy()))
    assert all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0])


@pytest.mark.parametrize("mbs", [True, False])
def test_basic_mac_soft_policies(mbs):
    """tests/test_gpu_a2c.py's acting procedure with use_rnn: False: BasicMAC stepped against the float64 module."""
    c = F.A2CFFCase("part")
    args, buf, mac, learner, logger = build_a2c(c, mask_before_softmax=mbs, **FF)
    ref = RefFFAgent(c.I, c.A).double()
    ref.load_state_dict({k: th.tensor(v, dtype=th.float64) for k, v in c.agent_params.items()})
    batch = sample(buf, c)
    mac.init_hidden(c.B)
    oh = (batch["actions_onehot"] * batch["filled"].unsqueeze(-1)).double().cpu()
    eye = th.eye(c.n, dtype=th.float64).expand(c.B, c.n, c.n)
    for t in range(batch.max_seq_length):
        out = mac.forward(batch, t, test_mode=False)
        avail = batch["avail_actions"][:, t].cpu()
        rows = (avail.sum(-1) > 0) if mbs else th.ones_like(avail[..., 0], dtype=th.bool)
        last = th.zeros_like(oh[:, 0]) if t == 0 else oh[:, t - 1]
        with th.no_grad():
            lg, h = ref(th.cat([batch["obs"][:, t].double().cpu(), last, eye], -1).reshape(c.B * c.n, -1))
        lg = lg.view(c.B, c.n, c.A)
        pi = th.softmax(lg.masked_fill(avail == 0, -1e10) if mbs else lg, -1)
        assert (out.double().cpu() - pi)[rows].abs().max().item() <= 1e-6, t
        assert (mac.hidden_states.double().cpu().reshape(-1, 64) - h).abs().max().item() <= 1e-5, t
