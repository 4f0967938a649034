"""The non-shared actor (agent: rnn_ns, mac: non_shared_mac) of ActorCriticLearner and PPOLearner on the
GPU against tests/a2c_ns_ref.py, under tests/test_gpu_a2c_ffn.py's procedure and gates with a block per agent and
tensor; each row's edge is asserted from last_plan()."""
import numpy as np
import pytest
import torch as th

from tests import a2c_ffn_ref as F
from tests import a2c_ns_ref as N
from tests import a2c_ref as R
from tests import ppo_ref as PR
from tests.a2c_helpers import all_buffers, build_a2c, learner_state
from tests.gpu_helpers import rel
from tests.test_gpu_a2c import rewards32, sample

pytestmark = pytest.mark.gpu
STREAMED = 5 * 64 * 68 * 4
per_agent = lambda p: (p["ns_tiles_per_agent"], p["ns_blocks_per_agent"], p["ffn_tiles_per_block"])   # noqa: E731
EDGES = {
    "ns_part": lambda p, c: p["rows"] == 54 and per_agent(p) == (1, 1, 1) and p["ffn_tiles"] == 3,
    "ns_tile64": lambda p, c: p["rows"] == 128 and per_agent(p) == (1, 1, 1),
    "ns_tile65": lambda p, c: p["rows"] == 130 and per_agent(p) == (2, 2, 1) and p["ns_slices_per_agent"] == 2,
    "ns_walk": lambda p, c: p["rows"] == 960 and per_agent(p) == (5, 5, 1) and p["ffn_blocks"] == 15,
    "ns_walk/6": lambda p, c: per_agent(p) == (5, 2, 3) and p["ffn_blocks"] == 6 and p["ns_slices_per_agent"] == 2,
    "ns_n10": lambda p, c: c.n == 10 and p["policy_lanes"] == 18 and p["ffn_blocks"] == 10,
    "ns_A33": lambda p, c: p["policy_lanes"] == 33 and p["ap"] == 36,
    "ns_wideI": lambda p, c: c.I == 264 and p["ffn_fwd_lds"] == STREAMED,
}


def gates(c, tag, learner, state, r64, r32, nb, plan, st, Vt64):
    """tests/test_gpu_a2c_ffn.py's gates 2-4 on one train() from `state`; returns the state after and the misses."""
    assert plan["agent"] == 2 and plan["bwd_blocks"] == plan["ffn_blocks"] == c.n * plan["ns_blocks_per_agent"], plan
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


@pytest.mark.parametrize("row,plan_env", [(r, None) for r in N.ROWS] + [("ns_walk", "ffn_actor_blocks=6")])
def test_a2c_ns_vs_ref(row, plan_env, monkeypatch):
    if plan_env:   # read once per handle, at the first train()
        monkeypatch.setenv("MQ_PLAN", plan_env)
    c = N.A2CNSCase(row)
    args, buf, mac, learner = N.build_ns(c)
    nb, bad = c.batch(), []
    with N.non_shared():
        for k in range(2):   # the second step from the GPU's own state
            batch = sample(buf, c)
            state = learner_state(learner)
            r64, r32 = R.a2c_ref_step(c, state, nb, R.F64), R.a2c_ref_step(c, state, nb, R.F32)
            kinks = F.kinks(c, state, nb, r64)
            assert min(kinks.values()) > R.MARGIN, (row, k, kinks)
            learner.train(batch, 1000 * (k + 1), 8 * k)
            plan = learner.last_plan()
            assert EDGES[row + "/6" if plan_env else row](plan, c), (row, plan)
            bad += gates(c, (row, plan_env, k), learner, state, r64, r32, nb, plan, learner.last_stats(), r64.Vt)[1]
            assert learner._opt_steps == k + 1
    assert not bad, bad


@pytest.mark.parametrize("row", list(N.PPO_SEEDS))
def test_ppo_ns_epochs_vs_ref(row):
    """§3l's procedure: a fresh learner with `epochs: k` is judged on epoch k, from the previous build's read-back."""
    c = N.PPONSCase(row)
    nb, bad, state, first = c.batch(), [], None, None
    with N.non_shared():
        for k in range(1, c.epochs + 1):
            args, buf, mac, learner = N.build_ns(c, "ppo_learner", epochs=k)
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
            assert last["clipped"] == r64.clipped == r32.clipped, (row, k, last["clipped"], r64.clipped)
    assert not bad and c.epochs == 4, bad


def test_ppo_one_epoch_is_the_actor_critic_learner_bitwise():
    """§3l's `epochs: 1` gate: every buffer but pg_loss's one word."""
    c = N.PPONSCase("ns_part")
    _, buf, _, ppo = N.build_ns(c, "ppo_learner", epochs=1)
    _, abuf, _, a2c = N.build_ns(c)
    ppo.train(sample(buf, c), 1000, 0)
    a2c.train(sample(abuf, c), 1000, 0)
    a, b = all_buffers(ppo), all_buffers(a2c)
    keep = np.arange(a["_agrad"].size) != ppo.n_agent_params
    a["_agrad"], b["_agrad"] = a["_agrad"][keep], b["_agrad"][keep]
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


def _pi_dl(learner, buf, c):
    learner.train(sample(buf, c), 1000, 0)
    return [learner.last_intermediate(i).cpu().numpy() for i in (3, 4)]


def test_identical_weights_are_the_shared_actor_bitwise():
    """All n agents loaded with the shared agent's weights: pi and dLoss/dlogits of a train() equal the shared
    use_rnn: False actor's bit for bit, though every row sits in another tile (two tiles per agent here)."""
    c, cs = N.A2CNSCase("ns_tile65"), N.A2CNSCase("ns_tile65")
    F._ff(cs)
    _, sbuf, _, shared, _ = build_a2c(cs, use_rnn=False)
    _, buf, mac, learner = N.build_ns(c)
    mac.agent.load_state_dict({"agents.{}.{}".format(g, k): th.from_numpy(v) for g in range(c.n)
                               for k, v in cs.agent_params.items()})
    for a, b in zip(_pi_dl(learner, buf, c), _pi_dl(shared, sbuf, cs)):
        assert a.shape == b.shape and np.array_equal(a, b)


def test_permuting_two_agents_changes_exactly_their_rows():
    c = N.A2CNSCase("ns_part")
    _, buf, _, one = N.build_ns(c)
    _, buf2, mac2, two = N.build_ns(c)
    swap = {0: 2, 2: 0, 1: 1}
    mac2.agent.load_state_dict({k: th.from_numpy(c.agent_params["agents.{}.{}".format(swap[int(k.split(".")[1])],
                                                                                      k.split(".", 2)[2])])
                                for k in c.agent_params})
    pi1, pi2 = _pi_dl(one, buf, c)[0], _pi_dl(two, buf2, c)[0]   # (B, T, n, A)
    assert np.array_equal(pi1[:, :, 1], pi2[:, :, 1])
    assert all((pi1[:, :, g] != pi2[:, :, g]).any() for g in (0, 2))


def test_two_runs_bitwise_equal():
    c, runs = N.A2CNSCase("ns_walk"), []
    for _ in range(2):
        args, buf, mac, learner = N.build_ns(c)
        for k in range(2):
            learner.train(sample(buf, c), 1000 * (k + 1), 8 * k)
        runs.append(dict(all_buffers(learner), stats=learner._stats.cpu().numpy().copy()))
    assert all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0])


def test_non_shared_mac_acting_and_checkpoint(tmp_path):
    """NonSharedMAC.forward against the float64 ModuleList (obs_last_action and obs_agent_id on); an agent.th written by
    that plain-torch module loads bit-equal, and the learner's checkpoint round-trips."""
    c = N.A2CNSCase("ns_part")
    args, buf, mac, learner = N.build_ns(c)
    ref = N.RefNSAgent(c.n, c.I, c.A)
    ref.load_state_dict({k: th.from_numpy(v) for k, v in c.agent_params.items()})
    ref = ref.double()
    batch = sample(buf, c)
    mac.init_hidden(c.B)
    oh = (batch["actions_onehot"] * batch["filled"].unsqueeze(-1)).double().cpu()
    eye = th.eye(c.n, dtype=th.float64).expand(c.B, c.n, c.n)
    for t in (0, 1, batch.max_seq_length - 1):
        out = mac.forward(batch, t, test_mode=False)
        avail = batch["avail_actions"][:, t].cpu()
        last = th.zeros_like(oh[:, 0]) if t == 0 else oh[:, t - 1]
        with th.no_grad():
            lg, h = ref(th.cat([batch["obs"][:, t].double().cpu(), last, eye], -1))[:2]
        pi = th.softmax(lg.masked_fill(avail == 0, -1e10), -1)
        assert (out.double().cpu() - pi)[avail.sum(-1) > 0].abs().max().item() <= 1e-6, t
        assert (mac.hidden_states.double().cpu() - h).abs().max().item() <= 1e-5, t
    learner.train(batch, 1000, 0)
    learner.save_models(str(tmp_path))
    _, _, mac2, other = N.build_ns(N.A2CNSCase("ns_part", seed=5))
    other.load_models(str(tmp_path))
    a, b = all_buffers(learner), all_buffers(other)
    assert all(np.array_equal(a[k], b[k]) for k in a if k not in ("_tcritic", "_agrad", "_cgrad"))
    th.save(ref.float().state_dict(), str(tmp_path / "agent.th"))
    mac2.load_models(str(tmp_path))
    flat = np.concatenate([v.ravel() for v in c.agent_params.values()])
    assert np.array_equal(mac2.agent.flat_params().cpu().numpy(), flat)
