"""The feed-forward actor at hidden width 128 (hidden_dim: 128) of ActorCriticLearner and PPOLearner on
the GPU against tests/a2c_ref.py / tests/ppo_ref.py on tests/a2c_w128_ref.py's cases, under tests/test_gpu_a2c_ffn.py's
procedure and gates (imported, not set anew); each row's edge is asserted from last_plan()."""
import numpy as np
import pytest
import torch as th

from tests import a2c_ffn_ref as F
from tests import a2c_ref as R
from tests import a2c_w128_ref as W
from tests import gpu_helpers as G
from tests import ppo_ref as PR
from tests.a2c_helpers import all_buffers, build_a2c, learner_state
from tests.ffn_ref import RefFFAgent
from tests.ppo_helpers import build_a2c_on, build_ppo
from tests.test_gpu_a2c import sample
from tests.test_gpu_a2c_ffn import gates

pytestmark = pytest.mark.gpu
# row -> (rows, 32-row backward tiles, workgroups, tiles per workgroup, actions, I); walk/4: they walk 8, 8, 8 and 6 tiles
EDGES = {"part": (18, 1, 1, 1, 5, 13), "tile32": (32, 1, 1, 1, 5, 12), "tile33": (33, 2, 2, 1, 5, 11),
         "tile64": (64, 2, 2, 1, 5, 12), "tile65": (65, 3, 3, 1, 5, 11), "walk": (960, 30, 30, 1, 5, 13),
         "walk/4": (960, 30, 4, 8, 5, 13), "A33": (54, 2, 2, 1, 33, 41), "A64": (54, 2, 2, 1, 64, 72),
         "wideI": (54, 2, 2, 1, 5, 68), "n10": (60, 2, 2, 1, 18, 33)}


def edge(p, c):
    return (p["rows"], p["ffn_tiles"], p["ffn_blocks"], p["ffn_tiles_per_block"], p["policy_lanes"], c.I)


@pytest.mark.parametrize("row,plan_env", [(r, None) for r in W.ROWS] + [("walk", "ffn_actor_blocks=4")])
def test_a2c_w128_vs_ref(row, plan_env, monkeypatch):
    if plan_env:   # read once per handle, at the first train()
        monkeypatch.setenv("MQ_PLAN", plan_env)
    c = W.A2CW128Case(row)
    args, buf, mac, learner, logger = build_a2c(c, **W.KEYS)
    assert mac.agent.hidden_dim == 128 and learner.critic.hidden_dim == 128
    nb, bad = c.batch(), []
    for k in range(2):   # the second step from the GPU's own state
        batch = sample(buf, c)
        state = learner_state(learner)
        r64, r32 = R.a2c_ref_step(c, state, nb, R.F64), R.a2c_ref_step(c, state, nb, R.F32)
        kinks = F.kinks(c, state, nb, r64)
        assert min(kinks.values()) > R.MARGIN, (row, k, kinks)
        learner.train(batch, 1000 * (k + 1), 8 * k)
        plan = learner.last_plan()
        assert plan["ffn_fwd_lds"] == 162816 and edge(plan, c) == EDGES[row + "/4" if plan_env else row], (row, plan)
        bad += gates(c, (row, plan_env, k), learner, state, r64, r32, nb, plan, learner.last_stats(), r64.Vt)[1]
        assert learner._opt_steps == k + 1
    assert not bad, bad


@pytest.mark.parametrize("row", list(W.PPO_SEEDS))
def test_ppo_w128_epochs_vs_ref(row):
    """§3l's procedure: a fresh learner with `epochs: k` is judged on epoch k, from the previous build's read-back."""
    c = W.PPOW128Case(row)
    nb, bad, state, first = c.batch(), [], None, None
    for k in range(1, c.epochs + 1):
        args, buf, mac, learner, logger = build_ppo(c, epochs=k, **W.KEYS)
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
    assert not bad and c.epochs == 4, bad


def test_ppo_one_epoch_is_the_actor_critic_learner_bitwise():
    """§3l's `epochs: 1` gate at width 128: every buffer but pg_loss's one word."""
    c = W.PPOW128Case("part")
    _, buf, _, ppo, _ = build_ppo(c, epochs=1, **W.KEYS)
    _, abuf, _, a2c, _ = build_a2c_on(c, **W.KEYS)
    ppo.train(sample(buf, c), 1000, 0)
    a2c.train(sample(abuf, c), 1000, 0)
    a, b = all_buffers(ppo), all_buffers(a2c)
    keep = np.arange(a["_agrad"].size) != ppo.n_agent_params
    a["_agrad"], b["_agrad"] = a["_agrad"][keep], b["_agrad"][keep]
    assert set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_two_runs_bitwise_equal():
    c, runs = W.A2CW128Case("walk"), []
    for _ in range(2):
        args, buf, mac, learner, logger = build_a2c(c, **W.KEYS)
        for k in range(2):
            learner.train(sample(buf, c), 1000 * (k + 1), 8 * k)
        runs.append(dict(all_buffers(learner), stats=learner._stats.cpu().numpy().copy()))
    assert all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0])


@pytest.mark.parametrize("route", ["inline_ids", "device", "host_resident"])
def test_basic_mac_acting_and_checkpoint(route, tmp_path):
    """BasicMAC.forward at t = 0, t = 1 and a padded step (episode 1 is over) against the float64 module on the three
    replay routes; an agent.th written by that plain-torch module loads bit-equal, and the learner's checkpoint
    round-trips with the optimiser state."""
    c = W.A2CW128Case("part")
    args, buf, mac, learner, logger = build_a2c(c, **W.KEYS)
    ref = RefFFAgent(c.I, c.A, 128)
    ref.load_state_dict({k: th.from_numpy(v) for k, v in c.agent_params.items()})
    ref = ref.double()
    host = route == "host_resident"
    if host:   # the reference ParallelRunner's batch under buffer_cpu_only
        buf = G.ReplayBuffer(G.make_scheme(c), {"agents": c.n}, c.n_episodes, c.T + 1, device="cpu",
                             preprocess={"actions": ("actions_onehot", [G.OneHot(out_dim=c.A)])})
        buf.load_arrays(c.data)
    batch = sample(buf, c) if route == "inline_ids" else buf[0:c.B]
    batch = seen = batch[:, :batch.max_t_filled()]
    mac.init_hidden(c.B)
    oh = (batch["actions_onehot"] * batch["filled"].unsqueeze(-1)).double().cpu()
    eye = th.eye(c.n, dtype=th.float64).expand(c.B, c.n, c.n)
    for t in (0, 1, batch.max_seq_length - 1):
        out = mac.forward(seen, t, test_mode=False)
        avail = batch["avail_actions"][:, t].cpu()
        last = th.zeros_like(oh[:, 0]) if t == 0 else oh[:, t - 1]
        with th.no_grad():
            lg, h = ref(th.cat([batch["obs"][:, t].double().cpu(), last, eye], -1))
        pi = th.softmax(lg.masked_fill(avail == 0, -1e10), -1)
        assert out.device.type == ("cpu" if host else "cuda") and mac.hidden_states.shape == (c.B, c.n, 128)
        assert (out.double().cpu() - pi)[avail.sum(-1) > 0].abs().max().item() <= 1e-6, t
        assert (mac.hidden_states.double().cpu() - h).abs().max().item() <= 1e-5, t
    if route != "inline_ids":
        return
    learner.train(batch, 1000, 0)
    learner.save_models(str(tmp_path))
    _, _, mac2, other, _ = build_a2c(W.A2CW128Case("part", seed=5), **W.KEYS)
    other.load_models(str(tmp_path))
    a, b = all_buffers(learner), all_buffers(other)
    assert other._opt_steps == 1 and all(np.array_equal(a[k], b[k]) for k in a if k not in ("_tcritic", "_agrad", "_cgrad"))
    th.save(ref.float().state_dict(), str(tmp_path / "agent.th"))
    mac2.load_models(str(tmp_path))
    assert np.array_equal(mac2.agent.flat_params().cpu().numpy(), np.concatenate([v.ravel() for v in c.agent_params.values()]))
