"""The non-shared actor (agent: rnn_ns, mac: non_shared_mac) without a GPU: the registry keys, epymarl's
state_dict names, the refusals, the seeds of tests/a2c_ns_ref.py's rows, and the grouped plan against what ma_create
allocates (tests/host/actor_ns_probe.cpp)."""
import json
import os
import shutil
import subprocess

import pytest

from pymarl_amd import _lib
from pymarl_amd.controllers import REGISTRY as mac_REGISTRY
from pymarl_amd.learners import REGISTRY as le_REGISTRY
from pymarl_amd.learners.actor_critic_learner import make_a2c_config
from pymarl_amd.modules.agents import REGISTRY as agent_REGISTRY
from tests import a2c_ns_ref as N
from tests import a2c_ref as R
from tests.ffn_ref import ff_agent_shapes
from tests.test_plan_host import HIPCC, ROOT

STREAMED = 5 * 64 * 68 * 4
# row -> what the plan of its step must show (and MQ_PLAN for it)
PLANS = {
    "ns_part": (None, dict(tpa=1, bpa=1, tpb=1, slices=1, ffn_tiles=3, ffn_blocks=3)),
    "ns_tile64": (None, dict(tpa=1, bpa=1, ffn_tiles=2)),
    "ns_tile65": (None, dict(tpa=2, bpa=2, tpb=1, slices=2, ffn_blocks=4)),
    "ns_walk": (None, dict(tpa=5, bpa=5, tpb=1, slices=5, ffn_tiles=15, ffn_blocks=15)),
    "ns_walk/6": ("ffn_actor_blocks=6", dict(tpa=5, bpa=2, tpb=3, slices=2, ffn_blocks=6)),
    "ns_n10": (None, dict(tpa=1, bpa=1, ffn_tiles=10, ffn_blocks=10)),
    "ns_A33": (None, dict(tpa=1, resident=1)),
    "ns_wideI": (None, dict(tpa=1, resident=0, fwd_lds=STREAMED)),
    "cfg5": (None, dict(tpa=23, bpa=23, tpb=1, ffn_blocks=230)),   # bench.py's cfg5: n 10, B 8, T 180
}
CFG5 = dict(n=10, A=18, O=176, S=322, B=8, t_len=181)


@pytest.mark.parametrize("learner", ["actor_critic_learner", "ppo_learner"])
def test_keys_names_and_layout(learner):
    assert agent_REGISTRY["rnn_ns"].__name__ == "RNNNSAgent" and mac_REGISTRY["non_shared_mac"].__name__ == "NonSharedMAC"
    c = N.A2CNSCase("ns_part") if learner == "actor_critic_learner" else N.PPONSCase("ns_part")
    args, _, mac, made = N.build_ns(c, learner, device="cpu")
    names = ["agents.{}.{}".format(g, k) for g in range(c.n) for k in ff_agent_shapes(c.I, c.A)]
    assert list(mac.agent.state_dict()) == names == [k for k, _ in mac.agent.named_parameters()] == list(c.agent_shapes)
    assert made.n_agent_params == sum(a.size for a in c.agent_params.values()) and made.non_shared
    cfg = make_a2c_config(args, made.cfg, mac.agent.input_dim, made.critic, c.B, c.T + 1, made._gpow)
    assert cfg.agent == _lib.AGENT_FFN_NS == 2 and _lib.MAConfig._fields_[-1][0] == "agent"
    assert [k for k, _ in _lib.MAActor._fields_][-3:] == ["ns_tiles_per_agent", "ns_blocks_per_agent",
                                                          "ns_slices_per_agent"]


@pytest.mark.parametrize("over,match", [
    (dict(use_rnn=True), "use_rnn"), (dict(use_rnn=None), "use_rnn"),      # the non-shared GRU actor is not built
    (dict(agent="rnn"), "agent"), (dict(mac="basic_mac"), "non_shared_mac"),
    (dict(learner="coma_learner"), "learner"), (dict(learner="q_learner"), "learner"),
    (dict(critic_type="cv_critic_ns"), "critic_type"), (dict(critic_type="ac_critic_ns"), "critic_type"),
])
def test_refusals_name_their_key(over, match):
    with pytest.raises(ValueError, match=match) as e:
        N.build_ns(N.A2CNSCase("ns_part"), device="cpu", **over)
    assert "use_rnn" not in over or "not built" in str(e.value)


def test_learner_and_mac_must_agree():
    c = N.A2CNSCase("ns_part")
    args, buf, mac, _ = N.build_ns(c, device="cpu")
    args.agent = "rnn"
    with pytest.raises(ValueError, match="agent"):
        le_REGISTRY["actor_critic_learner"](mac, buf.scheme, None, args)


@pytest.mark.parametrize("row", list(N.ROWS) + ["ppo_" + r for r in N.PPO_SEEDS])
def test_seed_conditions(row):
    ppo = row.startswith("ppo_")
    c = N.PPONSCase(row[4:]) if ppo else N.A2CNSCase(row)
    assert N.seed_minimum(c, ppo) > R.MARGIN, row


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc to build tests/host/actor_ns_probe.cpp with")
    exe = str(tmp_path_factory.mktemp("actor_ns_probe") / "actor_ns_probe")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1",
                    os.path.join(ROOT, "tests", "host", "actor_ns_probe.cpp"), "-o", exe], check=True)
    return exe


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("name", list(PLANS))
def test_grouped_plan_fits_the_handle(probe, name, exact):
    plan_env, want = PLANS[name]
    d = CFG5 if name == "cfg5" else N.ROWS[name.split("/")[0]]
    B, t_len = d["B"], d["t_len"]
    max_B, max_t = (B, t_len) if exact else (2 * B + 1, t_len + 3)
    env = {k: v for k, v in os.environ.items() if k not in ("MQ_PLAN", "MQ_DIAG")}
    if plan_env:
        env["MQ_PLAN"] = plan_env
    argv = [d["n"], d["A"], d["O"], d["S"], 1, B, t_len, max_B, max_t]
    r = json.loads(subprocess.run([probe] + [str(a) for a in argv], env=env, check=True, capture_output=True,
                                  text=True).stdout)
    print(name, exact, r)
    assert all(r["plan"][k] == v for k, v in want.items()), (name, r["plan"])
    assert r["fits"] and r["slices_ok"], (name, r)   # over every batch up to the handle's
    assert all(0 < r["need"][k] <= r["size"][k] for k in r["need"]), (name, r)
    assert r["regions"] == 2 and r["Pa"] == d["n"] * r["Pa1"] and r["plan"]["slices"] == r["plan"]["bpa"] <= r["slabs_max"]
