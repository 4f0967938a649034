"""The feed-forward actor at width 128 (hidden_dim: 128) without a GPU: epymarl's args are accepted by
both learners, every other agent and learner refuses the width with a ValueError that names its key, ma_create refuses
it before any HIP call, the seeds of tests/a2c_w128_ref.py's rows hold, and tests/host/actor_w128_probe.cpp shows the
plan, slabs, workspace rows and LDS bytes inside what ma_create allocates over every batch up to the handle's."""
import ctypes
import json
import os
import shutil
import subprocess
from types import SimpleNamespace as SN

import pytest

from pymarl_amd import _lib
from pymarl_amd.learners import REGISTRY as le_REGISTRY
from pymarl_amd.learners.actor_critic_learner import make_a2c_config
from tests import a2c_ffn_ref as F
from tests import a2c_ref as R
from tests import a2c_w128_ref as W
from tests.a2c_helpers import build_a2c, make_a2c_args
from tests.ffn_ref import ff_agent_shapes
from tests.ppo_helpers import build_ppo
from tests.test_plan_host import HIPCC, ROOT

BUILD = {"actor_critic_learner": (build_a2c, W.A2CW128Case), "ppo_learner": (build_ppo, W.PPOW128Case)}


@pytest.mark.parametrize("name", list(BUILD))
def test_epymarl_args_are_accepted(name):
    build, case = BUILD[name]
    c = case("part")
    args, _, mac, learner, _ = build(c, device="cpu", **W.KEYS)
    assert args.rnn_hidden_dim is None and args.hidden_dim == 128 and type(learner) is le_REGISTRY[name]
    assert mac.agent.hidden_dim == 128 and not mac.agent.use_rnn
    assert list(mac.agent.state_dict()) == list(ff_agent_shapes(c.I, c.A, 128))
    assert learner.n_agent_params == sum(p.numel() for p in mac.agent.parameters()) == 128 * (c.I + 1 + 129) + 129 * c.A
    cfg = make_a2c_config(args, learner.cfg, mac.agent.input_dim, learner.critic, c.B, c.T + 1, learner._gpow)
    assert (cfg.rnn_hidden_dim, cfg.critic_hidden, cfg.agent) == (128, 128, _lib.AGENT_FFN)
    assert build(c, device="cpu", use_rnn=False, rnn_hidden_dim=128)[2].agent.hidden_dim == 128   # the explicit key


@pytest.mark.parametrize("learner,over,key", [
    ("actor_critic_learner", dict(rnn_hidden_dim=None), "hidden_dim"),                     # the GRU agent at 128
    ("ppo_learner", dict(rnn_hidden_dim=128, epochs=4, eps_clip=0.2), "rnn_hidden_dim"),
    ("actor_critic_learner", dict(W.KEYS, agent="rnn_ns", mac="non_shared_mac"), "hidden_dim"),
    ("coma_learner", dict(rnn_hidden_dim=128, optimizer="rmsprop"), "rnn_hidden_dim"),
    ("q_learner", dict(rnn_hidden_dim=128, mixer="vdn", optimizer="rmsprop"), "rnn_hidden_dim"),
    ("q_learner", dict(W.KEYS, mixer=None, optimizer="rmsprop"), "hidden_dim"),
])
def test_refusals_name_their_key(learner, over, key):
    """Before any library call: the learner is given no MAC, scheme or logger to get further with."""
    args = make_a2c_args(W.A2CW128Case("part"), learner=learner, **over)
    with pytest.raises(ValueError, match=r"^{}: 128 ".format(key)):
        le_REGISTRY[learner](SN(agent=SN(use_rnn=getattr(args, "use_rnn", True))), None, None, args)


@pytest.mark.parametrize("agent,hidden", [(_lib.AGENT_GRU, 128), (_lib.AGENT_FFN_NS, 128), (_lib.AGENT_FFN, 96)])
def test_ma_create_refuses_before_any_hip_call(agent, hidden):
    lib = _lib.load()
    gpow = (ctypes.c_float * 7)(*[0.99 ** k for k in range(7)])
    cfg = _lib.MAConfig(n_agents=3, n_actions=5, obs_dim=5, state_dim=7, rnn_hidden_dim=hidden, critic_hidden=128,
                        critic_type=_lib.MA_CRITIC_CV, obs_last_action=1, obs_agent_id=1, q_nstep=5, lr=5e-4,
                        gamma_pow=ctypes.cast(gpow, ctypes.c_void_p), max_batch=2, max_seq=4, agent=agent)
    h = ctypes.c_void_p()
    assert lib.ma_create(ctypes.byref(cfg), ctypes.byref(h)) != 0 and not h.value
    assert b"rnn_hidden_dim" in lib.mq_last_error()


@pytest.mark.parametrize("row", list(W.ROWS) + ["ppo_" + r for r in W.PPO_SEEDS])
def test_seed_conditions(row):
    ppo = row.startswith("ppo_")
    c = W.PPOW128Case(row[4:]) if ppo else W.A2CW128Case(row)
    assert F.seed_minimum(c, ppo) > R.MARGIN, row


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc to build tests/host/actor_w128_probe.cpp with")
    exe = str(tmp_path_factory.mktemp("actor_w128_probe") / "actor_w128_probe")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1",
                    os.path.join(ROOT, "tests", "host", "actor_w128_probe.cpp"), "-o", exe], check=True)
    return exe


SHAPES = {row: (d["n"], d["A"], d["O"], d["S"], 1, d["B"], d["t_len"]) for row, d in W.ROWS.items()}
SHAPES["bench_cfg5"] = (10, 18, 176, 322, 1, 8, 181)   # bench.py CONFIGS["cfg5"]: T = 180, B = 8
PROBES = [(name, s, exact, plan) for name, s in SHAPES.items() for exact in (True, False) for plan in (None,)]
PROBES += [("walk", SHAPES["walk"], exact, "ffn_actor_blocks=4") for exact in (True, False)]


@pytest.mark.parametrize("name,shape,exact,plan", PROBES,
                         ids=["{}-{}{}".format(p[0], "exact" if p[2] else "larger", "-capped" if p[3] else "") for p in PROBES])
def test_handle_covers_every_batch(probe, name, shape, exact, plan):
    n, A, O, S, last, B, t_len = shape
    env = {k: v for k, v in os.environ.items() if k not in ("MQ_PLAN", "MQ_DIAG")}
    if plan:
        env["MQ_PLAN"] = plan
    max_B, max_t = (B, t_len) if exact else (2 * B + 1, 2 * t_len + 1)
    out = subprocess.run([probe] + [str(a) for a in (n, A, O, S, last, max_B, max_t, t_len)], env=env, check=True,
                         capture_output=True, text=True)
    r = json.loads(out.stdout)
    print(name, r)
    assert r["fwd_lds"] == 162816 and r["bwd_lds"] == 160768 and max(r["fwd_lds"], r["bwd_lds"]) <= r["lds_max"] == 163840
    for buf, need in r["need"].items():
        assert 0 < need <= r["size"][buf], (name, buf, need, r["size"][buf])
    assert r["regions_inside"] and r["slices_non_empty"] and r["norm_part"] <= r["norm_part_max"], (name, r)
    assert r["len_rnn"] == 128 * 128 + 128 + A * 128 + A and r["P"] == 128 * (O + A + n) + 128 + r["len_rnn"]
    if name == "walk":   # the largest batch's plan: capped workgroups walk several tiles, uncapped ones a tile each
        assert (r["ffn_blocks"] == 4 and r["ffn_tpb"] >= 8) if plan else (r["ffn_blocks"] >= 30 and r["ffn_tpb"] == 1)
