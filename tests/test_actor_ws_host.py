"""The policy-gradient actor's buffers must cover what any step's plan asks of them (a short one shows only as silent
corruption on the device, as tests/test_workspace_host.py says of the Q learner's). Both sides are pure functions
(pymarl_amd/csrc/actor_plan.hpp: actor_ws_rows, actor_plan, actor_reduce_plan; learner_layout.hpp for the agent handle's
own buffers), so tests/host/actor_ws_probe.cpp compares them without a GPU: every slab buffer, the policy kernel's
arrays, red_tmp and norm_part are at least what the plan needs, every region of the reduction plan lies inside the
buffer it starts in, and the norm partials fit kNormPartMax.

The shapes: every row of tests/a2c_ref.ROWS and tests/a2c_ffn_ref.ROWS, the two golden COMA shapes of
scripts/coma_state_digest.py and bench.py's cfg5 (MMM2), each with both agent kinds; each once with the handle sized for
exactly the batch and once with a larger, odd max_batch / max_seq; the `split` row also under MQ_PLAN
ffn_actor_blocks=1 and =3.
"""
import json
import os
import shutil
import subprocess

import pytest

from tests import a2c_ffn_ref, a2c_ref
from tests.golden_utils import ComaCase
from tests.test_plan_host import HIPCC, ROOT

NEED = ("agent.slab_fc1", "agent.slab_rnn", "slab_fc2", "slab_ffn", "ppart", "dL", "dHo", "pi", "red_tmp", "norm_part")
KINDS = (("gru", 0), ("ffn", 1))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc to build tests/host/actor_ws_probe.cpp with")
    exe = str(tmp_path_factory.mktemp("actor_ws_probe") / "actor_ws_probe")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1",
                    os.path.join(ROOT, "tests", "host", "actor_ws_probe.cpp"), "-o", exe], check=True)
    return exe


def shapes():
    """name -> (n, A, O, S, obs_last_action, B, t_len)"""
    out = {}
    for prefix, rows in (("a2c_", a2c_ref.ROWS), ("a2c_ffn_", a2c_ffn_ref.ROWS)):
        for row, d in rows.items():
            last = dict(a2c_ref.DEFAULTS, **d.get("over", {}))["obs_last_action"]
            out[prefix + row] = (d["n"], d["A"], d["O"], d["S"], int(bool(last)), d["B"], d["t_len"])
    for name in ("coma_tiny_masked", "coma_cfg5"):
        c = ComaCase(name)
        out[name] = (c.n, c.A, c.O, c.S, 1, c.B, c.T + 1)
    out["bench_cfg5"] = (10, 18, 176, 322, 1, 8, 181)   # bench.py CONFIGS["cfg5"]: T = 180, B = 8
    return out


# (id, shape, agent, exact, MQ_PLAN)
CASES = [("{}-{}-{}".format(name, kind, "exact" if exact else "larger"), s, agent, exact, None)
         for name, s in shapes().items() for kind, agent in KINDS for exact in (True, False)]
CASES += [("a2c_ffn_split-ffn-{}-blocks{}".format("exact" if exact else "larger", k), shapes()["a2c_ffn_split"], 1,
           exact, "ffn_actor_blocks={}".format(k)) for k in (1, 3) for exact in (True, False)]
RESULTS = {}


def run_probe(probe, case, *overrides):
    cid, (n, A, O, S, last, B, t_len), agent, exact, plan = case
    env = {k: v for k, v in os.environ.items() if k not in ("MQ_PLAN", "MQ_DIAG")}
    if plan:
        env["MQ_PLAN"] = plan
    max_B, max_t = (B, t_len) if exact else (2 * B + 1, 2 * t_len + 1)
    argv = [n, A, O, S, last, 1, agent, B, t_len, max_B, max_t]
    out = subprocess.run([probe] + [str(a) for a in argv] + list(overrides), env=env, check=True, capture_output=True,
                         text=True)
    return json.loads(out.stdout)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_actor_buffers_cover_the_plan(probe, case):
    r = RESULTS[case[0]] = run_probe(probe, case)
    for buf in NEED:
        print(case[0], buf, "need", r["need"][buf], "size", r["size"][buf])
        assert r["need"][buf] <= r["size"][buf], (case[0], buf, r["need"][buf], r["size"][buf])
    assert r["regions_inside"], (case[0], r)
    assert r["need"]["norm_part"] <= r["norm_part_max"] == r["size"]["norm_part"], (case[0], r)
    assert r["regions"] >= 3 and r["need"]["red_tmp"] > 0, (case[0], r)


def test_the_cases_reach_every_path(probe):
    """No case above passes for want of work: split-K in both weight gradients, several feed-forward slabs, a partial
    last tile, and workgroups that walk more than one tile."""
    rs = [RESULTS.get(c[0]) or run_probe(probe, c) for c in CASES]
    plans = [r["plan"] for r in rs]
    assert any(p["ns_w1"] >= 2 for p in plans)
    assert any(p["ns_w2"] >= 2 for p in plans)
    assert any(p["ffn_blocks"] >= 2 for p in plans)
    assert any(p["ffn_tiles"] and p["rows"] % 64 for p in plans)
    assert any(p["ffn_tpb"] >= 2 for p in plans)


def test_the_probe_sees_a_short_buffer(probe):
    case = next(c for c in CASES if c[0] == "a2c_ffn_split-ffn-exact")
    r = run_probe(probe, case)
    assert r["regions_inside"]
    for buf in ("red_tmp", "slab_ffn"):
        short = run_probe(probe, case, "{}={}".format(buf, r["need"][buf] - 1))
        assert short["size"][buf] == r["need"][buf] - 1 and not short["regions_inside"], (buf, short)
        assert run_probe(probe, case, "{}={}".format(buf, r["need"][buf]))["regions_inside"], buf
