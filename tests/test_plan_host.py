"""Which kernels a train step runs is plan_step's answer (pymarl_amd/csrc/step_plan.hpp), a pure function of the
config, the batch shape, MQ_PLAN and the CU count: checked here without a GPU through tests/host/plan_probe.cpp.

Group A: every row of tests/test_gpu_grad_blocks.ROWS must get the plan the library reported for it before plan_step
existed (tests/golden/plans_parent.json: last_plan() of that library on an MI355X, with the CU count and each row's
t_len recorded beside it). Group B: the thresholds between plans, one shape either side, and the bench shapes; the
expected items were read from that library's code, and its last_plan() of the same shapes (the "edges" / "bench"
records of the same file) is asserted in full where a record exists (num_cu = 0 cannot be recorded on a GPU).
"""
import json
import os
import shutil
import subprocess

import pytest

from pymarl_amd import _lib
from tests import ref64
from tests.gpu_helpers import switch_value
from tests.test_gpu_grad_blocks import ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
MIXERS = {"none": _lib.MIXER_NONE, "vdn": _lib.MIXER_VDN, "qmix": _lib.MIXER_QMIX}
DWH_NAMES = ("red1", "bptt_grid")
with open(os.path.join(ROOT, "tests", "golden", "plans_parent.json")) as f:
    PARENT = json.load(f)
CUS = PARENT["multi_processor_count"]
BASE = dict(ref64.SHAPES["base"], mixer="qmix")   # n=3, A=9, O=30, S=48


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc to build tests/host/plan_probe.cpp with")
    exe = str(tmp_path_factory.mktemp("plan_probe") / "plan_probe")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1",
                    os.path.join(ROOT, "tests", "host", "plan_probe.cpp"), "-o", exe], check=True)
    return exe


def plan_of(probe, num_cu, shape, B, t_len, switches=None, E=32):
    """last_plan()'s dict for `shape` (n, A, O, S, mixer) at B episodes of t_len steps under MQ_PLAN `switches`."""
    env = {k: v for k, v in os.environ.items() if k not in ("MQ_PLAN", "MQ_DIAG")}
    for key, v in (switches or {}).items():
        var, val = switch_value(env, key, v)
        env[var] = val
    argv = [num_cu, MIXERS[shape["mixer"]], shape["n"], shape["A"], shape["O"], shape["S"], E, 1, 1, 1, B, t_len]
    out = subprocess.run([probe] + [str(a) for a in argv], env=env, check=True, capture_output=True, text=True)
    d = json.loads(out.stdout)
    d["hyper"], d["mix"], d["dwh"] = _lib.HYP_NAMES[d["hyper"]], _lib.MIX_NAMES[d["mix"]], DWH_NAMES[d["dwh"]]
    return d


@pytest.mark.parametrize("row", list(ROWS))
def test_rows_get_the_parents_plan(probe, row):
    shape, mixer, switches, want = ROWS[row]
    rec = PARENT["rows"][row]
    s = ref64.SHAPES[shape]
    plan = plan_of(probe, CUS, dict(s, mixer=mixer), s["B"], rec["t_len"], switches)
    assert plan == rec["plan"], (row, plan)
    for key, v in want.items():   # and what the GPU row itself asserts
        assert plan[key] == v, (row, key, plan)


# (id, num_cu, B, switches, expected items, the parent's record of the same shape or None)
EDGES = [
    ("r255_cu256", 256, 85, {}, dict(rows=255, fused_fwd=2, bwd_lean=1, dwh="red1"), "r255"),
    ("r258_cu256", 256, 86, {}, dict(rows=258, fused_fwd=1, hyper="ws", bwd_lean=0, dwh="bptt_grid"), "r258"),
    ("r258_cu0", 0, 86, {}, dict(rows=258, fused_fwd=1, dwh="red1"), None),
    ("b170", 256, 170, {}, dict(rows=510, tiles=0, fused_bwd=1), "b170"),
    ("b171", 256, 171, {}, dict(rows=513, tiles=1), "b171"),
    ("b171_row_tiles0", 256, 171, {"row_tiles": 0}, dict(tiles=0, fused_bwd=0, rw_bwd=2, rw_fwd=2), "b171_notiles"),
    ("lambda_path", 256, 4, {"lambda_path": 1}, dict(td_lambda=1), "lambda_path"),
    ("unfused_bwd", 256, 4, {"unfused_bwd": True}, dict(fused_fwd=2, fused_bwd=0, bwd_lean=0), "unfused_bwd"),
]


@pytest.mark.parametrize("name,num_cu,B,switches,want,rec", EDGES, ids=[e[0] for e in EDGES])
def test_edges(probe, name, num_cu, B, switches, want, rec):
    plan = plan_of(probe, num_cu, BASE, B, 6, switches)
    for key, v in want.items():
        assert plan[key] == v, (name, key, plan)
    if rec is not None:
        r = PARENT["edges"][rec]
        assert (r["B"], r["t_len"], num_cu) == (B, 6, CUS), r
        assert plan == r["plan"], (name, plan)


BENCH = {   # bench.py CONFIGS: (mixer, n, A, O, S, T, B), and the plan items at 256 CUs with t_len = T + 1
    "cfg2": (("qmix", 8, 14, 80, 168, 120, 32),
             dict(fused_fwd=2, fused_bwd=1, bwd_lean=1, hyper="ws", mix="fast16", dwh="red1")),
    "cfg4": (("qmix", 5, 11, 80, 120, 120, 64),
             dict(fused_fwd=1, fused_bwd=1, bwd_lean=0, hyper="ws", dwh="bptt_grid")),
    "cfg3": (("vdn", 27, 36, 285, 1170, 180, 128), dict(tiles=1, mix="stream")),
}


@pytest.mark.parametrize("cfg", list(BENCH))
def test_bench_shapes(probe, cfg):
    (mixer, n, A, O, S, T, B), want = BENCH[cfg]
    plan = plan_of(probe, 256, dict(n=n, A=A, O=O, S=S, mixer=mixer), B, T + 1)
    for key, v in want.items():
        assert plan[key] == v, (cfg, key, plan)
    r = PARENT["bench"][cfg]
    assert (r["t_len"], CUS) == (T + 1, 256), r
    assert plan == r["plan"], (cfg, plan)
