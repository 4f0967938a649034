"""What a COMA train step launches, without a GPU: coma_plan (pymarl_amd/csrc/coma_plan.hpp) through
tests/host/coma_plan_probe.cpp, one shape either side of every threshold. Every expected number is worked out by hand
from the formulas of the step as it stood before the plan existed (mc_train_step deciding inline, coma_chain.hpp's
cc_ok, actor_forward / actor_backward); the formula stands beside each."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

CFG5 = dict(n=10, A=18, O=176, S=322, B=8, t_len=181)   # MMM2, T = 180
SMALL = dict(n=1, A=5, O=10, S=20, t_len=2)             # Kc = 20 + 10 + 2*5 + 1 = 41: NK = 1, NG = 8; T = 1, RT = R = B


def _build(tmp_path_factory, name):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc to build tests/host/{}.cpp with".format(name))
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1",
                    os.path.join(ROOT, "tests", "host", name + ".cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return _build(tmp_path_factory, "coma_plan_probe")


@pytest.fixture(scope="module")
def a2c_probe(tmp_path_factory):
    return _build(tmp_path_factory, "a2c_plan_probe")


def plan_of(probe, num_cu=256, n=1, A=5, O=10, S=20, ola=1, aid=1, B=1, t_len=2, exchange=0, replicated=0, timing=0,
            chain_enabled=1, overlap_enabled=1, shard=(0, 0)):
    argv = [num_cu, n, A, O, S, ola, aid, B, t_len, exchange, replicated, timing, chain_enabled, overlap_enabled,
            shard[0], shard[1]]
    out = subprocess.run([probe] + [str(a) for a in argv], check=True, capture_output=True, text=True).stdout
    return json.loads(out)


def test_cfg5_worked_example(probe):
    p = plan_of(probe, 256, **CFG5)
    # Kc = S + O + 2 n A + n = 322 + 176 + 360 + 10; already a multiple of 4
    assert (p["Kc"], p["Kp"], p["R"], p["T"]) == (868, 868, 80, 180)
    # NK = ceil(868 / 112), NG = 8 NK, nhead = ceil(80 / 16), KS = ceil(868 / 176),
    # nwgrad = 8 ceil(869 / 64) + 24 + 3 ceil(18 / 16) + 1 = 112 + 24 + 6 + 1
    assert (p["NK"], p["NG"], p["nhead"], p["KS"], p["nwgrad"]) == (8, 64, 5, 5, 143)
    assert (p["chain"], p["overlap"], p["refused"]) == (1, 1, "")
    # A = 18 > 16: unfused forward; R = 80 <= 512 and <= 256: one row per workgroup either way
    assert (p["fused_fwd"], p["rw_fwd"], p["rw_bwd"], p["nblk_bwd"]) == (0, 1, 1, 80)
    # RT = 14400: min(128, 14400 // 256) = 56 slices (I = 204: two dW1 tiles, cap 256), chunk = ceil(258 / 16) * 16 = 272,
    # ceil(14400 / 272) = 53
    assert (p["actor_rows"], p["ns_w1"], p["ns_w2"], p["npol"], p["qv_r0"]) == (14400, 53, 53, 3600, 0)
    # dynamic LDS: Tp (n + 3) floats; (16 + 128) rows of 177; the head's (128 + 32 + 48) 129 + 16 33 + 128 + 32; the
    # chain's carve at A16 = 32 (coma_chain.hpp CCLds: 40128 floats)
    assert (p["lds_td"], p["lds_l1"], p["lds_head"], p["lds_chain"]) == (181 * 13 * 4, 144 * 177 * 4, 27520 * 4, 40128 * 4)
    # mc_create's bounds: cpart by the heads, cnorm at least the chain's 1024, H1p max(l1 slices, chain owners)
    assert (p["ws_nhead"], p["ws_cnorm"], p["ws_h1p_slices"]) == (5, 1024, 8)
    assert p["Pc"] == 128 * 868 + 128 + 128 * 128 + 128 + 18 * 128 + 18


def test_chain_row_and_action_thresholds(probe):
    assert plan_of(probe, B=80, **SMALL)["chain"] == 1    # R = 80 = CC_MAXR
    assert plan_of(probe, B=81, **SMALL)["chain"] == 0    # R = 81
    wide = dict(SMALL, n=2, B=4)
    assert plan_of(probe, **dict(wide, A=32))["chain"] == 1
    p = plan_of(probe, **dict(wide, A=33))
    assert (p["chain"], p["overlap"]) == (0, 0)
    assert p["lds_chain"] == (40128 + 16 * 132 + 16) * 4   # A16 = 48: W3's rows and b3 grow


def test_chain_cu_count(probe):
    assert plan_of(probe, 64, **CFG5)["chain"] == 1    # 8 NK = 64 workgroups, one per CU
    p = plan_of(probe, 63, **CFG5)
    assert (p["chain"], p["overlap"]) == (0, 0)
    p = plan_of(probe, 0, **CFG5)                      # the device query failed
    assert (p["chain"], p["overlap"]) == (0, 0)
    assert plan_of(probe, 8, B=80, **SMALL)["chain"] == 1 and plan_of(probe, 7, B=80, **SMALL)["chain"] == 0


def test_fewer_owners_than_heads(probe):
    p = plan_of(probe, B=160, **SMALL)   # NG = 8 phase-A owners, ceil(160 / 16) = 10 heads
    assert (p["NG"], p["nhead"], p["chain"], p["overlap"]) == (8, 10, 0, 0)
    assert (p["ws_nhead"], p["ws_h1p_slices"]) == (10, 1)   # Kp = 44: one l1 slice, one owner


def test_modes(probe):
    assert [plan_of(probe, exchange=1, **CFG5)[k] for k in ("chain", "overlap")] == [0, 0]
    assert [plan_of(probe, timing=1, **CFG5)[k] for k in ("chain", "overlap")] == [1, 0]
    assert [plan_of(probe, chain_enabled=0, **CFG5)[k] for k in ("chain", "overlap")] == [0, 0]
    assert [plan_of(probe, overlap_enabled=0, **CFG5)[k] for k in ("chain", "overlap")] == [1, 0]
    p = plan_of(probe, replicated=1, shard=(2, 5), **CFG5)
    # the actor: 3 episodes of 10 agents over 180 steps, from row 2 * 10 of the critic's Q values
    assert (p["actor_B"], p["actor_R"], p["actor_rows"], p["qv_r0"], p["npol"]) == (3, 30, 5400, 20, 1350)
    assert (p["nblk_bwd"], p["rw_bwd"]) == (30, 1)
    # min(128, 5400 // 256) = 21 slices, chunk = ceil(258 / 16) * 16 = 272, ceil(5400 / 272) = 20
    assert (p["ns_w1"], p["ns_w2"]) == (20, 20)
    # the critic: the whole batch
    assert (p["R"], p["nhead"], p["NG"], p["chain"], p["overlap"]) == (80, 5, 64, 1, 1)


def test_refusals_keep_their_texts(probe):
    assert plan_of(probe, **dict(CFG5, t_len=3150))["refused"] == ""     # 3150 * 13 * 4 = 163800 <= 160 KiB
    assert plan_of(probe, **dict(CFG5, t_len=3151))["refused"] == "episode too long for the LDS TD(lambda) pass"


def test_actor_plan_thresholds(probe):
    few = dict(SMALL, n=2, B=4, t_len=5)   # I = 10 + A + 2 <= 112, O <= 128, R = 8
    assert plan_of(probe, **dict(few, A=16))["fused_fwd"] == 1
    assert plan_of(probe, **dict(few, A=17))["fused_fwd"] == 0
    p = plan_of(probe, B=512, **SMALL)
    assert (p["rw_fwd"], p["fused_fwd"]) == (1, 1)
    p = plan_of(probe, B=513, **SMALL)   # ceil(513 / 2) = 257 workgroups of two rows forward and backward
    assert (p["rw_fwd"], p["fused_fwd"], p["rw_bwd"], p["nblk_bwd"]) == (2, 0, 2, 257)
    p = plan_of(probe, B=256, **SMALL)
    assert (p["rw_bwd"], p["nblk_bwd"]) == (1, 256)
    p = plan_of(probe, B=257, **SMALL)
    assert (p["rw_bwd"], p["nblk_bwd"]) == (2, 129)
    # split-K at T = 1 (RT = B): 511 // 256 = 1 slice; 512: two chunks of 256; 544: two chunks of 272
    assert [(plan_of(probe, B=b, **SMALL)[k]) for b in (511, 512, 544) for k in ("ns_w1", "ns_w2")] == [1, 1, 2, 2, 2, 2]


@pytest.mark.parametrize("n,A,O,B,t_len", [(4, 5, 5, 8, 18), (10, 18, 176, 8, 181), (3, 5, 5, 3, 7), (1, 5, 10, 512, 2),
                                           (1, 5, 10, 257, 2), (5, 9, 20, 13, 61)])
def test_actor_items_equal_the_actor_critic_plan(probe, a2c_probe, n, A, O, B, t_len):
    """One actor plan for all: what coma_plan launches the shared actor with is what a2c_plan reports."""
    p = plan_of(probe, n=n, A=A, O=O, S=7, B=B, t_len=t_len)
    argv = [0, 64, n, A, O, 7, 1, 1, B, t_len]
    q = json.loads(subprocess.run([a2c_probe] + [str(a) for a in argv], check=True, capture_output=True,
                                  text=True).stdout)
    assert (p["ns_w1"], p["ns_w2"], p["nblk_bwd"]) == (q["ns_aw1"], q["ns_aw2"], q["bwd_blocks"])
    assert p["actor_rows"] == q["rows"] and p["npol"] == q["policy_blocks"]
    if (n, B, t_len) == (4, 8, 18):   # 544 rows: every split is 2
        assert (p["actor_rows"], p["ns_w1"], p["ns_w2"], p["nblk_bwd"]) == (544, 2, 2, 32)


def test_red_builder_refuses_a_region_past_its_table(probe):
    r = json.loads(subprocess.run([probe, "red"], check=True, capture_output=True, text=True).stdout)
    assert r["ok"] == 0 and r["nr"] == r["max_regions"] == 6
