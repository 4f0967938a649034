"""A handle's workspace must cover what any step's plan asks of it, and a buffer that is too small shows only as silent
corruption on the device. Both sides are pure functions of the config (pymarl_amd/csrc/learner_layout.hpp,
step_plan.hpp, reduce_plan.hpp), so tests/host/ws_probe.cpp compares them without a GPU: for a handle sized for a
batch, and a step of exactly that batch, every slab buffer, red_tmp and norm_part is at least what the plan needs, and
every region of the reduction plan lies inside the buffer it starts in.

The shapes: every row of tests/test_gpu_grad_blocks.ROWS (t_len from tests/golden/plans_parent.json), the bench shapes
and the threshold shapes of tests/test_plan_host.py, each also with the feed-forward agent and, under QMIX, with the
two-layer hypernet; and one wide-input shape whose norm_part exceeds its floor of 256 floats.

The probe's parameter offsets are also held against the Python side's flat layout (what
tests/test_host_logic.py::test_parameter_names_order_and_flat_layout checks of it: the modules' parameters() order,
packed) for the four agent x hypernet combinations.
"""
import json
import logging
import os
import shutil
import subprocess

import pytest

from pymarl_amd import _lib
from tests import ref64
from tests.gpu_helpers import switch_value
from tests.test_gpu_grad_blocks import ROWS
from tests.test_plan_host import BASE, BENCH, CUS, EDGES, HIPCC, MIXERS, PARENT, ROOT

HE = 64   # hypernet_embed of the two-layer cases (epymarl's default)
NEED = ("slab_fc1", "slab_rnn", "slab_mix", "slab_v2", "loss_part", "red_tmp", "norm_part")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc to build tests/host/ws_probe.cpp with")
    exe = str(tmp_path_factory.mktemp("ws_probe") / "ws_probe")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1",
                    os.path.join(ROOT, "tests", "host", "ws_probe.cpp"), "-o", exe], check=True)
    return exe


def run_probe(probe, num_cu, shape, B, t_len, switches=None, agent=0, layers=1, E=32, flags=(1, 1, 1)):
    env = {k: v for k, v in os.environ.items() if k not in ("MQ_PLAN", "MQ_DIAG")}
    for key, v in (switches or {}).items():
        var, val = switch_value(env, key, v)
        env[var] = val
    argv = [num_cu, MIXERS[shape["mixer"]], shape["n"], shape["A"], shape["O"], shape["S"], E, *flags, B, t_len,
            agent, layers, HE]
    out = subprocess.run([probe] + [str(a) for a in argv], env=env, check=True, capture_output=True, text=True)
    return json.loads(out.stdout)


def cases():
    """(id, num_cu, shape, B, t_len, switches) of every shape the module docstring names."""
    out = []
    for row, (shape, mixer, switches, _) in ROWS.items():
        s = ref64.SHAPES[shape]
        out.append(("row_" + row, CUS, dict(s, mixer=mixer), s["B"], PARENT["rows"][row]["t_len"], switches))
    for name, num_cu, B, switches, _, _ in EDGES:
        out.append(("edge_" + name, num_cu, BASE, B, 6, switches))
    for cfg, ((mixer, n, A, O, S, T, B), _) in BENCH.items():
        out.append(("bench_" + cfg, 256, dict(n=n, A=A, O=O, S=S, mixer=mixer), B, T + 1, {}))
    for mixer in ("vdn", "qmix"):   # norm_part past its floor: (64 * I + 64) / 256 alone is 300 blocks
        out.append(("wide_input_" + mixer, 256, dict(n=2, A=5, O=1200, S=8, mixer=mixer), 2, 3, {}))
    return out


CASES = cases()
VARIANTS = [("gru", 0, 1), ("ffn", 1, 1), ("gru_hyper2", 0, 2), ("ffn_hyper2", 1, 2)]
# the two-layer hypernet exists under QMIX only
SIZED = [(c, v) for c in CASES for v in VARIANTS if v[2] == 1 or c[2]["mixer"] == "qmix"]


@pytest.mark.parametrize("case,var", SIZED, ids=[c[0] + "-" + v[0] for c, v in SIZED])
def test_workspace_covers_the_plan(probe, case, var):
    name, num_cu, shape, B, t_len, switches = case
    variant, agent, layers = var
    r = run_probe(probe, num_cu, shape, B, t_len, switches, agent, layers)
    for buf in NEED:
        print(name, variant, buf, "need", r["need"][buf], "size", r["size"][buf])
        assert r["need"][buf] <= r["size"][buf], (name, variant, buf, r["need"][buf], r["size"][buf])
    assert r["need"]["norm_part"] > 0 and r["regions"] >= 3, r
    assert r["regions_inside"], (name, variant, r)


def test_wide_input_is_past_the_norm_part_floor(probe):
    for case in CASES:
        if case[0].startswith("wide_input"):
            r = run_probe(probe, *case[1:])
            assert r["size"]["norm_part"] > 256 and r["need"]["norm_part"] > 256, r


@pytest.mark.parametrize("variant,agent,layers", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_offsets_are_the_python_sides_flat_layout(probe, variant, agent, layers):
    """The learner's flat buffer is its modules' parameters() in order, packed (test_host_logic): the library's offsets
    of the same config name the same places, and the tensors the config lacks sit at the total."""
    from pymarl_amd.components.episode_buffer import ReplayBuffer
    from pymarl_amd.components.transforms import OneHot
    from pymarl_amd.controllers import REGISTRY as mac_REGISTRY
    from pymarl_amd.learners import REGISTRY as le_REGISTRY
    from pymarl_amd.utils.logging import Logger
    from tests.test_host_logic import args, scheme
    a = args("qmix")
    if agent:
        a.use_rnn = False
    if layers == 2:
        a.hypernet_layers, a.hypernet_embed = 2, HE
    rb = ReplayBuffer(scheme(), {"agents": 2}, 4, 3, preprocess={"actions": ("actions_onehot", [OneHot(5)])})
    mac = mac_REGISTRY["basic_mac"](rb.scheme, {"agents": 2}, a)
    learner = le_REGISTRY["q_learner"](mac, rb.scheme, Logger(logging.getLogger("t")), a)
    want, o = {}, 0
    for mod in (mac.agent, learner.mixer):
        for pname, p in mod.named_parameters():
            assert p.data_ptr() == learner._online.data_ptr() + 4 * o, pname
            # the two-layer hypernet's first layers take the one-layer entries' places in MQ_P_*
            key = pname.replace("hyper_w_1.0.", "hyper_w_1.").replace("hyper_w_final.0.", "hyper_w_final.")
            want[key] = o
            o += p.numel()
    assert o == learner.n_params
    r = run_probe(probe, 256, dict(n=2, A=5, O=3, S=4, mixer="qmix"), 4, 3, agent=agent, layers=layers)
    got = r["offsets"]
    assert len(got) == _lib.P_COUNT + 1 and got[-1] == o
    for i, pname in enumerate(_lib.PARAM_NAMES):
        assert got[i] == want.get(pname, o), (variant, pname, got[i], want.get(pname))
    assert set(want) <= set(_lib.PARAM_NAMES), want
