"""The two-layer QMIX hypernetwork (hypernet_layers: 2) without a GPU: the module's state_dict against upstream's
restated module (tests/hyper2_ref.RefQMixer2), checkpoint interchange both ways, the configuration errors, the plan
through tests/host/plan2_probe.cpp, and the conditions the GPU gradient gate of tests/test_gpu_hyper2.py rests on
(the float32 reference run leaves the gate room; the chosen seeds keep clear of the mixer's kinks)."""
import ctypes
import json
import os
import shutil
import subprocess
from types import SimpleNamespace as SN

import numpy as np
import pytest
import torch as th

from pymarl_amd import _lib
from pymarl_amd.learners.q_learner import make_config
from pymarl_amd.modules.mixers.qmix import QMixer
from tests import hyper2_ref as R
from tests import ref64
from tests.test_plan_host import CUS, HIPCC, MIXERS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def mixer_args(n=3, S=48, E=32, **kw):
    return SN(n_agents=n, state_shape=S, mixing_embed_dim=E, **kw)


@pytest.mark.parametrize("n,S,He", [(3, 48, 64), (2, 30, 20)])
def test_state_dict_is_upstreams(n, S, He):
    ours = QMixer(mixer_args(n, S, hypernet_layers=2, hypernet_embed=He)).state_dict()
    ref = R.RefQMixer2(n, S, 32, He).state_dict()
    assert list(ours) == list(ref) == list(R.mixer2_shapes(S, n, He))
    for k, v in ref.items():
        assert tuple(ours[k].shape) == tuple(v.shape) == R.mixer2_shapes(S, n, He)[k], k


def test_flat_buffer_follows_parameters_order():
    m = QMixer(mixer_args(hypernet_layers=2, hypernet_embed=20))
    shapes = R.mixer2_shapes(48, 3, 20)
    assert [tuple(p.shape) for p in m.parameters()] == list(shapes.values())
    o = 0
    for p in m.parameters():   # each parameter is a view of the flat buffer at its running offset
        assert p.data_ptr() == m.flat_params().data_ptr() + 4 * o
        o += p.numel()
    assert o == m.flat_params().numel() == sum(int(np.prod(s)) for s in shapes.values())


def test_checkpoint_interchanges_with_upstream(tmp_path):
    th.manual_seed(5)
    ref = R.RefQMixer2(3, 48, 32, 64)
    ours = QMixer(mixer_args(hypernet_layers=2, hypernet_embed=64))
    th.save(ref.state_dict(), str(tmp_path / "mixer.th"))   # upstream writes, we load
    ours.load_state_dict(th.load(str(tmp_path / "mixer.th"), weights_only=True))
    for k, v in ref.state_dict().items():
        assert th.equal(ours.state_dict()[k], v), k
    flat = th.cat([p.detach().reshape(-1) for p in ref.parameters()])
    assert th.equal(ours.flat_params(), flat)   # and the flat buffer the kernels read holds them in that order
    with th.no_grad():
        ours.flat_params().mul_(0.5)
    th.save(ours.state_dict(), str(tmp_path / "ours.th"))   # we write, upstream loads
    back = R.RefQMixer2(3, 48, 32, 64)
    back.load_state_dict(th.load(str(tmp_path / "ours.th"), weights_only=True))
    for k, v in ref.state_dict().items():
        assert th.equal(back.state_dict()[k], 0.5 * v), k


def test_one_layer_is_the_default_and_unchanged():
    for kw in ({}, dict(hypernet_layers=1), dict(hypernet_layers=1, hypernet_embed=999)):
        m = QMixer(mixer_args(**kw))
        assert list(m.state_dict())[:4] == ["hyper_w_1.weight", "hyper_w_1.bias", "hyper_w_final.weight",
                                            "hyper_w_final.bias"]
        assert m.hypernet_layers == 1


def test_configuration_errors():
    with pytest.raises(Exception, match="Sorry >2 hypernet layers is not implemented!"):
        QMixer(mixer_args(hypernet_layers=3))
    for bad in (0, -1, "two"):
        with pytest.raises(Exception, match="Error setting number of hypernet layers."):
            QMixer(mixer_args(hypernet_layers=bad))
    for bad in (0, 65, 128):
        with pytest.raises(ValueError, match="64"):
            QMixer(mixer_args(hypernet_layers=2, hypernet_embed=bad))
    QMixer(mixer_args(hypernet_layers=2, hypernet_embed=1))
    QMixer(mixer_args(hypernet_layers=2))   # hypernet_embed defaults to 64


def learner_args(**kw):
    return SN(n_agents=3, n_actions=9, obs_shape=30, state_shape=48, rnn_hidden_dim=64, mixing_embed_dim=32,
              obs_last_action=True, obs_agent_id=True, **kw)


def test_make_config_passes_the_keys_and_other_mixers_ignore_them():
    cfg = make_config(learner_args(hypernet_layers=2, hypernet_embed=20), _lib.MIXER_QMIX)
    assert (cfg.hypernet_layers, cfg.hypernet_embed) == (2, 20)
    cfg = make_config(learner_args(), _lib.MIXER_QMIX)
    assert (cfg.hypernet_layers, cfg.hypernet_embed) == (1, 64)
    for mixer in (_lib.MIXER_VDN, _lib.MIXER_NONE):   # VDN / IQL: not even validated
        cfg = make_config(learner_args(hypernet_layers=7, hypernet_embed=4096), mixer)
        assert (cfg.hypernet_layers, cfg.hypernet_embed) == (0, 0)


@pytest.mark.parametrize("layers,embed,word", [(2, 0, b"hypernet_embed"), (2, 65, b"hypernet_embed"),
                                               (3, 64, b"hypernet_layers"), (-1, 64, b"hypernet_layers")])
def test_library_rejects_bad_values_before_any_hip_call(layers, embed, word):
    lib = _lib.load()
    cfg = _lib.MQConfig(n_agents=3, n_actions=9, obs_dim=30, state_dim=48, rnn_hidden_dim=64, mixing_embed_dim=32,
                        mixer=2, max_batch=4, max_seq=11, hypernet_layers=layers, hypernet_embed=embed)
    h = ctypes.c_void_p()
    assert lib.mq_create(ctypes.byref(cfg), ctypes.byref(h)) == 1   # MQ_ERR_ARG
    assert word in lib.mq_last_error()
    assert lib.mq_qmix_forward2(None, 3, 48, 32, 64, None, None, None, 1, None) == 1
    one = ctypes.c_void_p(8)   # never dereferenced: the argument check comes first
    assert lib.mq_qmix_forward2(one, 3, 48, 32, 65, one, one, one, 1, None) == 1
    assert b"hypernet_embed" in lib.mq_last_error()


# ---------------------------------------------------------------------------------------------- the gate's conditions
@pytest.fixture(scope="module")
def steps():
    """{row: [(case, params, targets, batch, float64 result)] for step 0 and step 1}, step 1 from the float64
    reference's own RMSprop update of step 0."""
    out = {}
    for row in R.ROW_SHAPES:
        case = R.synth_case2(row)
        p = t = ref64.flat_of(case)
        sq = np.zeros_like(p, np.float64)
        recs = []
        for k in range(2):
            nb, _ = case.batch(k)
            r = ref64.ref_step(case, p, t, nb)
            recs.append((case, p, t, nb, r))
            p, sq = ref64.rmsprop(case, p, sq, r.clipped_flat)
            p = p.astype(np.float32)
        out[row] = recs
    return out


@pytest.mark.parametrize("row", list(R.ROW_SHAPES))
def test_seeds_keep_clear_of_the_kinks(steps, row):
    for k, (case, p, t, nb, r) in enumerate(steps[row]):
        ref64.assert_clear_of_kinks(r, "{} step {}".format(row, k))
        live = np.broadcast_to(r.mask.reshape(r.a1.shape[0], r.a1.shape[1], 1) > 0, r.a1.shape)
        assert np.isfinite(r.loss) and live.any()


def test_float32_reference_leaves_the_gate_room(steps):
    """e32 of every block on the base shape is below TOL_CAP / TOL_ROOM: the cap never decides a block there, so
    tol = TOL_ROOM * max(e32, E32_FLOOR) is a bound an fp32 implementation with another summation order can meet."""
    case, p, t, nb, r64 = steps["base"][0]
    r32 = ref64.ref_step(case, p, t, nb, dtype=th.float32, cur_max_override=r64.cur_max_actions,
                     relu_override=r64.pre > 0, hyp_relu_override=r64.a1 > 0)
    e32 = ref64.block_errors(r32.clipped_flat, r64.clipped, case)
    assert set(R.mixer2_shapes(case.S, case.n, case.He)) <= set(e32)
    worst = max(e32, key=e32.get)
    print("worst e32 {:.3g} at {}".format(e32[worst], worst))
    assert e32[worst] < ref64.TOL_CAP / ref64.TOL_ROOM, (worst, e32[worst])
    assert abs(r32.norm - r64.norm) <= 1e-5 * r64.norm


def test_overrides_at_the_references_own_decisions_change_nothing(steps):
    case, p, t, nb, r = steps["base_he20"][0]
    r2 = ref64.ref_step(case, p, t, nb, cur_max_override=r.cur_max_actions, relu_override=r.pre > 0,
                    hyp_relu_override=r.a1 > 0)
    assert np.array_equal(r2.clipped_flat, r.clipped_flat)
    c = ref64.classify(r, r.cur_max_actions, r.pre > 0, got_hyp_relu=r.a1 > 0)
    assert c["dq_flips"] == c["relu_flips"] == c["hyp_relu_flips"] == 0
    assert c["hyp_relu_decisions"] == r.a1.size


def test_restated_module_agrees_with_ref_step_mixer():
    """RefQMixer2 (the standalone forward's reference) and ref_step's functional mixer are the same function."""
    th.manual_seed(3)
    m = R.RefQMixer2(3, 48, 32, 20).double()
    qs, st = th.randn(2, 5, 3, dtype=th.float64), th.randn(2, 5, 48, dtype=th.float64)
    y = ref64.qmix(dict(m.state_dict()), qs, st, 3)[0]
    assert th.allclose(m(qs, st), y, rtol=1e-13, atol=1e-13)


def test_reference_restatement_reproduces_the_reference_learners_golden_step():
    """tests/golden/tiny_qmix_h2.npz was written by the reference's own CPU QLearner around the restated mixer: ref_step
    in float64 reproduces its step-0 loss, stats, Q_tot, double-Q actions and clipped gradient to fp32 rounding."""
    case = R.GoldenCase2()
    z = case.z
    nb, ids = case.batch(0)
    assert np.array_equal(ids, z["ids"][0])
    p = ref64.flat_of(case)
    r = ref64.ref_step(case, p, p, nb)
    assert abs(r.loss - float(z["stat_loss"][0])) <= 1e-6 * r.loss
    for k in ("grad_norm", "td_error_abs", "q_taken_mean", "target_mean"):
        assert abs(r.stats[k] - float(z["stat_" + k][0])) <= 2e-6 * abs(r.stats[k]), k
    assert np.array_equal(r.cur_max_actions, z["step0_cur_max_actions"])
    assert np.abs(r.clipped_flat - z["step0_grads_clipped"]).max() <= 1e-5 * np.abs(r.clipped_flat).max()
    p1, _ = ref64.rmsprop(case, p, np.zeros_like(p, np.float64), z["step0_grads_clipped"])
    assert np.abs(p1 - z["step_params"][0]).max() <= 1e-6


# ---------------------------------------------------------------------------------------------- the plan
@pytest.fixture(scope="module")
def probe2(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc to build tests/host/plan2_probe.cpp with")
    exe = str(tmp_path_factory.mktemp("plan2_probe") / "plan2_probe")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1",
                    os.path.join(ROOT, "tests", "host", "plan2_probe.cpp"), "-o", exe], check=True)
    return exe


def plan2(probe2, mixer, d, t_len, layers, num_cu=CUS, plan_env=""):
    env = {k: v for k, v in os.environ.items() if k not in ("MQ_PLAN", "MQ_DIAG")}
    if plan_env:
        env["MQ_PLAN"] = plan_env
    argv = [num_cu, MIXERS[mixer], d["n"], d["A"], d["O"], d["S"], 32, 1, 1, 1, d["B"], t_len, layers, 64]
    out = subprocess.run([probe2] + [str(a) for a in argv], env=env, check=True, capture_output=True, text=True)
    return json.loads(out.stdout)


FWD_BWD = ("rows", "fused_fwd", "rw_fwd", "fused_bwd", "rw_bwd", "inline_ids", "tiles", "bwd_lean", "td_lambda", "mix")


@pytest.mark.parametrize("shape,plan_env", [("base", ""), ("gemm", ""), ("stream", ""), ("tiles_r21", "row_tiles=1"),
                                            ("base", "lambda_path=1"), ("base", "hyp_in_fwd=1"),
                                            ("base", "dwh_in_bwd=1")])
def test_two_layer_plan_is_the_vdn_plan_with_its_own_hypernet(probe2, shape, plan_env):
    d = ref64.SHAPES[shape]
    two = plan2(probe2, "qmix", d, d["T"] + 1, 2, plan_env=plan_env)
    vdn = plan2(probe2, "vdn", d, d["T"] + 1, 2, plan_env=plan_env)
    one = plan2(probe2, "qmix", d, d["T"] + 1, 1, plan_env=plan_env)
    assert (two["hyper_layers"], one["hyper_layers"], vdn["hyper_layers"]) == (2, 1, 0)
    for k in FWD_BWD:
        assert two[k] == vdn[k], (k, two, vdn)
    assert two["hyper"] == 3 and two["dwh"] == 0, two   # layer 1 as the GEMM; no dW_hyper tiles in the BPTT's grid
    if shape == "base" and not plan_env:
        assert (two["fused_fwd"], two["fused_bwd"], two["bwd_lean"]) == (2, 1, 1), two


def test_two_waves_of_rows_keep_the_hypernet_out_of_the_forward_and_the_bptt(probe2):
    d = dict(ref64.SHAPES["base"], B=86)   # R = 258 > 256 CUs: one layer appends the hypernet and dW_hyper there
    one = plan2(probe2, "qmix", d, 6, 1)
    two = plan2(probe2, "qmix", d, 6, 2)
    vdn = plan2(probe2, "vdn", d, 6, 1)
    assert one["dwh"] == 1 and two["dwh"] == 0
    for k in FWD_BWD:
        assert two[k] == vdn[k], (k, two, vdn)
