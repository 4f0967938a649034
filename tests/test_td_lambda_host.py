"""Host-side checks of the opt-in TD(lambda) targets (mq_config.td_lambda; q_targets: td_lambda), no GPU needed:
the numpy lambda-oracle is pinned bitwise to the reference's build_td_lambda_targets (fixture written by
tests/golden/make_golden_lambda.py), reduces to the one-step oracle at lambda = 0, and the C ABI / Python config
carry the new field as include/mq_learner.h declares it."""
import ctypes
import os
import subprocess
from types import SimpleNamespace as SN

import numpy as np
import pytest

from pymarl_amd import _lib
from tests.golden_utils import GOLDEN
from tests.lambda_oracle import LambdaOracleQLearner, td_lambda_returns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE_CASES = ["tiny_qmix", "tiny_vdn", "tiny_iql", "cfg1_qmix"]


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(GOLDEN, "td_lambda_returns.npz"), allow_pickle=False)
    return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_numpy_returns_equal_reference_bitwise(fixture, name):
    """td_lambda_returns == the reference's build_td_lambda_targets on the same inputs, for every lambda."""
    gamma, lams = float(fixture["gamma"]), fixture["lams"]
    assert [round(float(x), 6) for x in lams] == [0.0, 0.6, 1.0]
    rew, term, mask, tq = (fixture[name + "__" + k] for k in ("rew", "term", "mask", "tq"))
    assert (tq.shape[2] > 1) == (name == "tiny_iql")   # one value per agent without a mixer
    for i, lam in enumerate(lams):
        got = td_lambda_returns(rew, term, mask, tq, gamma, float(lam))
        ref = fixture["{}__ret{}".format(name, i)]
        assert got.dtype == np.float32 and got.shape == ref.shape
        assert np.array_equal(got, ref), (name, float(lam), float(np.abs(got - ref).max()))
        # the plain decimal the user writes rounds to the same f32
        assert np.array_equal(td_lambda_returns(rew, term, mask, tq, 0.99, round(float(lam), 6)), ref)


@pytest.mark.parametrize("name", ["tiny_qmix", "tiny_vdn", "tiny_iql"])
def test_lambda_zero_is_the_one_step_oracle(golden_cases, name):
    from oracle.qlearner_np import OracleQLearner
    case = golden_cases[name]
    nb, _ = case.batch(0)
    o = OracleQLearner(case.agent_params, case.mixer_params, case.cfg())
    ol = LambdaOracleQLearner(case.agent_params, case.mixer_params, dict(case.cfg(), td_lambda=0.0))
    ag, mg, fw = o.gradients(nb)
    agl, mgl, fwl = ol.gradients(nb)
    assert np.array_equal(fwl["td"] * fwl["mask"], fw["td"] * fw["mask"])
    assert np.array_equal(fwl["targets"] * fwl["mask"], fw["targets"] * fw["mask"])
    assert fwl["loss"] == fw["loss"]
    for g, gl in ((ag, agl), (mg, mgl)):
        assert list(g) == list(gl)
        for k in g:
            assert np.array_equal(g[k], gl[k]), (name, k)


def test_lambda_changes_the_targets(golden_cases):
    """lambda > 0 is not the one-step target (the oracle's new piece is live), and lambda = 1 is the masked
    Monte-Carlo return plus the bootstrap of unterminated episodes."""
    from oracle.qlearner_np import OracleQLearner
    case = golden_cases["tiny_qmix"]
    nb, _ = case.batch(0)
    fw = OracleQLearner(case.agent_params, case.mixer_params, case.cfg()).forward(nb)
    fwl = LambdaOracleQLearner(case.agent_params, case.mixer_params, dict(case.cfg(), td_lambda=0.8)).forward(nb)
    live = fw["mask"] > 0
    assert np.abs(fwl["targets"] - fw["targets"])[live].max() > 1e-3
    fw1 = LambdaOracleQLearner(case.agent_params, case.mixer_params, dict(case.cfg(), td_lambda=1.0)).forward(nb)
    rew = nb["reward"][:, :-1].astype(np.float64)
    term = nb["terminated"][:, :-1].astype(np.float64)
    m = fw["mask"].astype(np.float64)
    L = rew.shape[1]
    g = 0.99
    mc = np.zeros_like(rew)
    acc = fw["target_q_tot"][:, L - 1].astype(np.float64) * (1.0 - term.sum(1))
    for t in range(L - 1, -1, -1):
        acc = g * acc + m[:, t] * rew[:, t]
        mc[:, t] = acc
    assert np.abs(fw1["targets"] - mc).max() <= 1e-5 * max(1.0, np.abs(mc).max())


def _probe(tmp_path):
    src = tmp_path / "probe_lambda.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "mq_learner.h"
int main(void) {
  printf("%zu %zu %zu %zu\\n", offsetof(mq_config, td_lambda), sizeof(mq_config), offsetof(mq_plan, td_lambda),
         sizeof(mq_plan));
  printf("%zu %zu\\n", sizeof(((mq_config*)0)->td_lambda), sizeof(((mq_plan*)0)->td_lambda));
  return 0;
}
""")
    exe = tmp_path / "probe_lambda"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    return [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]


def test_abi_layout_of_the_new_fields(tmp_path):
    c = _probe(tmp_path)
    py = [_lib.MQConfig.td_lambda.offset, ctypes.sizeof(_lib.MQConfig), _lib.MQPlan.td_lambda.offset,
          ctypes.sizeof(_lib.MQPlan), _lib.MQConfig.td_lambda.size, _lib.MQPlan.td_lambda.size]
    assert c == py
    assert _lib.MQConfig.td_lambda.offset == _lib.MQConfig.huber_delta.offset + 4   # appended after huber_delta
    assert _lib.MQPlan.td_lambda.offset == _lib.MQPlan.dwh.offset + 4


@pytest.mark.parametrize("bad", [-0.1, 1.5, float("nan")])
def test_td_lambda_outside_unit_interval_is_an_argument_error(bad):
    """Rejected in mq_create before any HIP call (this test runs without a GPU)."""
    lib = _lib.load()
    cfg = _lib.MQConfig(n_agents=3, n_actions=9, obs_dim=30, state_dim=48, rnn_hidden_dim=64, mixing_embed_dim=32,
                        mixer=2, max_batch=4, max_seq=11, td_lambda=bad)
    h = ctypes.c_void_p()
    assert lib.mq_create(ctypes.byref(cfg), ctypes.byref(h)) == 1
    assert b"td_lambda" in lib.mq_last_error()
    assert not h.value


def test_scan_lds_bound_is_an_argument_error():
    """The scan stages L (k + 3) floats of an episode in LDS, at most 64 KB: a longer max_seq is refused in mq_create
    (no mixer, 64 agents, 300 stored steps: 299 * 67 * 4 B = 80 KB) before any HIP call."""
    lib = _lib.load()
    h = ctypes.c_void_p()
    kw = dict(n_agents=64, n_actions=9, obs_dim=30, state_dim=48, rnn_hidden_dim=64, mixing_embed_dim=32, mixer=0,
              max_batch=1, max_seq=300)
    assert lib.mq_create(ctypes.byref(_lib.MQConfig(td_lambda=0.5, **kw)), ctypes.byref(h)) == 1
    msg = lib.mq_last_error()
    assert b"td_lambda" in msg and b"LDS" in msg
    assert not h.value


def _args(**over):
    a = SN(n_agents=3, n_actions=5, obs_shape=30, state_shape=48, rnn_hidden_dim=64, mixing_embed_dim=32,
           obs_last_action=True, obs_agent_id=True)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_make_config_selects_lambda_only_through_q_targets():
    from pymarl_amd.learners.q_learner import make_config
    # a COMA-style global td_lambda must not change the Q learner
    assert make_config(_args(td_lambda=0.8), _lib.MIXER_QMIX).td_lambda == 0.0
    assert make_config(_args(td_lambda=0.8, q_targets="one_step"), _lib.MIXER_QMIX).td_lambda == 0.0
    assert make_config(_args(), _lib.MIXER_QMIX).td_lambda == 0.0
    cfg = make_config(_args(q_targets="td_lambda", td_lambda=0.6), _lib.MIXER_QMIX)
    assert cfg.td_lambda == float(np.float32(0.6))
    assert abs(cfg.td_lambda - 0.6) < 1e-7
    with pytest.raises(ValueError, match="q_targets"):
        make_config(_args(q_targets="nstep", td_lambda=0.6), _lib.MIXER_QMIX)
