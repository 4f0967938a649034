"""GPU checks of the fused BPTT's lean per-step path (pymarl_amd/csrc/gru_bwd_fused.hpp LEAN; MQ_PLAN bwd_lean,
mq_plan.bwd_lean), through the product path QLearner.train -> libmq_learner.so.

A. bwd_lean=1 against bwd_lean=0, the classic step: the same seeded learner trained two steps under each; flat
   gradients, parameters and the five stats of both steps are bitwise equal. Shapes are the smallest at which each
   piece can go wrong: A = 9 (A mod 4 != 0: a lane's register slots past the last action), and T transitions
   (T + 1 unrolled steps, 16 to a chunk) = 1 (no walked load at all), 10 (one partial chunk), 15 / 16 / 17 (an exact
   chunk end, then one and two steps in the top chunk: the per-chunk inputs' hand-over), 33 (three chunks, partial
   top), each full-length and ragged (episodes from one step on), QMIX and VDN.
B. the lean path rides with the row-pair forward: under fwd_pair=0 the plan falls back to the classic step
   (mq_plan.bwd_lean == 0) and the case still passes its golden.
"""
import numpy as np
import pytest

from tests import test_gpu_parity as P
from tests.golden_utils import Case, SynthCase
from tests.gpu_helpers import build, flat_grads, flat_params, set_switch

pytestmark = pytest.mark.gpu

STATS = ("loss", "grad_norm", "td_error_abs", "q_taken_mean", "target_mean")


def train_two_steps(case, lean, monkeypatch):
    set_switch(monkeypatch, "bwd_lean", lean)   # read once, at handle creation
    args, buf, mac, learner, logger = build(case)
    np.random.seed(case.sampler_seed)
    out = []
    for k in range(2):
        batch = buf.sample(case.B)
        batch = batch[:, :batch.max_t_filled()]
        learner.train(batch, 1000 * k, case.episodes[k])
        st = learner.last_stats()
        out.append((flat_grads(learner), flat_params(learner), np.array([st[s] for s in STATS], np.float64)))
    return out, learner.last_plan()


@pytest.mark.parametrize("mixer", ["qmix", "vdn"])
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("T", [1, 10, 15, 16, 17, 33])
def test_lean_equals_classic_bitwise(T, ragged, mixer, monkeypatch):
    case = SynthCase("lean_T{}".format(T), n=3, A=9, O=30, S=48, T=T, B=2, n_episodes=2, steps=2, mixer=mixer,
                     ragged=ragged, min_len=1)
    got = {}
    for lean in (1, 0):
        got[lean], plan = train_two_steps(case, lean, monkeypatch)
        assert plan["bwd_lean"] == lean, plan
        assert plan["fused_fwd"] == 2 and plan["fused_bwd"] == 1, plan
    for k in range(2):
        for a, b, what in zip(got[1][k], got[0][k], ("grads", "params", "stats")):
            assert np.isfinite(a).all(), (T, ragged, mixer, k, what)
            assert np.array_equal(a, b), (T, ragged, mixer, k, what, float(np.abs(a - b).max()))


def test_lean_falls_back_without_the_pair_forward(monkeypatch):
    """The classic gate record of the one-row-net forward still feeds the BPTT: fwd_pair=0 with bwd_lean=1 asked for."""
    set_switch(monkeypatch, "fwd_pair", "0")
    set_switch(monkeypatch, "bwd_lean", 1)
    learner = P.run_teacher_forced(Case("cfg2_qmix_ragged"), 3, False, monkeypatch)
    plan = learner.last_plan()
    assert plan["fused_fwd"] == 1 and plan["fused_bwd"] == 1 and plan["bwd_lean"] == 0, plan
