"""TD(lambda) critic targets (q_targets: td_lambda) of ActorCriticLearner and PPOLearner on the GPU.
The returns are gated bitwise against tests/lambda_oracle.py fed the GPU's own V'. The training steps run the
procedures of tests/test_gpu_a2c.py (§3k) and tests/test_gpu_ppo.py (§3l) with every gate of theirs (the seeds' kink
margins too), the two keys added to the learners and only the return swapped (tests/test_a2c_lambda_host.py)."""
from functools import partial

import numpy as np
import pytest

from tests import a2c_ref as R
from tests import a2c_w128_ref as W
from tests import ppo_ref as PR
from tests import test_a2c_lambda_host as L
from tests import test_gpu_a2c as TA
from tests import test_gpu_ppo as TP
from tests.a2c_helpers import all_buffers, build_a2c

pytestmark = pytest.mark.gpu
ON = dict(q_targets="td_lambda", td_lambda=0.8)
PROCEDURES = {"a2c": (R.A2CCase, TA, TA.test_a2c_vs_ref, ("build_a2c",)),
              "ppo": (PR.PPOCase, TP, TP.test_ppo_epochs_vs_ref, ("build_ppo",)),
              "ppo1": (PR.PPOCase, TP, TP.test_one_epoch_is_the_actor_critic_learner_bitwise,
                       ("build_ppo", "build_a2c_on"))}


# B = 1; a partial workgroup of three with an empty episode; every lambda; two full workgroups; standardised rewards;
# B = 5 with n = 1 and episodes of length 1 that end before T; n = 10; two and one episodes a workgroup
@pytest.mark.parametrize("row,lam,plan_env", [
    ("one", 0.8, None), ("part", 0.0, None), ("part", 0.8, None), ("part", 1.0, None), ("split", 0.8, None),
    ("part_n10", 0.8, None), ("w128:tile65", 0.8, None), ("w128:n10", 0.8, None),
    ("split", 0.8, "lambda_episodes=2"), ("w128:tile65", 0.8, "lambda_episodes=1")])
def test_returns_bitwise(row, lam, plan_env, monkeypatch):
    if plan_env:   # read once per handle, at ma_create
        monkeypatch.setenv("MQ_PLAN", plan_env)
    wide = row.startswith("w128:")
    c = W.A2CW128Case(row[5:]) if wide else R.A2CCase(row)
    _, buf, _, learner, _ = build_a2c(c, q_targets="td_lambda", td_lambda=lam, **(W.KEYS if wide else {}))
    nb = c.batch()
    T = nb["filled"].shape[1] - 1
    m = np.asarray(nb["filled"][:, :T], np.float32)
    m[:, 1:] *= 1 - np.asarray(nb["terminated"][:, :T - 1], np.float32)
    for k in range(2):   # the second step standardises with merged statistics
        learner.train(TA.sample(buf, c), 1000 * (k + 1), 8 * k)
        Vt, ret = (learner.last_intermediate(i).cpu().numpy() for i in (0, 2))
        want = L.elem(c, Vt, TA.rewards32(c, nb, learner), m, lam)
        assert learner.last_returns() == 1 and ret.shape == (c.B, T, c.n) and np.array_equal(want, ret), (row, lam, k)


@pytest.mark.parametrize("kind,row", [("a2c", "part"), ("a2c", "part_n10"), ("ppo", "default"), ("ppo1", "part")])
def test_training_vs_ref(kind, row, monkeypatch):
    case, module, procedure, builders = PROCEDURES[kind]
    for name in builders:
        monkeypatch.setattr(module, name, partial(getattr(module, name), **ON))
    monkeypatch.delenv("MQ_PARITY_DIR", raising=False)   # the n-step rows' records stay theirs
    L.swap_returns(monkeypatch, case(row))
    procedure(row)


def test_one_step_is_the_absent_key_and_two_runs_are_bitwise_equal():
    c, runs = R.A2CCase("split"), []
    for over in ({}, dict(q_targets="one_step", td_lambda=0.8), ON, ON):
        _, buf, _, learner, _ = build_a2c(c, **over)
        for k in range(2):
            learner.train(TA.sample(buf, c), 1000 * (k + 1), 8 * k)
        runs.append(dict(all_buffers(learner), stats=learner._stats.cpu().numpy().copy(),
                         ret=learner.last_intermediate(2).cpu().numpy(), which=np.array(learner.last_returns())))
    for a, b, which in ((0, 1, 0), (2, 3, 1)):
        assert all(np.array_equal(runs[a][k], runs[b][k]) for k in runs[a]) and runs[a]["which"] == which
    assert not np.array_equal(runs[0]["ret"], runs[2]["ret"])
