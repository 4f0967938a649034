"""TD(lambda) critic targets of the actor-critic and PPO learners, without a GPU: the two keys' parsing
and refusals and the two entry points' argument checks. `swap_returns` is the reference tests/test_gpu_a2c_lambda.py
uses: tests/a2c_ref.py's and tests/ppo_ref.py's steps with only the return swapped."""
import numpy as np
import pytest
import torch as th

from pymarl_amd import _lib
from pymarl_amd.learners.actor_critic_learner import a2c_config
from pymarl_amd.learners.ppo_learner import ppo_config
from tests import a2c_ref as R
from tests import ppo_ref as PR
from tests.a2c_helpers import make_a2c_args
from tests.lambda_oracle import lambda_coefficients, td_lambda_returns
from tests.ppo_helpers import make_ppo_args

CONFIGS = ((a2c_config, make_a2c_args), (ppo_config, make_ppo_args))


def lambda_loop(Vt, r, m, term, gamma, lam):
    lg, og = (float(x) for x in lambda_coefficients(gamma, lam))   # as the C ABI forms them; torch at Vt's dtype
    ret, out = Vt[:, -1] * (1 - term.sum(1)), []
    for t in range(r.shape[1] - 1, -1, -1):
        ret = lg * ret + m[:, t] * (r[:, t] + og * Vt[:, t + 1] * (1 - term[:, t]))
        out.append(ret)
    return th.stack(out[::-1], 1)


def elem(case, Vt, r, m, lam):
    term = np.asarray(case.batch()["terminated"][:, :-1], np.float32)
    return td_lambda_returns(r, term, m, np.asarray(Vt, np.float32)[:, 1:], case.keys["gamma"], lam)


def swap_returns(monkeypatch, case, lam=0.8):
    term = np.asarray(case.batch()["terminated"][:, :-1], np.float64)

    def loop(Vt, r, m, *_):
        return lambda_loop(Vt, r, m, th.tensor(term, dtype=Vt.dtype), case.keys["gamma"], lam)
    monkeypatch.setattr(R, "nstep_loop", loop)
    monkeypatch.setattr(PR, "nstep_loop", loop)
    monkeypatch.setattr(R, "nstep_elem", lambda Vt, r, m, *_: elem(case, Vt, r, m, lam))


def test_key_parsing():
    c = PR.PPOCase("default")
    for config, args in CONFIGS:
        for lam in (0, 0.8, 1, np.float32(0.5)):
            got = config(args(c, q_targets="td_lambda", td_lambda=lam)).td_lambda
            assert type(got) is float and got == float(lam)
        absent = vars(config(args(c)))   # absent or one_step: the config as it is, whatever td_lambda says
        assert absent["td_lambda"] is None and vars(config(args(c, q_targets="one_step", td_lambda="x"))) == absent


@pytest.mark.parametrize("over,match", [
    (dict(td_lambda=1.5), "td_lambda"), (dict(td_lambda=-0.1), "td_lambda"), (dict(td_lambda=None), "td_lambda"),
    (dict(td_lambda="0.8"), "td_lambda"), (dict(td_lambda=True), "td_lambda"), (dict(td_lambda=float("nan")), "td_lambda"),
    (dict(q_targets=None), "q_targets"), (dict(q_targets="gae", td_lambda=0.8), "q_targets gae not recognised")])
def test_refusals(over, match):
    for config, args in CONFIGS:
        with pytest.raises(ValueError, match=match):
            config(args(PR.PPOCase("default"), **dict(dict(q_targets="td_lambda"), **over)))


def test_entry_points_check_arguments_before_the_handle():
    lib = _lib.load()
    for lam, gamma, msg in ((1.5, 0.99, b"td_lambda"), (float("nan"), 0.99, b"td_lambda"), (0.8, 1.5, b"gamma"),
                            (0.8, -0.1, b"gamma"), (0.8, float("nan"), b"gamma"), (0.8, 0.99, b"NULL handle"),
                            (-1.0, 0.99, b"NULL handle")):
        assert lib.ma_set_td_lambda(None, lam, gamma) != 0 and msg in lib.mq_last_error(), (lam, gamma)
    assert lib.ma_last_returns(None) == -1

