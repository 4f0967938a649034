"""The feed-forward actor of the actor-critic and PPO learners (use_rnn: False) without a GPU: the key, the
pi_logits BasicMAC, COMALearner's refusal, epymarl's state_dict names, and the seeds of tests/a2c_ffn_ref.py's rows."""
import pytest

from pymarl_amd import _lib
from pymarl_amd.learners import REGISTRY as le_REGISTRY
from pymarl_amd.learners.actor_critic_learner import make_a2c_config
from tests import a2c_ffn_ref as F
from tests import a2c_ref as R
from tests.a2c_helpers import build_a2c, make_a2c_args
from tests.ffn_ref import ff_agent_shapes
from tests.ppo_helpers import build_ppo

BUILD = {"actor_critic_learner": (build_a2c, lambda: F.A2CFFCase("part")),
         "ppo_learner": (build_ppo, lambda: F.PPOFFCase("part"))}


@pytest.mark.parametrize("name", list(BUILD))
def test_key_is_accepted(name):
    build, case = BUILD[name]
    c = case()
    args, _, mac, learner, _ = build(c, device="cpu", use_rnn=False)
    assert type(learner) is le_REGISTRY[name] and mac.agent_output_type == "pi_logits" and not mac.agent.use_rnn
    assert list(mac.agent.state_dict()) == list(ff_agent_shapes(c.I, c.A)) == [k for k, _ in mac.agent.named_parameters()]
    assert learner.n_agent_params == sum(a.size for a in c.agent_params.values())
    cfg = make_a2c_config(args, learner.cfg, mac.agent.input_dim, learner.critic, c.B, c.T + 1, learner._gpow)
    assert cfg.agent == _lib.AGENT_FFN == 1 and _lib.MAConfig._fields_[-1][0] == "agent"
    assert make_a2c_config(make_a2c_args(c), learner.cfg, mac.agent.input_dim, learner.critic, c.B, c.T + 1,
                           learner._gpow).agent == _lib.AGENT_GRU == 0
    assert [k for k, _ in _lib.MAActor._fields_][:3] == ["agent", "ffn_tiles", "ffn_blocks"]
    with pytest.raises(ValueError, match="use_rnn"):
        build(c, device="cpu", use_rnn="no")
    with pytest.raises(ValueError, match="use_rnn"):
        le_REGISTRY["coma_learner"](None, None, None, make_a2c_args(c, use_rnn=False, optimizer="rmsprop"))


@pytest.mark.parametrize("row", list(F.ROWS) + ["ppo_" + r for r in F.PPO_SEEDS])
def test_seed_conditions(row):
    ppo = row.startswith("ppo_")
    c = F.PPOFFCase(row[4:]) if ppo else F.A2CFFCase(row)
    assert F.seed_minimum(c, ppo) > R.MARGIN, row
