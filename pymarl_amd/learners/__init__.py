from .actor_critic_learner import ActorCriticLearner
from .coma_learner import COMALearner
from .ppo_learner import PPOLearner
from .q_learner import QLearner

REGISTRY = {}
REGISTRY["q_learner"] = QLearner
REGISTRY["coma_learner"] = COMALearner
REGISTRY["actor_critic_learner"] = ActorCriticLearner
REGISTRY["ppo_learner"] = PPOLearner
