from .ac import ACCritic
from .centralv import CentralVCritic
from .coma import COMACritic

REGISTRY = {"coma": COMACritic}
REGISTRY["cv_critic"] = CentralVCritic
REGISTRY["ac_critic"] = ACCritic
