from .rnn_agent import RNNAgent
from .rnn_ns_agent import RNNNSAgent

REGISTRY = {}
REGISTRY["rnn"] = RNNAgent
REGISTRY["rnn_ns"] = RNNNSAgent
