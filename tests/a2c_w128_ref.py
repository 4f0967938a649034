"""tests/a2c_ref.py's and tests/ppo_ref.py's cases with the feed-forward actor at hidden width 128 (`hidden_dim: 128`
and no `rnn_hidden_dim`). ref64.unroll reads the agent's width off fc1.weight, so a2c_ref_step,
ppo_ref_epoch, judge and judge_updates serve as they are: only the case's agent shapes and weights are restated here,
at width W. The critic is 128 wide as well: epymarl's one key sets both.

The rows are in tiles of the forward's 64 rows and the backward's 32 (RT = T B n, dead rows included; I = O + A + n).
All but one episode are short, as §3k's `split` and §3n's `ns_walk` are, so that a seed exists: a seed is valid under
tests/a2c_ffn_ref.py's conditions (seed_minimum). `python -m tests.a2c_w128_ref` prints the first valid seed of 0..63 per
row."""
from collections import OrderedDict

from pymarl_amd.utils.synthetic import init_params
from tests import a2c_ffn_ref as F
from tests import a2c_ref as R
from tests import ppo_ref as PR
from tests.ffn_ref import ff_agent_shapes

W = 128
_S = dict(A=5, S=7, O=5)
_WALK = (16, 2, 1, 3) + (0,) * 16   # 66 live rows of the 960: §3n's nineteen short episodes leave PPO no seed at width 128
ROWS = OrderedDict([
    ("part", dict(_S, n=3, t_len=4, B=2, lengths=(3, 1), seed=0)),             # RT = 18: one partial tile; I = 13
    ("tile32", dict(_S, n=2, t_len=9, B=2, lengths=(8, 2), seed=0)),           # RT = 32: one full backward tile
    ("tile33", dict(_S, n=1, t_len=12, B=3, lengths=(11, 2, 1), seed=0)),      # RT = 33: .. and one row
    ("tile64", dict(_S, n=2, t_len=17, B=2, lengths=(16, 2), seed=0)),         # RT = 64: one full forward tile
    ("tile65", dict(_S, n=1, t_len=14, B=5, lengths=(13, 2, 1, 3, 1), seed=3)),   # RT = 65: .. and one row
    ("walk", dict(_S, n=3, t_len=17, B=20, lengths=_WALK, seed=18)),            # RT = 960: 30 backward, 15 forward tiles
    ("A33", dict(R._PART, A=33, seed=6)),                                      # fc2's and dW2's second column tile
    ("A64", dict(R._PART, A=64, seed=0)),                                      # .. full
    ("wideI", dict(R._PART, O=60, seed=1)),                                    # I = 68: three K chunks, I % 8 = 4
    ("n10", dict(n=10, A=18, t_len=4, S=7, O=5, B=2, lengths=(3, 1), seed=0)),   # cfg5's n and A
])
PPO_SEEDS = dict(part=3, walk=18)
PPO_KEYS = dict(PR.CLIP, epochs=4)
PPO_LENGTHS = dict(walk=(16,) + (0,) * 19)   # 48 live rows: four epochs of `walk`'s 66 leave no seed in 0..63


def _wide(case):
    case.agent_shapes = ff_agent_shapes(case.I, case.A, W)
    case.agent_params = init_params(case.agent_shapes, seed=case.seed + 1)


def _row(row):
    return dict(ROWS[row], over=dict(hidden_dim=W))


class A2CW128Case(R.A2CCase):
    def __init__(self, row, seed=None):
        R.ROWS["_w128"] = _row(row)   # A2CCase reads its row from a2c_ref.ROWS
        try:
            super().__init__("_w128", seed)
        finally:
            del R.ROWS["_w128"]
        self.row = row
        _wide(self)


class PPOW128Case(PR.PPOCase):
    def __init__(self, row, seed=None):
        R.ROWS["_w128"] = dict(_row(row), lengths=PPO_LENGTHS.get(row, ROWS[row]["lengths"]))
        PR.ROWS["_w128"] = dict(PPO_KEYS, base="_w128", seed=PPO_SEEDS[row])
        try:
            super().__init__("_w128", seed)
        finally:
            del R.ROWS["_w128"], PR.ROWS["_w128"]
        self.row = row
        _wide(self)


KEYS = dict(use_rnn=False, rnn_hidden_dim=None)   # epymarl's args: hidden_dim alone (the case's keys set it to 128)

if __name__ == "__main__":
    for ppo, rows, mk in ((False, ROWS, A2CW128Case), (True, PPO_SEEDS, PPOW128Case)):
        for row in rows:
            ok = next(((s, v) for s in range(64) for v in [F.seed_minimum(mk(row, s), ppo)] if v > R.MARGIN), None)
            print("ppo" if ppo else "a2c", row, "first valid seed (minimum):", ok or "none in 0..63", flush=True)
