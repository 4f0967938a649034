"""tests/a2c_ref.py's and tests/ppo_ref.py's cases with the feed-forward agent (use_rnn: False): ref64.unroll
takes its feed-forward branch from the parameter names, so a2c_ref_step and ppo_ref_epoch serve as they are. A seed is
valid when the four kink minima (critic fc1 / fc2, agent fc1, and the agent's second relu, taken from ref64.unroll's
third result) stay above ref64.KINK_EPS at both steps in float64, the float32 run's update standing in for the GPU's;
a PPO row also needs every live ratio clear of the clip bounds and float64 / float32 agreeing on w at each epoch.
`python -m tests.a2c_ffn_ref` prints the first valid seed of 0..63 per row."""
from collections import OrderedDict

import numpy as np
import torch as th

from pymarl_amd.utils.synthetic import init_params
from tests import a2c_ref as R
from tests import ppo_ref as PR
from tests import ref64
from tests.ffn_ref import ff_agent_shapes

_PART = R._PART
# a2c_ref.ROWS' shapes by name where one fits (RT = 64-row tiles of the T B n rows; I = O + A + n):
ROWS = OrderedDict([
    ("one", dict(R.ROWS["one"], seed=0)),             # RT = 2, A = 2
    ("part", dict(R.ROWS["part"], seed=0)),           # 54 rows: one partial tile; I = 13, not a multiple of 4
    ("part_n10", dict(R.ROWS["part_n10"], seed=0)),   # obs_last_action: False, RMSprop, reward standardisation
    ("tile64", dict(n=4, A=5, t_len=5, S=7, O=5, B=4, lengths=(4, 4, 4, 4), seed=4)),   # RT = 64 exactly, all live
    ("A33", dict(R.ROWS["A33"], seed=6)),             # two column tiles of W2 with a remainder
    ("A64", dict(R.ROWS["A64"], seed=0)),             # .. and without
    ("split", dict(R.ROWS["split"], seed=9)),         # RT = 544: nine tiles, the last of 32 rows; split-K in Dw1Prob
    # O = 256: I = 264 > 248, so W1 [64][268] is 68,608 B, past kFfnActorW1Budget = 65,536 B: streamed in five K chunks
    ("wideI", dict(_PART, O=256, seed=0)),
])
PPO_SEEDS = dict(part=0, split=9, part_n10=0)   # tests/ppo_ref.py's rows of these names, at eps_clip 0.01, epochs 3


def _ff(case):
    case.agent_shapes = ff_agent_shapes(case.I, case.A)
    case.agent_params = init_params(case.agent_shapes, seed=case.seed + 1)


class A2CFFCase(R.A2CCase):
    def __init__(self, row, seed=None):
        R.ROWS["_ffn"] = ROWS[row]   # A2CCase reads its row from a2c_ref.ROWS
        try:
            super().__init__("_ffn", seed)
        finally:
            del R.ROWS["_ffn"]
        self.row = row
        _ff(self)


class PPOFFCase(PR.PPOCase):
    def __init__(self, row, seed=None):
        super().__init__(row, PPO_SEEDS[row] if seed is None else seed)
        _ff(self)


def relu2_min(case, state, batch, mask):
    """min |pre-activation| of the agent's second relu over live rows, float64. mask: the step's (B, T, 1)."""
    T = mask.shape[1]
    t = lambda a: th.tensor(np.asarray(a, np.float64))   # noqa: E731
    Pa = R._params(case.views()[0], state["agent"], R.F64)
    onehot = t(batch["actions_onehot"][:, :T]) * t(batch["filled"][:, :T])[..., None]
    with th.no_grad():
        pre2 = ref64.unroll(Pa, t(batch["obs"][:, :T]), onehot, (case.obs_last_action, True), R.F64)[2]
    return float(pre2.abs()[th.tensor(np.array(np.broadcast_to(mask > 0, pre2.shape[:3])))].min())


def kinks(case, state, batch, r64):
    return dict(r64.kink_minima, agent_relu2=relu2_min(case, state, batch, r64.mask))


def seed_minimum(case, ppo):
    """The smallest of what a seed must keep above the margin, over the two steps (a2c) or the case's epochs (ppo)."""
    b, st, lo = case.batch(), case.init_state(), np.inf
    old64 = old32 = ret64 = ret32 = None
    for _ in range(case.epochs if ppo else 2):
        if ppo:
            r64 = PR.ppo_ref_epoch(case, st, b, old64, ret64, R.F64)
            r32 = PR.ppo_ref_epoch(case, st, b, old32, ret32, R.F32)
            if old64 is None:
                old64, ret64, old32, ret32 = r64.old, r64.ret, r32.old, r32.ret
            lo = min(lo, r64.bound_dist, r32.bound_dist, 1.0 if np.array_equal(r64.w[r64.live], r32.w[r32.live]) else 0.0)
        else:
            r64, r32 = R.a2c_ref_step(case, st, b, R.F64), R.a2c_ref_step(case, st, b, R.F32)
        lo = min(lo, *kinks(case, st, b, r64).values())
        st = R.to32(r32.new)
    return lo


if __name__ == "__main__":
    for ppo, rows, mk in ((False, ROWS, A2CFFCase), (True, PPO_SEEDS, PPOFFCase)):
        for row in rows:
            ok = next(((s, v) for s in range(64) for v in [seed_minimum(mk(row, s), ppo)] if v > R.MARGIN), None)
            print("ppo" if ppo else "a2c", row, "first valid seed (minimum):", ok or "none in 0..63", flush=True)
