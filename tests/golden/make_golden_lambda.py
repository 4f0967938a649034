"""Generate tests/golden/td_lambda_returns.npz with the REFERENCE's build_td_lambda_targets.

    python tests/golden/make_golden_lambda.py

Not part of the product and never run on the GPU box (it needs /root/reference, like make_golden.py). It imports
the reference's src/utils/rl_utils.py and applies build_td_lambda_targets (rl_utils.py:4-14) the way COMALearner
does (coma_learner.py:103-104) to the inputs the Q learner would hand it: reward, terminated and the learner's mask
(q_learner.py:39-44) of golden step 0, and the target network's mixed values y' of that step from the numpy oracle
(oracle/qlearner_np.py, itself pinned to the reference). target_qs[:, t + 1] = y'[:, t]; target_qs[:, 0] is never
read by the function and is left zero.

gamma and lambda go in as the doubles of their f32 roundings: the C ABI carries both as floats (mq_config), so the
reference function is pinned at the values the kernels see (f32(0.6) differs from 0.6 by 2.4e-8, enough to move the
f32 product lambda * gamma by an ulp).

Per case <c> in CASES the file holds <c>__rew, <c>__term, <c>__mask (B, L, 1), <c>__tq (B, L, k) and, per lambda
index i of `lams`, <c>__ret<i> (B, L, k); plus `gamma` and `lams` (float64, the f32-rounded values).
"""
from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True   # /root/reference is read-only: no __pycache__ there

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF_SRC = "/root/reference/src"
sys.path.insert(0, REPO)
sys.path.insert(0, REF_SRC)

import torch as th  # noqa: E402

from utils.rl_utils import build_td_lambda_targets  # noqa: E402  (reference)

from oracle.qlearner_np import OracleQLearner  # noqa: E402
from tests.golden_utils import Case  # noqa: E402

CASES = ["tiny_qmix", "tiny_vdn", "tiny_iql", "cfg1_qmix"]
LAMS = [0.0, 0.6, 1.0]
GAMMA = 0.99


def main():
    gamma = float(np.float32(GAMMA))
    lams = [float(np.float32(x)) for x in LAMS]
    out = {"gamma": np.float64(gamma), "lams": np.array(lams, np.float64)}
    for name in CASES:
        case = Case(name)
        nb, _ = case.batch(0)
        fw = OracleQLearner(case.agent_params, case.mixer_params, case.cfg()).forward(nb)
        rew = nb["reward"][:, :-1].astype(np.float32)
        term = nb["terminated"][:, :-1].astype(np.float32)
        mask = fw["mask"][..., :1].astype(np.float32).copy()
        tq = fw["target_q_tot"].astype(np.float32)
        B, L, k = tq.shape
        target_qs = th.cat([th.zeros(B, 1, k), th.from_numpy(tq)], dim=1)
        out.update({name + "__rew": rew, name + "__term": term, name + "__mask": mask, name + "__tq": tq})
        for i, lam in enumerate(lams):
            ret = build_td_lambda_targets(th.from_numpy(rew), th.from_numpy(term), th.from_numpy(mask), target_qs,
                                          case.n, gamma, lam)
            assert ret.shape == (B, L, k) and ret.dtype == th.float32
            out["{}__ret{}".format(name, i)] = ret.numpy().copy()
    path = os.path.join(HERE, "td_lambda_returns.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
