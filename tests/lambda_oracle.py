"""ORACLE for the opt-in TD(lambda) targets of the QMIX / VDN / IQL learner — test infrastructure only.

`td_lambda_returns` restates the reference's `build_td_lambda_targets` (src/utils/rl_utils.py:4-14) in numpy float32,
applied as COMALearner applies it (coma_learner.py:103-104) to the target network's mixed values:

    lg = f32(double(lambda) * double(gamma));  og = f32((1 - double(lambda)) * double(gamma))
    ret[L]  = y'[L-1] * (1 - sum_{t<L} term[t])
    ret[t]  = (lg * ret[t+1]) + mask[t] * (rew[t] + (og * y'[t]) * (1 - term[t]))        t = L-1 .. 0

with every product and sum rounded separately to f32 in this order (torch evaluates the reference's expression
left to right; its Python-float products lambda * gamma and (1 - lambda) * gamma become f32 scalars). lambda and
gamma are first rounded to f32, because that is how the C ABI carries them (mq_config.gamma / td_lambda are floats);
the fixture tests/golden/td_lambda_returns.npz holds the reference function's outputs for those f32 values
(tests/golden/make_golden_lambda.py), and tests/test_td_lambda_host.py pins this function to it bitwise.

`LambdaOracleQLearner` is the numpy QLearner of oracle/qlearner_np.py with its one-step target replaced by these
returns; everything after the TD error (mask, L2 or Huber, gradients, clip, RMSprop, stats) is the parent's.
"""
from __future__ import annotations

import numpy as np

from oracle.qlearner_np import F32, OracleQLearner


def lambda_coefficients(gamma, lam):
    """(lg, og) as f32, from lambda and gamma as the C ABI carries them (f32), multiplied in double."""
    g, la = float(F32(gamma)), float(F32(lam))
    return F32(la * g), F32((1.0 - la) * g)


def td_lambda_returns(rew, term, mask, tq, gamma, lam):
    """rew, term, mask (B, L, 1) and tq = y' (B, L, k) float32, y'[:, t] the target net's value at step t + 1.
    Returns the lambda targets (B, L, k) float32."""
    rew, term, mask, tq = (np.asarray(x, F32) for x in (rew, term, mask, tq))
    lg, og = lambda_coefficients(gamma, lam)
    L = tq.shape[1]
    out = np.empty_like(tq)
    one = F32(1.0)
    ret = (tq[:, L - 1] * (one - term.sum(1, dtype=F32))).astype(F32)
    for t in range(L - 1, -1, -1):
        inner = (rew[:, t] + ((og * tq[:, t]).astype(F32) * (one - term[:, t])).astype(F32)).astype(F32)
        ret = ((lg * ret).astype(F32) + (mask[:, t] * inner).astype(F32)).astype(F32)
        out[:, t] = ret
    return out


class LambdaOracleQLearner(OracleQLearner):
    """OracleQLearner with TD(lambda) targets: cfg["td_lambda"] in [0, 1] (0 reproduces the one-step target on every
    unmasked transition)."""

    def forward(self, batch, keep_cache=False, cur_max_override=None, relu_override=None):
        fw = super().forward(batch, keep_cache, cur_max_override, relu_override)
        c = self.cfg
        rew = batch["reward"][:, :-1].astype(F32)
        term = batch["terminated"][:, :-1].astype(F32)
        mask1 = fw["mask"][..., :1]   # the learner's (B, T, 1) mask (expanded over agents without a mixer)
        targets = td_lambda_returns(rew, term, mask1, fw["target_q_tot"], c["gamma"], c["td_lambda"])
        td = (fw["q_tot"] - targets).astype(F32)
        m = fw["mask"]
        mtd = td * m
        msum = fw["mask_sum"]
        hd = F32(c.get("huber_delta", 0.0))
        if hd > 0:
            ax = np.abs(mtd)
            loss = F32(np.where(ax <= hd, F32(0.5) * mtd * mtd, hd * (ax - F32(0.5) * hd)).astype(F32).sum()) / msum
        else:
            loss = F32((mtd * mtd).sum()) / msum
        fw.update(targets=targets, td=td, loss=float(loss))
        return fw
