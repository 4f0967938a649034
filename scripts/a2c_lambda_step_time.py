#!/usr/bin/env python3
"""What TD(lambda) critic targets (`q_targets: td_lambda`) cost beside the n-step return, at the cfg5
shape of bench.py with scripts/a2c_ffn_step_time.py's storage, keys and method (maa2c.yaml's / mappo.yaml's keys,
`use_rnn: False`), for one ActorCriticLearner.train() and one four-epoch PPOLearner.train().

    python scripts/a2c_lambda_step_time.py [--epochs 4] [--rounds 6] [--steps 100] [--td-lambda 0.8]

Four learners (each learner under the n-step return and under lambda-returns) on ONE storage and one library in
interleaved rounds of --steps steps of ReplayBuffer.sample -> train, after one untimed round of the same: the per-step
times of every round, their medians and round-to-round spreads, in microseconds. The n-step step is the scale, not a
bound: a2c_lambda_kernel's scan is T = 180 dependent steps a lane, a2c_nstep_kernel's q_nstep + 1 = 6.
Prints one JSON line. Needs a HIP device: there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import a2c_ffn_step_time as ffn  # noqa: E402  (the keys)
import a2c_step_time as base  # noqa: E402  (the shape, the storage)
import ppo_step_time as ppo  # noqa: E402  (the timed loop)

WARMUP, KINDS, RETURNS = base.WARMUP, ffn.KINDS, ("nstep", "lambda")


def make_learner(buf, groups, which, epochs, td_lambda):
    """a2c_ffn_step_time's feed-forward learner; td_lambda not None: rebuilt from its args with the two keys."""
    learner = ffn.make_learner(buf, groups, which, epochs, False)
    if td_lambda is None:
        return learner
    import logging

    from pymarl_amd.controllers import REGISTRY as mac_REGISTRY
    from pymarl_amd.learners import REGISTRY as le_REGISTRY
    from pymarl_amd.utils.logging import Logger
    args = learner.args
    args.q_targets, args.td_lambda = "td_lambda", td_lambda
    mac = mac_REGISTRY["basic_mac"](buf.scheme, groups, args)
    lam = le_REGISTRY[which](mac, buf.scheme, Logger(logging.getLogger("a2c_lambda_step_time")), args)
    lam.cuda()
    return lam


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--td-lambda", type=float, default=0.8)
    a = ap.parse_args()
    res = dict(shape="cfg5", n_agents=base.N_AGENTS, n_actions=base.N_ACTIONS, T=base.T, batch=base.B, epochs=a.epochs,
               rounds=a.rounds, steps=a.steps, td_lambda=a.td_lambda)
    sys.path.insert(0, base.HERE_ROOT)
    import torch as th
    if not th.cuda.is_available():
        raise SystemExit("a2c_lambda_step_time.py needs a HIP device")
    buf, groups = base.make_buffer()
    ls = {(w, r): make_learner(buf, groups, w, a.epochs, a.td_lambda if r == "lambda" else None)
          for w in KINDS for r in RETURNS}
    for le in ls.values():
        ppo.units_of(buf, le, WARMUP, 0, 1)
    for (w, r), le in ls.items():
        assert le.last_returns() == RETURNS.index(r), (w, r)
    for le in ls.values():   # one untimed interleaved round: the timed windows' own order, once
        ppo.timed(buf, le, a.steps, WARMUP, 1)
    times = {k: [] for k in ls}
    k0 = WARMUP + a.steps
    for _ in range(a.rounds):
        for k, le in ls.items():
            times[k].append(ppo.timed(buf, le, a.steps, k0, 1))
        k0 += a.steps
    for w in KINDS:
        out = {}
        for r in RETURNS:
            t = times[(w, r)]
            out[r + "_us"] = t
            out[r + "_median_us"] = statistics.median(t)
            out[r + "_spread_us"] = max(t) - min(t)
        out["added_us"] = out["lambda_median_us"] - out["nstep_median_us"]
        res[w] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
