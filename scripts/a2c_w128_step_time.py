#!/usr/bin/env python3
"""What the feed-forward actor costs at hidden width 128 (`hidden_dim: 128` with no `rnn_hidden_dim`, what epymarl's
tuned maa2c / mappo configs ship) beside the width-64 fused actor (§3m), at the cfg5 shape of bench.py
with scripts/a2c_ffn_step_time.py's storage, keys and method, for one ActorCriticLearner.train() and one four-epoch
PPOLearner.train().

    python scripts/a2c_w128_step_time.py [--epochs 4] [--rounds 6] [--steps 100] [--profile DIR]

Four learners (each learner at width 64 and at width 128; the critic is 128 wide in all four) on ONE storage and one
library in interleaved rounds of --steps steps of ReplayBuffer.sample -> train, after one untimed round of the same:
the per-step times of every round, their medians and round-to-round spreads, in microseconds. The width-64 step is the
scale, not a bound: the wide actor does about 3x its MFMA work. --profile DIR: in a fresh child process each, one
`rocprofv3 --kernel-trace --stats` pass (no counters) over 20 train() calls of the width-128 actor-critic and PPO
loops: launches per train(), every kernel's calls and mean duration.
Prints one JSON line. Needs a HIP device: there is no CPU path.
"""
import argparse
import gc
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import a2c_ffn_step_time as ffn  # noqa: E402  (the keys)
import a2c_step_time as base  # noqa: E402  (the shape, the storage, the profile readers)
import ppo_step_time as ppo  # noqa: E402  (the timed loop)

WARMUP, KINDS, WIDTHS = base.WARMUP, ffn.KINDS, (64, 128)


def make_learner(buf, groups, which, epochs, width):
    """a2c_ffn_step_time's feed-forward learner; at width 128 rebuilt from epymarl's args (hidden_dim alone)."""
    learner = ffn.make_learner(buf, groups, which, epochs, False)
    if width == 64:
        return learner
    import logging

    from pymarl_amd.controllers import REGISTRY as mac_REGISTRY
    from pymarl_amd.learners import REGISTRY as le_REGISTRY
    from pymarl_amd.utils.logging import Logger
    args = learner.args
    args.rnn_hidden_dim = None
    mac = mac_REGISTRY["basic_mac"](buf.scheme, groups, args)
    wide = le_REGISTRY[which](mac, buf.scheme, Logger(logging.getLogger("a2c_w128_step_time")), args)
    wide.cuda()
    assert mac.agent.hidden_dim == 128
    return wide


def child_loop(steps, epochs, which):
    sys.path.insert(0, base.HERE_ROOT)
    import torch as th
    buf, groups = base.make_buffer()
    learner = make_learner(buf, groups, which, epochs, 128)
    ppo.units_of(buf, learner, WARMUP + steps, 0, 1)
    th.cuda.synchronize()
    learner._handle = None
    del learner
    gc.collect()


def profile(outdir, epochs, which, steps=20):
    import subprocess
    os.makedirs(outdir, exist_ok=True)
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--",
                    sys.executable, os.path.abspath(__file__), "--loop", which, "--steps", str(steps), "--epochs",
                    str(epochs)], check=True, stdout=subprocess.DEVNULL, timeout=600)
    n = WARMUP + steps
    rows = sorted(((base.short(k), v["calls"] / n, v["mean_us"]) for k, v in base.kernel_stats(outdir).items()),
                  key=lambda r: -r[1] * r[2])
    return dict(trains=n, launches_per_train=round(sum(c for _, c, _ in rows), 2),
                kernel_sum_us_per_train=round(sum(c * u for _, c, u in rows), 1),
                kernels=[dict(name=k, calls_per_train=round(c, 3), mean_us=round(u, 2)) for k, c, u in rows])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--profile", default=None, help="directory for the two rocprofv3 --kernel-trace --stats passes")
    ap.add_argument("--loop", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.loop:
        return child_loop(a.steps, a.epochs, a.loop)
    res = dict(shape="cfg5", n_agents=base.N_AGENTS, n_actions=base.N_ACTIONS, T=base.T, batch=base.B, epochs=a.epochs,
               rounds=a.rounds, steps=a.steps)
    if a.profile:   # before this process opens the GPU: one child at a time
        res["profile"] = {w: profile(os.path.join(a.profile, w), a.epochs, w) for w in KINDS}
    sys.path.insert(0, base.HERE_ROOT)
    import torch as th
    if not th.cuda.is_available():
        raise SystemExit("a2c_w128_step_time.py needs a HIP device")
    buf, groups = base.make_buffer()
    ls = {(w, width): make_learner(buf, groups, w, a.epochs, width) for w in KINDS for width in WIDTHS}
    for le in ls.values():
        ppo.units_of(buf, le, WARMUP, 0, 1)
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
        for width in WIDTHS:
            t = times[(w, width)]
            out["w{}_us".format(width)] = t
            out["w{}_median_us".format(width)] = statistics.median(t)
            out["w{}_spread_us".format(width)] = max(t) - min(t)
        out["added_us"] = out["w128_median_us"] - out["w64_median_us"]
        out["plan"] = ls[(w, 128)].last_plan()
        res[w] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
