#!/usr/bin/env python3
"""What the non-shared actor (`agent: rnn_ns`, `mac: non_shared_mac`) costs beside the shared
`use_rnn: False` actor, at the cfg5 shape of bench.py with maa2c.yaml's / mappo.yaml's keys, for one
ActorCriticLearner.train() and one four-epoch PPOLearner.train(): scripts/a2c_ffn_step_time.py's method.

    python scripts/a2c_ns_step_time.py [--epochs 4] [--rounds 6] [--steps 100] [--profile DIR]

Four learners (each learner shared and non-shared) on ONE storage in interleaved rounds of --steps steps of
ReplayBuffer.sample -> train, after one untimed round of the same: the per-step times of every round, their medians and
round-to-round spreads, in microseconds, and the non-shared excess. --profile DIR: in a fresh child process, one
`rocprofv3 --kernel-trace --stats` pass (no counters) over 20 train() calls of the non-shared actor-critic loop.
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
import a2c_ffn_step_time as ffn  # noqa: E402  (the keys, the storage, the profile readers)
from a2c_ffn_step_time import B, KINDS, WARMUP, base, ppo  # noqa: E402


def make_learner(buf, groups, which, epochs, non_shared, seed=0):
    """a2c_ffn_step_time.make_learner's use_rnn: False learner, shared or with one agent per agent index."""
    import logging

    import torch as th
    from pymarl_amd.controllers import REGISTRY as mac_REGISTRY
    from pymarl_amd.learners import REGISTRY as le_REGISTRY
    from pymarl_amd.utils.logging import Logger
    from types import SimpleNamespace as SN
    shared = ffn.make_learner(buf, groups, which, epochs, False, seed)
    if not non_shared:
        return shared
    args = SN(**dict(vars(shared.args), agent="rnn_ns", mac="non_shared_mac"))   # the same keys but these two
    del shared
    th.manual_seed(seed)
    mac = mac_REGISTRY[args.mac](buf.scheme, groups, args)
    learner = le_REGISTRY[which](mac, buf.scheme, Logger(logging.getLogger("a2c_ns_step_time")), args)
    learner.cuda()
    return learner


def child_loop(steps, epochs, which):
    sys.path.insert(0, base.HERE_ROOT)
    import torch as th
    buf, groups = base.make_buffer()
    learner = make_learner(buf, groups, which, epochs, True)
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
    ap.add_argument("--profile", default=None, help="directory for the rocprofv3 --kernel-trace --stats pass")
    ap.add_argument("--loop", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.loop:
        return child_loop(a.steps, a.epochs, a.loop)
    res = dict(shape="cfg5", n_agents=base.N_AGENTS, n_actions=base.N_ACTIONS, T=base.T, batch=B, epochs=a.epochs,
               rounds=a.rounds, steps=a.steps)
    if a.profile:   # before this process opens the GPU: one child at a time
        res["profile"] = {KINDS[0]: profile(os.path.join(a.profile, KINDS[0]), a.epochs, KINDS[0])}
    sys.path.insert(0, base.HERE_ROOT)
    import torch as th
    if not th.cuda.is_available():
        raise SystemExit("a2c_ns_step_time.py needs a HIP device")
    buf, groups = base.make_buffer()
    ls = {(w, ns): make_learner(buf, groups, w, a.epochs, ns) for w in KINDS for ns in (False, True)}
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
        s, n = times[(w, False)], times[(w, True)]
        ms, mn = statistics.median(s), statistics.median(n)
        res[w] = dict(shared_us=s, ns_us=n, shared_median_us=ms, ns_median_us=mn, shared_spread_us=max(s) - min(s),
                      ns_spread_us=max(n) - min(n), excess_us=mn - ms, plan=ls[(w, True)].last_plan())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
