#!/usr/bin/env python3
"""What the Adam opt-in (optimizer: adam) costs per train step, and whether the RMSprop step is what it was, on the cfg2
shape of bench.py (QMIX, 8 agents, T = 120, batch 32) with a 128-episode synthetic replay, as
scripts/hyper2_step_time.py measures the two-layer hypernet (its buffer, loops and timer are reused).

    python scripts/adam_step_time.py [--rounds 6] [--steps 100] [--ab PARENT_TREE] [--profile DIR]

(b) Two learners, RMSprop and Adam, on ONE storage in interleaved rounds of --steps steps of ReplayBuffer.sample ->
    train, synchronising only at round ends: the per-step times of every round and Adam minus RMSprop in microseconds
    (medians). Then, with the rounds over, 50 steps of each with HIP events around the `apply` phase alone
    (mq_set_timing / mq_phase_times): the mean time of the step's last launch under each optimiser.
(a) --ab PARENT_TREE: the RMSprop step of this tree against the same step of another checkout with its own built
    library (PARENT_TREE/pymarl_amd/lib/libmq_learner.so), each round a fresh child process, alternating parent / new;
    the difference of the medians beside each side's own round-to-round spread.
--profile DIR: in fresh child processes, one `rocprofv3 --kernel-trace --stats` pass (no counters) over 20 steps of
    each loop: the mean duration of `apply_adam_kernel` beside `apply_kernel`'s.
Prints one JSON line. Needs a HIP device: there is no CPU path.
"""
import argparse
import json
import logging
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace as SN

HERE = os.path.dirname(os.path.abspath(__file__))
HERE_ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

from hyper2_step_time import (B, MIXER, N_ACTIONS, N_AGENTS, OBS, STATE, kernel_stats, make_buffer,  # noqa: E402
                              steps_of, timed, use_tree)

PHASE_STEPS = 50


def make_learner(buf, groups, optimizer, seed=0):
    import torch as th
    from pymarl_amd.controllers import REGISTRY as mac_REGISTRY
    from pymarl_amd.learners import REGISTRY as le_REGISTRY
    from pymarl_amd.utils.logging import Logger
    args = SN(n_agents=N_AGENTS, n_actions=N_ACTIONS, state_shape=STATE, obs_shape=OBS, rnn_hidden_dim=64,
              mixing_embed_dim=32, mixer=MIXER, lr=5e-4, optim_alpha=0.99, optim_eps=1e-5, grad_norm_clip=10.0,
              gamma=0.99, double_q=True, target_update_interval=200, learner_log_interval=10 ** 12,
              obs_last_action=True, obs_agent_id=True, agent="rnn", mac="basic_mac", agent_output_type="q",
              action_selector="epsilon_greedy", epsilon_start=1.0, epsilon_finish=0.05, epsilon_anneal_time=50000,
              batch_size=B, learner="q_learner", device="cuda", use_cuda=True)
    if optimizer is not None:   # None: no key at all (a parent tree's learner does not know it)
        args.optimizer = optimizer
    th.manual_seed(seed)
    mac = mac_REGISTRY["basic_mac"](buf.scheme, groups, args)
    learner = le_REGISTRY["q_learner"](mac, buf.scheme, Logger(logging.getLogger("adam_step_time")), args)
    learner.cuda()
    return learner


def child_rmsprop(root, steps):
    """--child: one round of the RMSprop loop from the tree `root`; prints its per-step microseconds."""
    use_tree(root)
    buf, groups = make_buffer()
    learner = make_learner(buf, groups, None)
    steps_of(buf, learner, 10, 0)
    print(json.dumps(dict(us=timed(buf, learner, steps, 10), plan=learner.last_plan())))


def child_loop(optimizer, steps):
    """--loop: 10 warm-up and `steps` steps of one loop, for the rocprofv3 pass."""
    use_tree(HERE_ROOT)
    import torch as th
    buf, groups = make_buffer()
    steps_of(buf, make_learner(buf, groups, optimizer), 10 + steps, 0)
    th.cuda.synchronize()


def profile(outdir, steps=20):
    res = {}
    for opt in ("adam", "rmsprop"):
        d = os.path.join(outdir, opt)
        os.makedirs(d, exist_ok=True)
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
                        sys.executable, os.path.abspath(__file__), "--loop", opt, "--steps", str(steps)],
                       check=True, stdout=subprocess.DEVNULL, timeout=600)
        st = kernel_stats(d)
        res[opt] = {k: v for k, v in st.items() if any(w in k for w in ("apply_", "red_pass", "sumsq"))}
        res[opt + "_step_kernel_sum_us"] = sum(v["calls"] * v["mean_us"] for v in st.values()) / (10 + steps)
    return res


def run_child(argv):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, check=True, capture_output=True, text=True,
                         timeout=300)
    return json.loads(out.stdout.strip().splitlines()[-1])


def ab(parent, rounds, steps):
    old, new = [], []
    for _ in range(rounds):
        old.append(run_child(["--child", os.path.abspath(parent), "--steps", str(steps)])["us"])
        new.append(run_child(["--child", HERE_ROOT, "--steps", str(steps)])["us"])
    return dict(parent_us=old, new_us=new, parent_median_us=statistics.median(old),
                new_median_us=statistics.median(new),
                new_minus_parent_us=statistics.median(new) - statistics.median(old),
                parent_spread_us=max(old) - min(old), new_spread_us=max(new) - min(new))


def apply_phase_us(buf, learner, k0):
    """Mean microseconds of the `apply` phase over PHASE_STEPS steps (events around that phase only)."""
    import torch as th
    learner.set_timing(PHASE_STEPS, ["apply"])
    steps_of(buf, learner, PHASE_STEPS, k0)
    th.cuda.synchronize()
    us = learner.phase_times()["apply"] * 1e3
    learner.set_timing(0)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--ab", default=None, help="another checkout (built) to A/B the RMSprop step against")
    ap.add_argument("--profile", default=None, help="directory for the rocprofv3 --kernel-trace --stats passes")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--loop", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child_rmsprop(a.child, a.steps)
    if a.loop:
        return child_loop(a.loop, a.steps)
    res = dict(shape="cfg2", rounds=a.rounds, steps=a.steps)
    if a.ab:   # before this process opens the GPU: one child at a time
        res["rmsprop_ab"] = ab(a.ab, a.rounds, a.steps)
    if a.profile:
        res["kernels"] = profile(a.profile)
    use_tree(HERE_ROOT)
    import torch as th
    if not th.cuda.is_available():
        raise SystemExit("adam_step_time.py needs a HIP device")
    buf, groups = make_buffer()
    rms, adam = make_learner(buf, groups, "rmsprop"), make_learner(buf, groups, "adam")
    steps_of(buf, rms, 10, 0)
    steps_of(buf, adam, 10, 0)
    assert type(adam.optimiser) is th.optim.Adam and type(rms.optimiser) is th.optim.RMSprop
    assert int(adam._handle.lib.mq_opt_step(adam._handle.h)) == 10 and float(adam._m.abs().max()) > 0
    t1, t2 = [], []
    k0 = 10
    for _ in range(a.rounds):
        t1.append(timed(buf, rms, a.steps, k0))
        t2.append(timed(buf, adam, a.steps, k0))
        k0 += a.steps
    res.update(n_params=rms.n_params, rmsprop_us=t1, adam_us=t2, rmsprop_median_us=statistics.median(t1),
               adam_median_us=statistics.median(t2),
               adam_minus_rmsprop_us=statistics.median(t2) - statistics.median(t1),
               rmsprop_spread_us=max(t1) - min(t1), adam_spread_us=max(t2) - min(t2),
               apply_phase_rmsprop_us=apply_phase_us(buf, rms, k0), apply_phase_adam_us=apply_phase_us(buf, adam, k0),
               plan=adam.last_plan())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
