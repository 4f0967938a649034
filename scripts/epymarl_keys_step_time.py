#!/usr/bin/env python3
"""What epymarl's two learner keys cost per train step, and whether the step without them is what it was, on the cfg2
shape of bench.py (QMIX, 8 agents, T = 120, batch 32) with a 128-episode synthetic replay, as scripts/adam_step_time.py
measures the Adam opt-in (hyper2_step_time.py's buffer, loops and timer are reused).

    python scripts/epymarl_keys_step_time.py [--rounds 5] [--steps 100] [--ab PARENT_TREE]

Rounds of --steps steps of ReplayBuffer.sample -> train, synchronising only at round ends, each round a fresh child
process, the configurations alternating within every pass:
    parent   the same loop from another checkout with its own built library (--ab PARENT_TREE, optional)
    off      this tree, both keys absent
    soft     target_update_interval_or_tau: 0.01
    std      standardise_rewards: True
    both     the two together
Per configuration: every round's per-step microseconds, the median, the spread, and the median's difference to `off`
(for `off`: to `parent`). Then, in this process, 50 steps of each of off / soft / std with HIP events around one phase
(mq_set_timing / mq_phase_times): `apply` (the optimiser's launch, and the soft update behind it) and `mix` (the mixer
tail, and reward_norm_kernel in front of it), so each new launch's cost stands beside the launch it joins.
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

from hyper2_step_time import (B, MIXER, N_ACTIONS, N_AGENTS, OBS, STATE, make_buffer, steps_of, timed,  # noqa: E402
                              use_tree)

PHASE_STEPS = 50
KEYS = {
    "parent": {},
    "off": {},
    "soft": dict(target_update_interval_or_tau=0.01),
    "std": dict(standardise_rewards=True),
    "both": dict(target_update_interval_or_tau=0.01, standardise_rewards=True),
}


def make_learner(buf, groups, keys, seed=0):
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
    for k, v in keys.items():   # none for `off` and `parent` (a parent tree's learner does not know the keys)
        setattr(args, k, v)
    th.manual_seed(seed)
    mac = mac_REGISTRY["basic_mac"](buf.scheme, groups, args)
    learner = le_REGISTRY["q_learner"](mac, buf.scheme, Logger(logging.getLogger("epymarl_keys_step_time")), args)
    learner.cuda()
    return learner


def child(root, config, steps):
    """--child ROOT --config NAME: one round of one configuration from the tree ROOT; prints its per-step microseconds."""
    use_tree(root)
    buf, groups = make_buffer()
    learner = make_learner(buf, groups, KEYS[config])
    steps_of(buf, learner, 10, 0)
    plan = learner.last_plan()
    print(json.dumps(dict(us=timed(buf, learner, steps, 10), reward_norm=plan.get("reward_norm"),
                          soft_target=plan.get("soft_target"))))


def run_child(root, config, steps):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(root), "--config",
                          config, "--steps", str(steps)], check=True, capture_output=True, text=True, timeout=300)
    return json.loads(out.stdout.strip().splitlines()[-1])


def phase_us(buf, learner, phase, k0):
    """Mean microseconds of one phase over PHASE_STEPS steps (events around that phase only)."""
    import torch as th
    learner.set_timing(PHASE_STEPS, [phase])
    steps_of(buf, learner, PHASE_STEPS, k0)
    th.cuda.synchronize()
    us = learner.phase_times()[phase] * 1e3
    learner.set_timing(0)
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--ab", default=None, help="the parent commit's checkout (built), for the `parent` rounds")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--config", default="off", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.config, a.steps)
    configs = (["parent"] if a.ab else []) + ["off", "soft", "std", "both"]
    us = {c: [] for c in configs}
    for _ in range(a.rounds):   # before this process opens the GPU: one child at a time
        for c in configs:
            r = run_child(a.ab if c == "parent" else HERE_ROOT, c, a.steps)
            if c != "parent":
                want = (int("standardise_rewards" in KEYS[c]), int("target_update_interval_or_tau" in KEYS[c]))
                assert (r["reward_norm"], r["soft_target"]) == want, (c, r)
            us[c].append(r["us"])
    res = dict(shape="cfg2", rounds=a.rounds, steps=a.steps)
    med = {c: statistics.median(v) for c, v in us.items()}
    for c in configs:
        base = "parent" if c == "off" else "off"
        res[c] = dict(us=us[c], median_us=med[c], spread_us=max(us[c]) - min(us[c]))
        if c != "parent" and base in med:
            res[c]["minus_{}_us".format(base)] = med[c] - med[base]
    use_tree(HERE_ROOT)
    import torch as th
    if not th.cuda.is_available():
        raise SystemExit("epymarl_keys_step_time.py needs a HIP device")
    buf, groups = make_buffer()
    phases = {}
    for c, phase in (("off", "apply"), ("soft", "apply"), ("off", "mix"), ("std", "mix")):
        learner = make_learner(buf, groups, KEYS[c])
        steps_of(buf, learner, 10, 0)
        phases["{}_{}_us".format(phase, c)] = phase_us(buf, learner, phase, 10)
        del learner
    phases["soft_update_launch_us"] = phases["apply_soft_us"] - phases["apply_off_us"]
    phases["reward_norm_launch_us"] = phases["mix_std_us"] - phases["mix_off_us"]
    res["phases"] = phases
    print(json.dumps(res))


if __name__ == "__main__":
    main()
