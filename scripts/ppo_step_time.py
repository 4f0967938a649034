#!/usr/bin/env python3
"""What one PPOLearner.train() costs, at the cfg5 shape of bench.py (MMM2: 10 agents, 18 actions, obs 176, state 322,
T = 180, batch 8) with an 8-episode synthetic replay, beside what it replaces: `epochs` ActorCriticLearner.train()
calls on the same batch. Both learners run mappo.yaml's keys (cv_critic of width 128, Adam, reward standardisation,
soft target update); the yardstick is the actor-critic learner measured in the same run, not a recorded figure.

    python scripts/ppo_step_time.py [--epochs 4] [--rounds 6] [--steps 100] [--profile DIR [--min-us 2.5]] [--bench]

Two learners on ONE storage in interleaved rounds of --steps units; a unit is ReplayBuffer.sample, then one PPO
train() or `epochs` actor-critic train() calls on that batch. Per-unit times of every round and their medians, in
microseconds; `faster` is true when the PPO median is below the actor-critic one by more than the larger of the two
round-to-round spreads. Both learners read their stats back once per train(): one synchronisation per unit for PPO,
`epochs` for the actor-critic calls.
--profile DIR: in a fresh child process, one `rocprofv3 --kernel-trace --stats` pass (no counters) over 20 PPO
    train() calls: kernel launches per train() and every kernel's calls and mean duration.
--bench: the default `bench.py --gpus 1` line of this tree, from a fresh child process (the Q path's figure).
Prints one JSON line. Needs a HIP device: there is no CPU path.
"""
import argparse
import gc
import json
import logging
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace as SN

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import a2c_step_time as base  # noqa: E402  (the shape, the storage, the profile readers)

B, WARMUP = base.B, base.WARMUP


def make_learner(buf, groups, which, epochs, seed=0):
    import torch as th
    from pymarl_amd.controllers import REGISTRY as mac_REGISTRY
    from pymarl_amd.learners import REGISTRY as le_REGISTRY
    from pymarl_amd.utils.logging import Logger
    args = SN(n_agents=base.N_AGENTS, n_actions=base.N_ACTIONS, state_shape=base.STATE, obs_shape=base.OBS,
              rnn_hidden_dim=64, lr=5e-4, optim_alpha=0.99, optim_eps=1e-5, grad_norm_clip=10.0, gamma=0.99,
              target_update_interval=200, learner_log_interval=10 ** 12, obs_last_action=True, obs_agent_id=True,
              agent="rnn", mac="basic_mac", agent_output_type="pi_logits", mask_before_softmax=True, batch_size=B,
              device="cuda", use_cuda=True, action_selector="soft_policies", critic_type="cv_critic", hidden_dim=128,
              q_nstep=5, add_value_last_step=True, entropy_coef=0.001, optimizer="adam", standardise_rewards=True,
              target_update_interval_or_tau=0.01, learner=which)
    if which == "ppo_learner":
        args.__dict__.update(epochs=epochs, eps_clip=0.2)
    th.manual_seed(seed)
    mac = mac_REGISTRY["basic_mac"](buf.scheme, groups, args)
    learner = le_REGISTRY[which](mac, buf.scheme, Logger(logging.getLogger("ppo_step_time")), args)
    learner.cuda()
    return learner


def units_of(buf, learner, units, k0, calls):
    for k in range(units):
        b = buf.sample(B)
        b = b[:, :b.max_t_filled()]
        for _ in range(calls):
            learner.train(b, 1000 * (k0 + k), k0 + k)


def timed(buf, learner, units, k0, calls):
    import torch as th
    th.cuda.synchronize()
    t0 = time.perf_counter()
    units_of(buf, learner, units, k0, calls)
    th.cuda.synchronize()
    return (time.perf_counter() - t0) / units * 1e6


def child_loop(steps, epochs):
    """--loop: WARMUP and `steps` PPO train() calls, for the rocprofv3 pass. The library handle is released before the
    interpreter exits (a profiler's interception layer is still up)."""
    sys.path.insert(0, base.HERE_ROOT)
    import torch as th
    buf, groups = base.make_buffer()
    learner = make_learner(buf, groups, "ppo_learner", epochs)
    units_of(buf, learner, WARMUP + steps, 0, 1)
    th.cuda.synchronize()
    learner._handle = learner._ppo_handle = None
    del learner
    gc.collect()


def profile(outdir, epochs, min_us=0.0, steps=20):
    os.makedirs(outdir, exist_ok=True)
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--",
                    sys.executable, os.path.abspath(__file__), "--loop", "--steps", str(steps), "--epochs",
                    str(epochs)], check=True, stdout=subprocess.DEVNULL, timeout=600)
    st = base.kernel_stats(outdir)
    n = WARMUP + steps
    rows = sorted(((base.short(k), v["calls"] / n, v["mean_us"]) for k, v in st.items()), key=lambda r: -r[1] * r[2])
    return dict(trains=n, min_us=min_us,
                kernels=[dict(name=k, calls_per_train=round(c, 3), mean_us=round(u, 2), us_per_train=round(c * u, 2))
                         for k, c, u in rows if c * u >= min_us],
                launches_per_train=round(sum(c for _, c, _ in rows), 2),
                kernel_sum_us_per_train=round(sum(c * u for _, c, u in rows), 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--profile", default=None, help="directory for the rocprofv3 --kernel-trace --stats pass")
    ap.add_argument("--min-us", type=float, default=0.0, help="list only the kernels of this many us a train() and more")
    ap.add_argument("--bench", action="store_true", help="also take the default bench.py line")
    ap.add_argument("--loop", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.loop:
        return child_loop(a.steps, a.epochs)
    res = dict(shape="cfg5", n_agents=base.N_AGENTS, n_actions=base.N_ACTIONS, T=base.T, batch=B, epochs=a.epochs,
               rounds=a.rounds, steps=a.steps)
    if a.profile:   # before this process opens the GPU: one child at a time
        res["profile"] = profile(a.profile, a.epochs, a.min_us)
    if a.bench:
        res["bench"] = base.bench_line()
    sys.path.insert(0, base.HERE_ROOT)
    import torch as th
    if not th.cuda.is_available():
        raise SystemExit("ppo_step_time.py needs a HIP device")
    buf, groups = base.make_buffer()
    ppo = make_learner(buf, groups, "ppo_learner", a.epochs)
    a2c = make_learner(buf, groups, "actor_critic_learner", a.epochs)
    units_of(buf, ppo, WARMUP, 0, 1)
    units_of(buf, a2c, WARMUP, 0, a.epochs)
    tp, ta = [], []
    k0 = WARMUP
    for _ in range(a.rounds):
        tp.append(timed(buf, ppo, a.steps, k0, 1))
        ta.append(timed(buf, a2c, a.steps, k0, a.epochs))
        k0 += a.steps
    mp, ma = statistics.median(tp), statistics.median(ta)
    sp, sa = max(tp) - min(tp), max(ta) - min(ta)
    plan = ppo.last_plan()
    res.update(ppo_us=tp, a2c_x_epochs_us=ta, ppo_median_us=mp, a2c_x_epochs_median_us=ma, ppo_spread_us=sp,
               a2c_x_epochs_spread_us=sa, saved_us=ma - mp, saved_share=(ma - mp) / ma, faster=(ma - mp) > max(sp, sa),
               plan=plan, hoisted_launches_and_copies=plan["hoisted"], clip_frac=ppo.last_stats()["clip_frac"])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
