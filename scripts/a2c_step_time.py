#!/usr/bin/env python3
"""What one ActorCriticLearner.train() costs, at the cfg5 shape of bench.py (MMM2: 10 agents, 18 actions, obs 176,
state 322, T = 180, batch 8) with an 8-episode synthetic replay (pymarl_amd/utils/synthetic.py), beside the only other
actor-critic step the project has, COMALearner's, on the same batch. COMA is the reference point, not a target: its
critic takes T dependent optimiser steps per train(), the V critic here one.

    python scripts/a2c_step_time.py [--rounds 6] [--steps 100] [--profile DIR [--min-us 2.5]] [--bench]

Two learners (ActorCriticLearner: cv_critic, Adam; COMALearner) on ONE storage in interleaved rounds of --steps steps
of ReplayBuffer.sample -> train: the per-step times of every round and their medians, in microseconds. Both learners
read their stats back once per train() (one synchronisation each), as in training.
--profile DIR: in a fresh child process, one `rocprofv3 --kernel-trace --stats` pass (no counters) over 20 steps of the
    actor-critic loop: calls per step and mean duration of every kernel (--min-us X: of those that take X us a step
    and more), and the launches and kernel time per step over all of them.
--bench: the default `bench.py --gpus 1` line of this tree, from a fresh child process (the Q path's figure).
Prints one JSON line. Needs a HIP device: there is no CPU path.
"""
import argparse
import csv
import gc
import glob
import json
import logging
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace as SN

HERE_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_AGENTS, N_ACTIONS, OBS, STATE, T, B = 10, 18, 176, 322, 180, 8   # bench.py CONFIGS["cfg5"]
WARMUP = 10


def make_buffer(seed=0):
    import torch as th
    from pymarl_amd.components.episode_buffer import ReplayBuffer
    from pymarl_amd.components.transforms import OneHot
    from pymarl_amd.utils.synthetic import make_replay
    n, A, O, S = N_AGENTS, N_ACTIONS, OBS, STATE
    scheme = {
        "state": {"vshape": S},
        "obs": {"vshape": O, "group": "agents"},
        "actions": {"vshape": (1,), "group": "agents", "dtype": th.long},
        "avail_actions": {"vshape": (A,), "group": "agents", "dtype": th.int},
        "reward": {"vshape": (1,)},
        "terminated": {"vshape": (1,), "dtype": th.uint8},
    }
    groups = {"agents": n}
    buf = ReplayBuffer(scheme, groups, B, T + 1, preprocess={"actions": ("actions_onehot", [OneHot(A)])},
                       device="cuda")
    buf.load_arrays(make_replay(B, T, n, A, O, S, seed=seed))
    return buf, groups


def make_learner(buf, groups, which, seed=0):
    import torch as th
    from pymarl_amd.controllers import REGISTRY as mac_REGISTRY
    from pymarl_amd.learners import REGISTRY as le_REGISTRY
    from pymarl_amd.utils.logging import Logger
    args = SN(n_agents=N_AGENTS, n_actions=N_ACTIONS, state_shape=STATE, obs_shape=OBS, rnn_hidden_dim=64, lr=5e-4,
              critic_lr=5e-4, optim_alpha=0.99, optim_eps=1e-5, grad_norm_clip=10.0, gamma=0.99, td_lambda=0.8,
              target_update_interval=200, learner_log_interval=10 ** 12, obs_last_action=True, obs_agent_id=True,
              agent="rnn", mac="basic_mac", agent_output_type="pi_logits", mask_before_softmax=True, batch_size=B,
              device="cuda", use_cuda=True)
    if which == "a2c":
        args.__dict__.update(learner="actor_critic_learner", action_selector="soft_policies", critic_type="cv_critic",
                             hidden_dim=128, q_nstep=5, add_value_last_step=True, entropy_coef=0.01, optimizer="adam",
                             standardise_rewards=True, target_update_interval_or_tau=0.01)
    else:
        args.__dict__.update(learner="coma_learner", action_selector="multinomial", epsilon_start=0.5,
                             epsilon_finish=0.01, epsilon_anneal_time=100000)
    th.manual_seed(seed)
    mac = mac_REGISTRY["basic_mac"](buf.scheme, groups, args)
    learner = le_REGISTRY[args.learner](mac, buf.scheme, Logger(logging.getLogger("a2c_step_time")), args)
    learner.cuda()
    return learner


def steps_of(buf, learner, steps, k0):
    for k in range(steps):
        b = buf.sample(B)
        learner.train(b[:, :b.max_t_filled()], 1000 * (k0 + k), k0 + k)


def timed(buf, learner, steps, k0):
    import torch as th
    th.cuda.synchronize()
    t0 = time.perf_counter()
    steps_of(buf, learner, steps, k0)
    th.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def child_loop(steps):
    """--loop: WARMUP and `steps` steps of the actor-critic loop, for the rocprofv3 pass. The library handle is
    released before the interpreter exits (bench.py does the same: a profiler's interception layer is still up)."""
    sys.path.insert(0, HERE_ROOT)
    import torch as th
    buf, groups = make_buffer()
    learner = make_learner(buf, groups, "a2c")
    steps_of(buf, learner, WARMUP + steps, 0)
    th.cuda.synchronize()
    learner._handle = None
    del learner
    gc.collect()


def kernel_stats(outdir):
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no kernel_stats.csv under {}".format(outdir))
    out = {}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            out[row["Name"]] = dict(calls=int(row["Calls"]), mean_us=float(row["AverageNs"]) / 1e3)
    return out


def short(name):
    """A kernel's name without its argument list (templates kept: they tell the GEMM policies apart)."""
    depth, out = 0, []
    for ch in name:
        if ch == "(" and depth == 0:
            break
        depth += ch == "<"
        depth -= ch == ">"
        out.append(ch)
    return "".join(out).replace("void ", "").replace("mq::", "")


def profile(outdir, min_us=0.0, steps=20):
    os.makedirs(outdir, exist_ok=True)
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--",
                    sys.executable, os.path.abspath(__file__), "--loop", "--steps", str(steps)],
                   check=True, stdout=subprocess.DEVNULL, timeout=600)
    st = kernel_stats(outdir)
    n = WARMUP + steps
    rows = sorted(((short(k), v["calls"] / n, v["mean_us"]) for k, v in st.items()), key=lambda r: -r[1] * r[2])
    return dict(steps=n, min_us=min_us,
                kernels=[dict(name=k, calls_per_step=round(c, 3), mean_us=round(u, 2), us_per_step=round(c * u, 2))
                         for k, c, u in rows if c * u >= min_us],
                launches_per_step=round(sum(c for _, c, _ in rows), 2),
                kernel_sum_us_per_step=round(sum(c * u for _, c, u in rows), 1))


def bench_line():
    out = subprocess.run([sys.executable, os.path.join(HERE_ROOT, "bench.py"), "--gpus", "1"], check=True,
                         capture_output=True, text=True, timeout=900, cwd=HERE_ROOT)
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--profile", default=None, help="directory for the rocprofv3 --kernel-trace --stats pass")
    ap.add_argument("--min-us", type=float, default=0.0, help="list only the kernels of this many us a step and more")
    ap.add_argument("--bench", action="store_true", help="also take the default bench.py line")
    ap.add_argument("--loop", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.loop:
        return child_loop(a.steps)
    res = dict(shape="cfg5", n_agents=N_AGENTS, n_actions=N_ACTIONS, T=T, batch=B, rounds=a.rounds, steps=a.steps)
    if a.profile:   # before this process opens the GPU: one child at a time
        res["profile"] = profile(a.profile, a.min_us)
    if a.bench:
        res["bench"] = bench_line()
    sys.path.insert(0, HERE_ROOT)
    import torch as th
    if not th.cuda.is_available():
        raise SystemExit("a2c_step_time.py needs a HIP device")
    buf, groups = make_buffer()
    a2c, coma = make_learner(buf, groups, "a2c"), make_learner(buf, groups, "coma")
    steps_of(buf, a2c, WARMUP, 0)
    steps_of(buf, coma, WARMUP, 0)
    ta, tc = [], []
    k0 = WARMUP
    for _ in range(a.rounds):
        ta.append(timed(buf, a2c, a.steps, k0))
        tc.append(timed(buf, coma, a.steps, k0))
        k0 += a.steps
    res.update(a2c_us=ta, coma_us=tc, a2c_median_us=statistics.median(ta), coma_median_us=statistics.median(tc),
               a2c_spread_us=max(ta) - min(ta), coma_spread_us=max(tc) - min(tc), plan=a2c.last_plan(),
               coma_critic_path=coma.critic_path())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
