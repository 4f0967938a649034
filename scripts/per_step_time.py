#!/usr/bin/env python3
"""What prioritized replay costs per train step: the uniform loop (ReplayBuffer.sample -> train) against the PER loop
(PrioritizedReplayBuffer.sample -> train: sampler kernel, weighted mixer tail, priority write-back) on the cfg2 shape
of bench.py (QMIX, 8 agents, T = 120, batch 32) with a 5000-episode synthetic replay (pymarl_amd/utils/synthetic.py).

    python scripts/per_step_time.py [--rounds 6] [--steps 100] [--profile DIR]

Both loops run on ONE learner and one storage, in interleaved rounds of --steps steps, synchronising only at round
ends; prints one JSON line with the per-step times of every round and PER - uniform in microseconds (median of the
rounds). --profile DIR starts, in a fresh child process, one `rocprofv3 --kernel-trace --stats` pass over 20 steps of
each loop (no counters) and adds the mean duration of the sampler, the PER tail, the priority kernel, the plain tail
and the smallest kernel of the trace. Needs a HIP device: there is no CPU path.
"""
import argparse
import csv
import glob
import json
import logging
import os
import re
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace as SN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MIXER, N_AGENTS, N_ACTIONS, OBS, STATE, T, B = "qmix", 8, 14, 80, 168, 120, 32   # bench.py CONFIGS["cfg2"]


def build(n_episodes=5000, unique=512, seed=0, alpha=0.6, beta=0.4):
    import torch as th
    from pymarl_amd.components.episode_buffer import PrioritizedReplayBuffer
    from pymarl_amd.components.transforms import OneHot
    from pymarl_amd.controllers import REGISTRY as mac_REGISTRY
    from pymarl_amd.learners import REGISTRY as le_REGISTRY
    from pymarl_amd.utils.logging import Logger
    from pymarl_amd.utils.synthetic import make_replay

    n, A, O, S = N_AGENTS, N_ACTIONS, OBS, STATE
    args = SN(n_agents=n, n_actions=A, state_shape=S, obs_shape=O, rnn_hidden_dim=64, mixing_embed_dim=32,
              mixer=MIXER, lr=5e-4, optim_alpha=0.99, optim_eps=1e-5, grad_norm_clip=10.0, gamma=0.99,
              double_q=True, target_update_interval=200, learner_log_interval=10 ** 12, obs_last_action=True,
              obs_agent_id=True, agent="rnn", mac="basic_mac", agent_output_type="q",
              action_selector="epsilon_greedy", epsilon_start=1.0, epsilon_finish=0.05, epsilon_anneal_time=50000,
              batch_size=B, learner="q_learner", device="cuda", use_cuda=True)
    scheme = {
        "state": {"vshape": S},
        "obs": {"vshape": O, "group": "agents"},
        "actions": {"vshape": (1,), "group": "agents", "dtype": th.long},
        "avail_actions": {"vshape": (A,), "group": "agents", "dtype": th.int},
        "reward": {"vshape": (1,)},
        "terminated": {"vshape": (1,), "dtype": th.uint8},
    }
    groups = {"agents": n}
    buf = PrioritizedReplayBuffer(scheme, groups, n_episodes, T + 1,
                                  preprocess={"actions": ("actions_onehot", [OneHot(A)])}, device="cuda", seed=seed,
                                  per_alpha=alpha, per_beta=beta)
    data = make_replay(unique, T, n, A, O, S, seed=seed)
    for start in range(0, n_episodes, unique):   # tile the unique episodes across the HBM-resident buffer
        m = min(unique, n_episodes - start)
        for k, v in data.items():
            buf.data.transition_data[k][start:start + m] = th.as_tensor(v[:m], device="cuda")
    buf.episode_lengths[:] = buf.data.transition_data["filled"].sum(1).reshape(-1).cpu().numpy()
    buf.refresh_avail_bits()
    buf.episodes_in_buffer = n_episodes
    th.manual_seed(seed)
    mac = mac_REGISTRY["basic_mac"](buf.scheme, groups, args)
    learner = le_REGISTRY["q_learner"](mac, buf.scheme, Logger(logging.getLogger("per_step_time")), args)
    learner.cuda()
    return buf, learner


def uniform_steps(buf, learner, steps, k0):
    from pymarl_amd.components.episode_buffer import ReplayBuffer
    for k in range(steps):
        b = ReplayBuffer.sample(buf, B)   # the uniform host draw, on the same storage
        learner.train(b[:, :b.max_t_filled()], 1000 * (k0 + k), 0)


def per_steps(buf, learner, steps, k0):
    for k in range(steps):
        b = buf.sample(B)
        learner.train(b[:, :b.max_t_filled()], 1000 * (k0 + k), 0)


def timed(fn, buf, learner, steps, k0):
    import torch as th
    th.cuda.synchronize()
    t0 = time.perf_counter()
    fn(buf, learner, steps, k0)
    th.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def kernel_stats(outdir):
    """{kernel name: (calls, mean ns)} from rocprofv3's kernel stats csv."""
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no kernel_stats.csv under {}".format(outdir))
    out = {}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            out[row["Name"]] = (int(row["Calls"]), float(row["AverageNs"]))
    return out


def profile(outdir, alpha, beta):
    os.makedirs(outdir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--",
           sys.executable, os.path.abspath(__file__), "--rounds", "1", "--steps", "20", "--alpha", str(alpha),
           "--beta", str(beta)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    st = kernel_stats(outdir)

    def pick(pattern, want=True):
        rows = [(k, v) for k, v in st.items() if "mix_fast_kernel" in k or pattern.startswith("per_")]
        rows = [(k, v) for k, v in rows if bool(re.search(pattern, k)) == want]
        return {k: dict(calls=c, mean_us=ns / 1e3) for k, (c, ns) in rows}
    per_tail = r"mix_fast_kernel(ILi16ELi16ELi4E|<16, 16, 4[,>])"   # mangled or demangled: the MIX_PER instantiation
    small = min(st.items(), key=lambda kv: kv[1][1])
    return dict(sampler=pick("per_sample_kernel"), priority=pick("per_priority_kernel"),
                per_tail=pick(per_tail), plain_tail=pick(per_tail, want=False),
                smallest=dict(name=small[0], calls=small[1][0], mean_us=small[1][1] / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--alpha", type=float, default=0.6, help="per_alpha (1: the sampler takes no powf)")
    ap.add_argument("--beta", type=float, default=0.4, help="per_beta")
    ap.add_argument("--profile", default=None, help="directory for one rocprofv3 --kernel-trace --stats pass")
    a = ap.parse_args()
    import torch as th
    if not th.cuda.is_available():
        raise SystemExit("per_step_time.py needs a HIP device")
    buf, learner = build(alpha=a.alpha, beta=a.beta)
    uniform_steps(buf, learner, 10, 0)   # warm both loops: handle, workspaces, code objects
    per_steps(buf, learner, 10, 10)
    assert learner.last_plan()["per"] == 1
    uni, per = [], []
    k0 = 20
    for _ in range(a.rounds):
        uni.append(timed(uniform_steps, buf, learner, a.steps, k0))
        per.append(timed(per_steps, buf, learner, a.steps, k0 + a.steps))
        k0 += 2 * a.steps
    res = dict(shape="cfg2", alpha=a.alpha, beta=a.beta, episodes=buf.episodes_in_buffer, rounds=a.rounds,
               steps=a.steps, uniform_us=uni, per_us=per, uniform_median_us=statistics.median(uni),
               per_median_us=statistics.median(per),
               per_minus_uniform_us=statistics.median(per) - statistics.median(uni), plan=learner.last_plan())
    if a.profile:
        del buf, learner
        th.cuda.synchronize()
        res["kernels"] = profile(a.profile, a.alpha, a.beta)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
