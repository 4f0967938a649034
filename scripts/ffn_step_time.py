#!/usr/bin/env python3
"""What the feed-forward agent (use_rnn: False, epymarl's key) costs per train step beside the GRU agent, and whether
the step without the key is what it was, on the cfg2 shape of bench.py (QMIX, 8 agents, T = 120, batch 32) with a
128-episode synthetic replay (pymarl_amd/utils/synthetic.py).

    python scripts/ffn_step_time.py [--rounds 6] [--steps 100] [--ab PARENT_TREE] [--profile DIR]

(b) Two learners, use_rnn absent (the GRU) and use_rnn: False, on ONE storage in interleaved rounds of --steps steps of
    ReplayBuffer.sample -> train, synchronising only at round ends: the per-step times of every round and feed-forward
    minus GRU in microseconds (medians).
(a) --ab PARENT_TREE: the use_rnn-absent step of this tree against the same step of another checkout with its own built
    library (PARENT_TREE/pymarl_amd/lib/libmq_learner.so), each round a fresh child process, alternating parent / new
    as scripts/ab_bench.sh does; the difference of the medians beside each side's own round-to-round spread.
--profile DIR: in fresh child processes, one `rocprofv3 --kernel-trace --stats` pass (no counters) over 20 steps of
    the feed-forward loop and one of the GRU loop: the mean duration of the agent's launches of either path.
Prints one JSON line. Needs a HIP device: there is no CPU path.
"""
import argparse
import csv
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
MIXER, N_AGENTS, N_ACTIONS, OBS, STATE, T, B = "qmix", 8, 14, 80, 168, 120, 32   # bench.py CONFIGS["cfg2"]
EPISODES = 128


def use_tree(root):
    """Import pymarl_amd from `root` (this tree, or --ab's other checkout in a child process)."""
    os.environ.pop("MQ_LEARNER_LIB", None)
    sys.path.insert(0, os.path.abspath(root))


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
    buf = ReplayBuffer(scheme, groups, EPISODES, T + 1, preprocess={"actions": ("actions_onehot", [OneHot(A)])},
                       device="cuda")
    buf.load_arrays(make_replay(EPISODES, T, n, A, O, S, seed=seed))
    return buf, groups


def make_learner(buf, groups, ffn, seed=0):
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
    if ffn:
        args.use_rnn = False
    th.manual_seed(seed)
    mac = mac_REGISTRY["basic_mac"](buf.scheme, groups, args)
    learner = le_REGISTRY["q_learner"](mac, buf.scheme, Logger(logging.getLogger("ffn_step_time")), args)
    learner.cuda()
    return learner


def steps_of(buf, learner, steps, k0):
    for k in range(steps):
        b = buf.sample(B)
        learner.train(b[:, :b.max_t_filled()], 1000 * (k0 + k), 0)


def timed(buf, learner, steps, k0):
    import torch as th
    th.cuda.synchronize()
    t0 = time.perf_counter()
    steps_of(buf, learner, steps, k0)
    th.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e6


def child_gru(root, steps):
    """--child: one round of the use_rnn-absent loop from the tree `root`; prints its per-step microseconds."""
    use_tree(root)
    buf, groups = make_buffer()
    learner = make_learner(buf, groups, False)
    steps_of(buf, learner, 10, 0)
    print(json.dumps(dict(us=timed(buf, learner, steps, 10), plan=learner.last_plan())))


def child_loop(which, steps):
    """--loop: 10 warm-up and `steps` steps of one loop, for the rocprofv3 pass."""
    use_tree(HERE_ROOT)
    buf, groups = make_buffer()
    learner = make_learner(buf, groups, which == "ffn")
    steps_of(buf, learner, 10 + steps, 0)
    import torch as th
    th.cuda.synchronize()


def run_child(argv, **kw):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, check=True, capture_output=True, text=True,
                         timeout=300, **kw)
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


def kernel_stats(outdir):
    files = glob.glob(os.path.join(outdir, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit("no kernel_stats.csv under {}".format(outdir))
    out = {}
    with open(files[0]) as f:
        for row in csv.DictReader(f):
            out[row["Name"]] = dict(calls=int(row["Calls"]), mean_us=float(row["AverageNs"]) / 1e3)
    return out


def profile(outdir, steps=20):
    res = {}
    for tag in ("ffn", "gru"):
        d = os.path.join(outdir, tag)
        os.makedirs(d, exist_ok=True)
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
                        sys.executable, os.path.abspath(__file__), "--loop", tag, "--steps", str(steps)],
                       check=True, stdout=subprocess.DEVNULL, timeout=600)
        st = kernel_stats(d)
        words = ("Fc1Prob", "FfnHidProb", "Fc2Prob", "ffn_dp2", "FfnDx1Prob", "FfnDwrProb", "Dw1Prob", "hyper_", "dwh_",
                 "gru_fwd_pair", "gru_bwd_fused", "mix_fast", "red_pass", "apply_kernel")
        res[tag] = {k: v for k, v in st.items() if any(w in k for w in words)}
        res[tag + "_step_kernel_sum_us"] = sum(v["calls"] * v["mean_us"] for v in st.values()) / (10 + steps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--ab", default=None, help="another checkout (built) to A/B the use_rnn-absent step against")
    ap.add_argument("--profile", default=None, help="directory for the rocprofv3 --kernel-trace --stats passes")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--loop", default=None, choices=("ffn", "gru"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child_gru(a.child, a.steps)
    if a.loop:
        return child_loop(a.loop, a.steps)
    res = dict(shape="cfg2", episodes=EPISODES, rounds=a.rounds, steps=a.steps)
    if a.ab:   # before this process opens the GPU: one child at a time
        res["gru_ab"] = ab(a.ab, a.rounds, a.steps)
    if a.profile:
        res["kernels"] = profile(a.profile)
    use_tree(HERE_ROOT)
    import torch as th
    if not th.cuda.is_available():
        raise SystemExit("ffn_step_time.py needs a HIP device")
    buf, groups = make_buffer()
    gru, ffn = make_learner(buf, groups, False), make_learner(buf, groups, True)
    steps_of(buf, gru, 10, 0)
    steps_of(buf, ffn, 10, 0)
    assert ffn.last_agent() == 1 and gru.last_agent() == 0
    tg, tf = [], []
    k0 = 10
    for _ in range(a.rounds):
        tg.append(timed(buf, gru, a.steps, k0))
        tf.append(timed(buf, ffn, a.steps, k0))
        k0 += a.steps
    res.update(gru_us=tg, ffn_us=tf, gru_median_us=statistics.median(tg), ffn_median_us=statistics.median(tf),
               ffn_minus_gru_us=statistics.median(tf) - statistics.median(tg),
               ffn_below_gru_in_every_round=all(f < g for f, g in zip(tf, tg)), ffn_agent=ffn.last_agent(),
               plan_gru=gru.last_plan(), plan_ffn=ffn.last_plan())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
