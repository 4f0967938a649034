#!/usr/bin/env python3
"""What a train step with the QPLEX mixer (mixer: dmaq, num_kernel 4, hypernet_embed 64) costs beside the QMIX step, on
the cfg2 shape of bench.py (8 agents, T = 120, batch 32) with scripts/hyper2_step_time.py's storage, loop and method.

    python scripts/dmaq_step_time.py [--rounds 6] [--steps 100] [--profile DIR]

Two learners, QMIX and dmaq, on ONE storage: one untimed round, then interleaved rounds of --steps steps of
ReplayBuffer.sample -> train, synchronising only at round ends; the per-step times of every round and dmaq minus QMIX in
microseconds (medians). QMIX's step is the scale, not a bound.
--profile DIR: in a fresh child process, one `rocprofv3 --kernel-trace --stats` pass (no counters) over 20 steps of the
    dmaq loop: calls and mean duration of every kernel, and the library's kernels' sum per step.
Prints one JSON line. Needs a HIP device: there is no CPU path.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hyper2_step_time as H  # noqa: E402


def make_learner(buf, groups, mixer):
    """hyper2_step_time's learner (its arguments, one hypernet layer) with `mixer`; dmaq's keys at their defaults."""
    return H.make_learner(buf, groups, 1, mixer=mixer)


def child_loop(steps):
    """--loop: 10 warm-up and `steps` steps of the dmaq loop, for the rocprofv3 pass."""
    H.use_tree(H.HERE_ROOT)
    import torch as th
    buf, groups = H.make_buffer()
    H.steps_of(buf, make_learner(buf, groups, "dmaq"), 10 + steps, 0)
    th.cuda.synchronize()


def profile(outdir, steps=20):
    os.makedirs(outdir, exist_ok=True)
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", outdir, "--",
                    sys.executable, os.path.abspath(__file__), "--loop", "--steps", str(steps)],
                   check=True, stdout=subprocess.DEVNULL, timeout=600)
    st = H.kernel_stats(outdir)
    ours = {k: v for k, v in st.items() if "mq::" in k}   # the library's kernels: torch's set-up kernels are not a step's
    return dict(kernels=st, step_kernel_sum_us=sum(v["calls"] * v["mean_us"] for v in ours.values()) / (10 + steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--profile", default=None, help="directory for the rocprofv3 --kernel-trace --stats pass")
    ap.add_argument("--loop", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.loop:
        return child_loop(a.steps)
    res = dict(shape="cfg2", episodes=H.EPISODES, rounds=a.rounds, steps=a.steps)
    if a.profile:   # before this process opens the GPU: one process at a time
        res["profile"] = profile(a.profile)
    H.use_tree(H.HERE_ROOT)
    import torch as th
    if not th.cuda.is_available():
        raise SystemExit("dmaq_step_time.py needs a HIP device")
    buf, groups = H.make_buffer()
    qmix, dmaq = make_learner(buf, groups, "qmix"), make_learner(buf, groups, "dmaq")
    for le in (qmix, dmaq):   # the untimed round
        H.steps_of(buf, le, a.steps, 0)
    assert dmaq.last_mixer() == 3 and qmix.last_mixer() == 2
    tq, td, k0 = [], [], a.steps
    for _ in range(a.rounds):
        tq.append(H.timed(buf, qmix, a.steps, k0))
        td.append(H.timed(buf, dmaq, a.steps, k0))
        k0 += a.steps
    res.update(qmix_us=tq, dmaq_us=td, qmix_median_us=statistics.median(tq), dmaq_median_us=statistics.median(td),
               dmaq_minus_qmix_us=statistics.median(td) - statistics.median(tq), plan_qmix=qmix.last_plan(),
               plan_dmaq=dmaq.last_plan())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
