"""Cost of the opt-in TD(lambda) targets (q_targets: td_lambda) against the one-step target, same build, same run.

    python scripts/td_lambda_cost.py [--configs cfg2,cfg4] [--lam 0.8] [--warmup 5] [--steps 20] [--out FILE.json]

Per bench.py config and per target kind: the `mix` phase (HIP events around the mixer tail, QLearner.set_timing /
phase_times; the three launches of the lambda path sit inside that bracket), the sum of all phases, and the wall time
per step of the same number of steps without events in the stream. DESIGN.md "TD(lambda) targets" quotes the result
(profiles/td_lambda_cost.json).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def measure(cfg_name, lam, warmup, steps):
    import torch as th
    import bench
    B = bench.CONFIGS[cfg_name][6]
    out = {}
    for kind in ("one_step", "td_lambda"):
        # a workload of its own per target kind (same seeds: same replay, same initial weights)
        args, buf, learner, _ = bench.build_workload(cfg_name, th.device("cuda", 0))
        args.q_targets = kind   # read when the learner creates its handle, at the first train()
        args.td_lambda = lam
        np.random.seed(2)
        ep = [0]

        def step(k):
            gb = buf.sample(B)
            learner.train(gb[:, :gb.max_t_filled()], t_env=1000 * k, episode_num=ep[0])
            ep[0] += 8

        for k in range(warmup):
            step(k)
        th.cuda.synchronize()
        learner.set_timing(slots=steps)
        for k in range(steps):
            step(k)
        th.cuda.synchronize()
        ph = learner.phase_times()
        plan = learner.last_plan()
        learner.set_timing(slots=0)
        th.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(steps):
            step(k)
        th.cuda.synchronize()
        wall = (time.perf_counter() - t0) / steps * 1e3
        assert plan["td_lambda"] == int(kind == "td_lambda"), plan
        out[kind] = {"mix_ms": ph["mix"], "phases_sum_ms": float(sum(ph.values())), "wall_ms_per_step": wall,
                     "phase_ms": ph, "plan": plan, "loss": learner.last_stats()["loss"]}
        del args, buf, learner
        th.cuda.empty_cache()
    o, l = out["one_step"], out["td_lambda"]
    out["ratio"] = {"mix": l["mix_ms"] / o["mix_ms"], "phases_sum": l["phases_sum_ms"] / o["phases_sum_ms"],
                    "wall": l["wall_ms_per_step"] / o["wall_ms_per_step"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="cfg2,cfg4")
    ap.add_argument("--lam", type=float, default=0.8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "td_lambda_cost.json"))
    a = ap.parse_args()
    res = {"lambda": a.lam, "warmup": a.warmup, "steps": a.steps, "configs": {}}
    for c in a.configs.split(","):
        res["configs"][c] = measure(c, a.lam, a.warmup, a.steps)
        r = res["configs"][c]
        print(c, "mix ms one-step {:.4f} lambda {:.4f} (x{:.2f}); step ms {:.4f} -> {:.4f}".format(
            r["one_step"]["mix_ms"], r["td_lambda"]["mix_ms"], r["ratio"]["mix"],
            r["one_step"]["wall_ms_per_step"], r["td_lambda"]["wall_ms_per_step"]))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
