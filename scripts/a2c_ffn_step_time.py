#!/usr/bin/env python3
"""What the feed-forward actor (`use_rnn: False`, what epymarl's maa2c.yaml / mappo.yaml ship) saves
beside the GRU actor, at the cfg5 shape of bench.py (scripts/a2c_step_time.py's storage) with maa2c.yaml's / mappo.yaml's
keys (scripts/ppo_step_time.py's), for one ActorCriticLearner.train() and one four-epoch PPOLearner.train().

    python scripts/a2c_ffn_step_time.py [--epochs 4] [--rounds 6] [--steps 100] [--profile DIR]

Four learners (each learner with use_rnn: True and use_rnn: False) on ONE storage in interleaved rounds of --steps
steps of ReplayBuffer.sample -> train, after one untimed round of the same: the per-step times of every round, their medians and round-to-round spreads, in
microseconds; `faster` is true when the feed-forward median is below the GRU one by more than the larger of the two
spreads. --profile DIR: in a fresh child process each, one `rocprofv3 --kernel-trace --stats` pass (no counters) over
20 train() calls of the feed-forward actor-critic and PPO loops: launches per train(), every kernel's calls and mean
duration, and for the two ffn_actor kernels the bytes they move through HBM and the bytes/s that makes.
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
import a2c_step_time as base  # noqa: E402  (the shape, the storage, the profile readers)
import ppo_step_time as ppo  # noqa: E402  (the timed loop)

B, WARMUP = base.B, base.WARMUP
KINDS = ("actor_critic_learner", "ppo_learner")


def make_learner(buf, groups, which, epochs, use_rnn, seed=0):
    """ppo_step_time.make_learner's keys (mappo.yaml's / maa2c.yaml's) with use_rnn beside them."""
    import logging
    from types import SimpleNamespace as SN

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
              target_update_interval_or_tau=0.01, learner=which, use_rnn=use_rnn)
    if which == "ppo_learner":
        args.__dict__.update(epochs=epochs, eps_clip=0.2)
    th.manual_seed(seed)
    mac = mac_REGISTRY["basic_mac"](buf.scheme, groups, args)
    learner = le_REGISTRY[which](mac, buf.scheme, Logger(logging.getLogger("a2c_ffn_step_time")), args)
    learner.cuda()
    return learner


def hbm_bytes(plan, I, A):
    """Bytes each ffn_actor kernel moves through HBM per launch (weights once per workgroup, activations once)."""
    rt, ap = plan["rows"], plan["ap"]
    nf, nb = min(plan["ffn_tiles"], 512), plan["ffn_blocks"]
    w = 64 * I + 64 * 64 + A * 64
    fwd = 4 * (rt * (base.OBS + 2 * 64 + A + I) + nf * w)
    bwd = 4 * (rt * (ap + 3 * 64) + nb * (64 * 64 + A * 64) + nb * (64 * 65 + A * 65))
    return dict(ffn_actor_fwd_kernel=fwd, ffn_actor_bwd_kernel=bwd)


def child_loop(steps, epochs, which):
    sys.path.insert(0, base.HERE_ROOT)
    import torch as th
    buf, groups = base.make_buffer()
    learner = make_learner(buf, groups, which, epochs, False)
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
    res = dict(shape="cfg5", n_agents=base.N_AGENTS, n_actions=base.N_ACTIONS, T=base.T, batch=B, epochs=a.epochs,
               rounds=a.rounds, steps=a.steps)
    if a.profile:   # before this process opens the GPU: one child at a time
        res["profile"] = {w: profile(os.path.join(a.profile, w), a.epochs, w) for w in KINDS}
    sys.path.insert(0, base.HERE_ROOT)
    import torch as th
    if not th.cuda.is_available():
        raise SystemExit("a2c_ffn_step_time.py needs a HIP device")
    buf, groups = base.make_buffer()
    ls = {(w, r): make_learner(buf, groups, w, a.epochs, r) for w in KINDS for r in (True, False)}
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
        g, f = times[(w, True)], times[(w, False)]
        mg, mf, sg, sf = statistics.median(g), statistics.median(f), max(g) - min(g), max(f) - min(f)
        res[w] = dict(gru_us=g, ffn_us=f, gru_median_us=mg, ffn_median_us=mf, gru_spread_us=sg, ffn_spread_us=sf,
                      saved_us=mg - mf, faster=(mg - mf) > max(sg, sf), plan=ls[(w, False)].last_plan())
    plan = res[KINDS[0]]["plan"]
    I = base.OBS + base.N_ACTIONS + base.N_AGENTS
    res["hbm_bytes"] = hbm_bytes(plan, I, base.N_ACTIONS)
    if a.profile:
        for k in res["profile"][KINDS[0]]["kernels"]:
            if k["name"] in res["hbm_bytes"]:
                k["gbytes_per_s"] = round(res["hbm_bytes"][k["name"]] / k["mean_us"] / 1e3, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
