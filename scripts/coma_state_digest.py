#!/usr/bin/env python3
"""SHA-256 digests of everything three train() calls leave behind, for comparing two builds of libmq_learner.so whose
device code is the same and whose host sequence may not be (a host-side refactor of the COMA, actor-critic or PPO step).

    MQ_LEARNER_LIB=<path to a build> python scripts/coma_state_digest.py > digest_<build>.json
    python scripts/coma_state_digest.py --compare A.json B.json [C.json ..]     (no GPU: which digests differ)

Cases, each at fixed seeds: the golden COMA cases coma_tiny_masked and coma_cfg5 (MMM2's shape), each on the persistent
chain and under MQ_PLAN=coma_chain=0 (the three-launch critic step); the actor-critic learner on tests/a2c_ref.py's
`split` row (544 rows: every split-K weight gradient has two slices); the PPO learner on tests/ppo_ref.py's `split` row
at two epochs. After every train() it hashes every buffer the learner bound (parameters, square averages / Adam
moments, both gradient buffers with their tails, the target critic, the stats) and every *_copy_intermediate array.
Prints one JSON object {case: [{name: digest} per train()]}; two runs of one build show which digests repeat at all, a
run of another build is then compared digest by digest. Run it in a fresh process per build. Needs a HIP device.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = 3


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def digests(learner, names, intermediates):
    out = {k: sha(getattr(learner, k)) for k in names if getattr(learner, k, None) is not None}
    for i in intermediates:
        out["intermediate_{}".format(i)] = sha(learner.last_intermediate(i))
    return out


def coma_case(name, chain):
    import numpy as np
    from tests.golden_utils import ComaCase
    from tests.gpu_helpers import build_coma
    os.environ.pop("MQ_PLAN", None)
    if not chain:
        os.environ["MQ_PLAN"] = "coma_chain=0"   # read when the learner's handle is created, at its first train()
    cc = ComaCase(name)
    _, buf, mac, learner, _ = build_coma(cc)
    np.random.seed(cc.sampler_seed)
    out = []
    for k in range(STEPS):
        b = buf.sample(cc.B)
        b = b[:, :b.max_t_filled()]
        mac.action_selector.epsilon = cc.epsilon[k % len(cc.epsilon)]
        learner.train(b, 1000 * (k + 1), k)
        d = digests(learner, ("_agent", "_agrad", "_asq", "_critic", "_tcritic", "_cgrad", "_csq", "_stats"), (0, 1, 2))
        d["critic_path"] = int(learner._handle.lib.mc_last_critic_path(learner._handle.h))
        out.append(d)
    os.environ.pop("MQ_PLAN", None)
    return out


A2C_BUFFERS = ("_agent", "_agrad", "_asq", "_am", "_critic", "_tcritic", "_cgrad", "_csq", "_cm", "_stats", "rew_ms")


def a2c_case():
    from tests import a2c_ref
    from tests.a2c_helpers import build_a2c
    c = a2c_ref.A2CCase("split")
    _, buf, _, learner, _ = build_a2c(c)
    out = []
    for k in range(STEPS):
        b = buf.sample(c.B)
        learner.train(b[:, :b.max_t_filled()], 1000 * (k + 1), k)
        d = digests(learner, A2C_BUFFERS, (0, 1, 2, 3, 4))
        d["plan"] = learner.last_plan()
        out.append(d)
    return out


def ppo_case():
    from tests import ppo_ref
    from tests.ppo_helpers import build_ppo
    c = ppo_ref.PPOCase("split")
    _, buf, _, learner, _ = build_ppo(c, epochs=2)
    out = []
    for k in range(STEPS):
        b = buf.sample(c.B)
        learner.train(b[:, :b.max_t_filled()], 1000 * (k + 1), k)
        d = digests(learner, A2C_BUFFERS + ("_estats",), (0, 1, 2, 3, 4, 5, 6))
        d["plan"] = learner.last_plan()
        out.append(d)
    return out


def compare(paths):
    """--compare A.json B.json [C.json ..]: every (case, train(), name) whose value is not the same in all files."""
    runs = [json.load(open(p)) for p in paths]
    diff, total = [], 0
    for case in runs[0]:
        if case == "lib":
            continue
        for k, step in enumerate(runs[0][case]):
            for name, v in step.items():
                total += 1
                if any(r[case][k].get(name) != v for r in runs[1:]):
                    diff.append("{}[{}].{}".format(case, k, name))
    print(json.dumps(dict(files=[os.path.basename(p) for p in paths], compared=total, differ=diff)))
    return 1 if diff else 0


def main():
    if len(sys.argv) > 3 and sys.argv[1] == "--compare":
        raise SystemExit(compare(sys.argv[2:]))
    import numpy as np
    import torch as th
    if not th.cuda.is_available():
        raise SystemExit("coma_state_digest.py needs a HIP device")
    res = {"lib": os.path.basename(os.environ.get("MQ_LEARNER_LIB", "libmq_learner.so"))}
    for name in ("coma_tiny_masked", "coma_cfg5"):
        for chain in (True, False):
            res["{}/{}".format(name, "chain" if chain else "three_launch")] = coma_case(name, chain)
    np.random.seed(0)
    res["a2c/split"] = a2c_case()
    np.random.seed(0)
    res["ppo/split_epochs2"] = ppo_case()
    th.cuda.synchronize()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
