#!/usr/bin/env python3
"""SHA-256 digests of everything three train() calls leave behind, for comparing two builds of libmq_learner.so whose
device code is the same and whose host sequence may not be (a host-side refactor of the COMA, actor-critic or PPO step),
or two checkouts' Python over one build (a refactor of the learners' Python).

    MQ_LEARNER_LIB=<path to a build> python scripts/coma_state_digest.py [--tree CHECKOUT] > digest_<build>.json
    python scripts/coma_state_digest.py --compare A.json B.json [C.json ..]     (no GPU: which digests differ)

--tree CHECKOUT imports `pymarl_amd` and `tests` from that checkout instead of this script's own.

Cases, each at fixed seeds: the golden COMA cases coma_tiny_masked and coma_cfg5 (MMM2's shape), each on the persistent
chain and under MQ_PLAN=coma_chain=0 (the three-launch critic step); the actor-critic learner on tests/a2c_ref.py's
`split` row (544 rows: every split-K weight gradient has two slices); the PPO learner on tests/ppo_ref.py's `split` row
at two epochs. After every train() it hashes every buffer the learner bound (parameters, square averages / Adam
moments, both gradient buffers with their tails, the target critic, the stats) and every *_copy_intermediate array.
The Q learner on the goldens' tiny shapes: tiny_qmix / tiny_vdn / tiny_iql, tiny_qmix_adam (optimizer: adam),
tiny_qmix_h2 (the two-layer hypernet), tiny_qmix with the soft target update and standardised rewards, with TD(lambda)
targets, and as tests/test_gpu_per.py's prioritized-replay loop; the bound buffers, rew_ms and the intermediates that
step wrote. Checkpoints (`ckpt/...`): one Q, COMA, actor-critic and PPO case each save_models after its three steps
into a temporary directory; every tensor of every file as th.load returns it (path of keys, dtype, bytes), then the
flat buffers and step counts of a fresh learner after load_models.
Prints one JSON object {case: [{name: digest} per train()]}; two runs of one build show which digests repeat at all, a
run of another build is then compared digest by digest. Run it in a fresh process per build. Needs a HIP device.
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = "--tree" in sys.argv   # whether `pymarl_amd` and `tests` come from another checkout
if TREE:
    ROOT = os.path.abspath(sys.argv.pop(sys.argv.index("--tree") + 1))
    sys.argv.remove("--tree")
sys.path.insert(0, ROOT)
STEPS = 3
CKPT = {}   # case -> [digests of the saved files, digests of a fresh learner after load_models]


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def digests(learner, names, intermediates):
    out = {k: sha(getattr(learner, k)) for k in names if getattr(learner, k, None) is not None}
    for i in intermediates:
        out["intermediate_{}".format(i)] = sha(learner.last_intermediate(i))
    return out


def tree_digests(obj, path, out):
    """Every tensor under `obj` (dicts and lists as th.load returned them, in their own order): path -> dtype:sha."""
    import torch as th
    if isinstance(obj, th.Tensor):
        out[path] = "{}:{}".format(obj.dtype, sha(obj))
    elif isinstance(obj, dict):
        for k, v in obj.items():
            tree_digests(v, "{}/{!r}".format(path, k), out)
    elif isinstance(obj, (list, tuple)):
        for i, v in enumerate(obj):
            tree_digests(v, "{}[{}]".format(path, i), out)
    else:
        out[path] = repr(obj)


def checkpoint(name, learner, fresh, buffers):
    """save_models into a temporary directory, load_models into `fresh` (a learner built the same way)."""
    import tempfile
    import torch as th
    with tempfile.TemporaryDirectory() as d:
        learner.save_models(d)
        saved = {}
        for f in sorted(os.listdir(d)):
            tree_digests(th.load(os.path.join(d, f), map_location="cpu", weights_only=True), f, saved)
        fresh.load_models(d)
    loaded = digests(fresh, buffers, ())
    loaded["_opt_steps"] = getattr(fresh, "_opt_steps", None)
    for o in ("optimiser", "agent_optimiser", "critic_optimiser"):
        opt = getattr(fresh, o, None)
        if opt is not None:
            loaded[o + ".steps"] = [float(opt.state[p]["step"]) for g in opt.param_groups for p in g["params"]]
    CKPT["ckpt/" + name] = [saved, loaded]


Q_BUFFERS = ("_online", "_target", "_grad", "_sq", "_m", "_stats", "_curmax", "rew_ms")
# name -> (golden case, learner arguments, intermediates beyond 0 .. 3 that such a step writes)
Q_CASES = {
    "tiny_qmix": ("tiny_qmix", {}, ()),
    "tiny_vdn": ("tiny_vdn", {}, ()),
    "tiny_iql": ("tiny_iql", {}, ()),
    "tiny_qmix_adam": ("tiny_qmix_adam", dict(optimizer="adam"), ()),
    "tiny_qmix_h2": ("tiny_qmix_h2", None, (7,)),
    "tiny_qmix_soft_rewnorm": ("tiny_qmix", dict(target_update_interval_or_tau=0.01, standardise_rewards=True), (8,)),
    "tiny_qmix_td_lambda": ("tiny_qmix", dict(q_targets="td_lambda", td_lambda=0.8), (4, 5)),
}


def q_case(name, ckpt=False):
    import numpy as np
    from tests.golden_utils import Case
    from tests.gpu_helpers import build
    golden, over, extra = Q_CASES[name]
    if over is None:
        from tests.hyper2_ref import GoldenCase2
        case = GoldenCase2()
        over = case.over()
    else:
        case = Case(golden)
    _, buf, _, learner, _ = build(case, **over)
    np.random.seed(case.sampler_seed)
    out = []
    for k in range(STEPS):
        b = buf.sample(case.B)
        learner.train(b[:, :b.max_t_filled()], 1000 * k, 200 * k)
        d = digests(learner, Q_BUFFERS, (0, 1, 2, 3) + extra)
        d["plan"] = learner.last_plan()
        out.append(d)
    if ckpt:
        checkpoint(name, learner, build(case, **over)[3], Q_BUFFERS)
    return out


def per_case():
    from tests.golden_utils import Case
    from tests.test_gpu_per import build_per
    case = Case("tiny_qmix")
    _, _, pbuf, learner = build_per(case, seed=11)
    out = []
    for k in range(STEPS):
        pb = pbuf.sample(case.B)
        learner.train(pb, 1000 * k, 200 * k)
        d = digests(learner, Q_BUFFERS, (0, 1, 2, 3, 6))
        d.update(ep_ids=sha(pb.ep_ids), weights=sha(pb.weights), prio=sha(pbuf.prio), prio_max=sha(pbuf.prio_max),
                 plan=learner.last_plan())
        out.append(d)
    return out


COMA_BUFFERS = ("_agent", "_agrad", "_asq", "_critic", "_tcritic", "_cgrad", "_csq", "_stats")


def coma_case(name, chain, ckpt=False):
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
        d = digests(learner, COMA_BUFFERS, (0, 1, 2))
        d["critic_path"] = int(learner._handle.lib.mc_last_critic_path(learner._handle.h))
        out.append(d)
    os.environ.pop("MQ_PLAN", None)
    if ckpt:
        checkpoint("coma/" + name, learner, build_coma(cc)[3], COMA_BUFFERS)
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
    checkpoint("a2c/split", learner, build_a2c(c)[3], A2C_BUFFERS)
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
    checkpoint("ppo/split_epochs2", learner, build_ppo(c, epochs=2)[3], A2C_BUFFERS)
    return out


def compare(paths):
    """--compare A.json B.json [C.json ..]: every (case, train(), name) whose value is not the same in all files."""
    runs = [json.load(open(p)) for p in paths]
    diff, total = [], 0
    for case in runs[0]:
        if case in ("lib", "tree"):
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
    import pymarl_amd
    assert os.path.abspath(pymarl_amd.__file__).startswith(ROOT + os.sep), pymarl_amd.__file__
    res = {"lib": os.path.basename(os.environ.get("MQ_LEARNER_LIB", "libmq_learner.so")),
           "tree": "--tree" if TREE else "own"}
    for name in ("coma_tiny_masked", "coma_cfg5"):
        for chain in (True, False):
            res["{}/{}".format(name, "chain" if chain else "three_launch")] = coma_case(
                name, chain, ckpt=chain and name == "coma_tiny_masked")
    np.random.seed(0)
    res["a2c/split"] = a2c_case()
    np.random.seed(0)
    res["ppo/split_epochs2"] = ppo_case()
    for name in Q_CASES:
        res["q/" + name] = q_case(name, ckpt=name == "tiny_qmix_soft_rewnorm")
    res["q/tiny_qmix_per"] = per_case()
    res.update(CKPT)
    th.cuda.synchronize()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
