"""The Adam opt-in (optimizer: adam; mq_set_adam, mq_adam_update, apply_adam_kernel) on the GPU.

The gate is the project's rule: for each of p, exp_avg, exp_avg_sq the GPU's max error against torch.optim.Adam in
float64 on the CPU is at most 16 * max(error of torch's float32 CPU run against float64, 2e-7 * max|ref|), both runs
from the same float32 inputs.

1. the standalone kernel (mq_adam_update) over sizes, step numbers and weight decays, unaligned pointers;
2. learner steps: the new parameters and moments are torch's Adam applied to exactly the parameters / moments before
   the step and the clipped gradient after it with step k + 1; the prologue (grad_norm, clip coefficient, clipped
   gradient) is RMSprop's bitwise; the gradient buffer holds no weight-decay term;
3. the Adam learner does not step as the RMSprop learner does;
4. the reference's own CPU QLearner trained with torch.optim.Adam (tests/golden/tiny_qmix_adam.npz,
   make_golden_adam.py): stats and parameters of every step, with the elements whose gradient is rounding noise
   (the generator's mask) bounded by Adam's worst-case step;
5. composition: two runs bitwise; the data-parallel norm path; TD(lambda) + two-layer hypernet + PER + Adam in one
   step; a checkpoint round trip and a handle rebuild keep the step count and both moments; data parallelism.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch as th

from pymarl_amd import _lib
from tests import test_gpu_parity as P
from tests.golden_utils import GOLDEN, Case
from tests.gpu_helpers import build, flat_grads, flat_params, flat_targets, rel

pytestmark = pytest.mark.gpu

LR, BETAS, EPS = 5e-4, (0.9, 0.999), 1e-8   # gpu_helpers.make_args' lr; optimizer: adam's defaults (torch's)
ROOM, FLOOR = 16.0, 2e-7


# ---------------------------------------------------------------------------------------------- the reference
def torch_adam(p, g, m, v, step, dtype, lr=LR, betas=BETAS, eps=EPS, wd=0.0):
    """torch.optim.Adam's step number `step` (1-based) on the CPU in `dtype` from float32 inputs: (p, m, v) float64."""
    t = lambda a: th.tensor(np.asarray(a, np.float32), dtype=dtype)  # noqa: E731
    w = th.nn.Parameter(t(p))
    opt = th.optim.Adam([w], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    opt.state[w]["step"] = th.tensor(float(step - 1))
    opt.state[w]["exp_avg"] = t(m)
    opt.state[w]["exp_avg_sq"] = t(v)
    w.grad = t(g)
    opt.step()
    assert float(opt.state[w]["step"]) == step
    f = lambda x: x.detach().double().numpy()  # noqa: E731
    return f(w), f(opt.state[w]["exp_avg"]), f(opt.state[w]["exp_avg_sq"])


def gate(what, got, p, g, m, v, step, **kw):
    """The three outputs `got` = (p, m, v) against the float64 run under the module's rule; returns the ratios."""
    r64 = torch_adam(p, g, m, v, step, th.float64, **kw)
    r32 = torch_adam(p, g, m, v, step, th.float32, **kw)
    ratios, bad = {}, []
    for name, a, b64, b32 in zip(("p", "exp_avg", "exp_avg_sq"), got, r64, r32):
        scale = float(np.abs(b64).max())
        e32 = float(np.abs(b32 - b64).max())
        err = float(np.abs(np.asarray(a, np.float64) - b64).max())
        den = max(e32, FLOOR * scale)
        ratios[name] = err / den if den > 0 else (0.0 if err == 0 else float("inf"))
        if not err <= ROOM * den:
            bad.append((name, err, e32, scale))
    print("{}: err / max(e32, 2e-7 max|ref|) = {}".format(what, {k: round(x, 3) for k, x in ratios.items()}))
    assert not bad, (what, bad)
    return ratios


# ---------------------------------------------------------------------------------------------- 1. standalone
SENTINEL = 12345.0
PAD = 8


def gpu_adam(p, g, m, v, step, offs=(1, 1, 1, 1), lr=LR, betas=BETAS, eps=EPS, wd=0.0):
    """mq_adam_update on device copies whose pointers sit `offs` floats past a 16-byte boundary; the floats around
    every buffer must come back untouched."""
    lib = _lib.load()
    n = len(p)
    bufs = []
    for a, o in zip((p, g, m, v), offs):
        t = th.full((n + 2 * PAD,), SENTINEL, dtype=th.float32, device="cuda")
        assert t.data_ptr() % 16 == 0
        t[4 + o:4 + o + n] = th.from_numpy(np.asarray(a, np.float32))
        bufs.append((t, 4 + o))
    ptr = [ctypes.c_void_p(t.data_ptr() + 4 * o) for t, o in bufs]
    _lib.check(lib.mq_adam_update(ptr[0], ptr[1], ptr[2], ptr[3], n, lr, betas[0], betas[1], eps, wd, step,
                                  _lib.stream_ptr()))
    th.cuda.synchronize()
    out = []
    for t, o in bufs:
        h = t.cpu().numpy()
        assert (h[:o] == SENTINEL).all() and (h[o + n:] == SENTINEL).all(), "a write outside the buffer"
        out.append(h[o:o + n].copy())
    return out   # p, g, m, v


def adam_inputs(n, step, seed):
    """Gradients spanning 1e-12 .. 1e2 in magnitude with exact zeros (every index = 3 mod 5); moments of a run in
    progress (step > 1) or fresh zeros (step = 1), zero at the zero-gradient indices = 3 mod 10."""
    rng = np.random.default_rng(seed)
    mag = lambda: 10.0 ** rng.uniform(-12, 2, n) * rng.choice([-1.0, 1.0], n)  # noqa: E731
    p = rng.standard_normal(n)
    g = mag()
    idx = np.arange(n)
    g[idx % 5 == 3] = 0.0
    if step > 1:
        m, v = 0.3 * mag(), (0.05 * mag()) ** 2
        m[idx % 10 == 3] = 0.0
        v[idx % 10 == 3] = 0.0
    else:
        m, v = np.zeros(n), np.zeros(n)
    f = lambda a: a.astype(np.float32)  # noqa: E731
    return f(p), f(g), f(m), f(v)


SIZES = [1, 3, 255, 256, 257, 1027, 262144 + 259]   # the last: a second grid-stride sweep, a length != 0 mod 4


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("n", SIZES)
def test_standalone_kernel_vs_torch_adam(n, step, wd):
    p, g, m, v = adam_inputs(n, step, seed=7 * n + step)
    p1, g1, m1, v1 = gpu_adam(p, g, m, v, step, wd=wd)
    assert np.array_equal(g1.view(np.uint32), g.view(np.uint32))   # no clip, no normalisation: g is written back as is
    gate("n={} step={} wd={}".format(n, step, wd), (p1, m1, v1), p, g, m, v, step, wd=wd)
    still = (g == 0) & (m == 0) & (v == 0)
    if n >= 4:
        assert still.any()
    if wd == 0.0:   # nothing to apply: the parameter keeps its bits and the moments stay zero
        assert np.array_equal(p1[still].view(np.uint32), p[still].view(np.uint32))
        assert not m1[still].any() and not v1[still].any()


@pytest.mark.parametrize("n", [1027, 262144 + 259])
def test_standalone_kernel_result_does_not_depend_on_alignment_or_run(n):
    """The float4 body with a head (all pointers one float past a boundary), without one (aligned) and the scalar path
    (pointers that disagree modulo 16 bytes) give the same bits, and so do two runs."""
    p, g, m, v = adam_inputs(n, 2, seed=n)
    outs = [gpu_adam(p, g, m, v, 2, offs=o, wd=1e-2) for o in ((1, 1, 1, 1), (1, 1, 1, 1), (0, 0, 0, 0), (3, 3, 3, 3),
                                                                (0, 1, 2, 3))]
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------- 2. learner steps
@pytest.fixture(scope="module")
def cases():
    return {}


def get_case(cases, name):
    if name not in cases:
        cases[name] = Case(name)
    return cases[name]


def moments(learner):
    return learner._m.detach().cpu().numpy().copy(), learner._sq.detach().cpu().numpy().copy()


def train_checked(learner, batch, t_env, episode, k, what, wd=0.0):
    """One train() whose update must be torch's Adam step k + 1 on the state before it and the gradient after it."""
    p0 = flat_params(learner)
    m0, v0 = moments(learner)
    learner.train(batch, t_env, episode)
    th.cuda.synchronize()
    g = flat_grads(learner)
    assert np.isfinite(g).all() and np.abs(g).max() > 0
    m1, v1 = moments(learner)
    assert int(learner._handle.lib.mq_opt_step(learner._handle.h)) == k + 1 == learner._opt_steps
    return gate(what, (flat_params(learner), m1, v1), p0, g, m0, v0, k + 1, wd=wd)


def sampled(buf, case, k):
    batch = buf.sample(case.B)
    return batch[:, :batch.max_t_filled()]


@pytest.mark.parametrize("name", ["tiny_qmix", "tiny_vdn", "tiny_iql"])
def test_learner_steps_are_torch_adam_steps(cases, name):
    case = get_case(cases, name)
    args, buf, mac, learner, logger = build(case, optimizer="adam")
    assert type(learner.optimiser) is th.optim.Adam
    np.random.seed(case.sampler_seed)
    for k in range(4):
        train_checked(learner, sampled(buf, case, k), 1000 * k, case.episodes[k], k, "{} step {}".format(name, k))
        assert float(learner.optimiser.state[learner.params[0]]["step"]) == k + 1
    # the optimiser object sees the moments the kernel wrote
    st = learner.optimiser.state[learner.params[0]]
    n0 = learner.params[0].numel()
    assert th.equal(st["exp_avg"].reshape(-1), learner._m[:n0]) and float(st["exp_avg"].abs().max()) > 0
    assert th.equal(st["exp_avg_sq"].reshape(-1), learner._sq[:n0])


def first_step(case, **over):
    args, buf, mac, learner, logger = build(case, **over)
    np.random.seed(case.sampler_seed)
    learner.train(sampled(buf, case, 0), 0, case.episodes[0])
    th.cuda.synchronize()
    return learner


@pytest.mark.parametrize("name", ["tiny_qmix", "tiny_vdn", "tiny_iql"])
def test_prologue_is_rmsprops_bitwise_and_adam_steps_differently(cases, name):
    case = get_case(cases, name)
    adam, rms = first_step(case, optimizer="adam"), first_step(case)
    sa, sr = adam._stats.cpu().numpy(), rms._stats.cpu().numpy()
    assert np.array_equal(sa.view(np.uint32), sr.view(np.uint32)), (sa, sr)   # grad_norm, clip coefficient, the rest
    assert sa[1] > 0 and 0 < sa[6] <= 1
    assert np.array_equal(flat_grads(adam), flat_grads(rms))   # the clipped gradient clip_grad_norm_ leaves in .grad
    # 3. without the feature the key is ignored and both learners take RMSprop's step
    assert not np.array_equal(flat_params(adam), flat_params(rms))
    assert rms._m is None and float(adam._m.abs().max()) > 0
    assert type(rms.optimiser) is th.optim.RMSprop


def test_weight_decay_stays_out_of_the_gradient_buffer(cases):
    case = get_case(cases, "tiny_qmix")
    args, buf, mac, wd, logger = build(case, optimizer="adam", weight_decay=1e-2)
    np.random.seed(case.sampler_seed)
    train_checked(wd, sampled(buf, case, 0), 0, case.episodes[0], 0, "weight_decay step 0", wd=1e-2)
    plain = first_step(case, optimizer="adam")
    assert np.array_equal(flat_grads(wd), flat_grads(plain))   # .grad after clip_grad_norm_: no decay term
    assert np.array_equal(wd._stats.cpu().numpy(), plain._stats.cpu().numpy())   # and none in grad_norm
    assert not np.array_equal(flat_params(wd), flat_params(plain))
    train_checked(wd, sampled(buf, case, 1), 1000, case.episodes[1], 1, "weight_decay step 1", wd=1e-2)


# ---------------------------------------------------------------------------------------------- 4. the golden
def test_golden_run_of_the_reference_learner_with_adam():
    """tests/golden/tiny_qmix_adam.npz: the five stats of every step to the tolerance tests/test_gpu_parity.py holds
    the RMSprop goldens' stats to; the parameters after every step: the generator's noise-mask elements (gradient
    within 100 tolerances of zero at some step, at most 2 % of the parameters) within 2 * 3.2 * lr * steps (Adam's
    worst-case step |m_hat / sqrt(v_hat)| <= 1 / sqrt(1 - beta2) ~ 3.2 per unit of lr, times two), every other
    element within the existing parameter tolerance (1e-4 of the vector's max) plus 0.02 * lr * steps."""
    case = Case("tiny_qmix_adam")
    z = case.z
    aux = np.load(os.path.join(GOLDEN, "tiny_qmix_adam_state.npz"))
    lr = float(aux["lr"])
    mask = np.unpackbits(aux["noise_mask"])[:z["step_params"].shape[1]].astype(bool)
    share = float(mask.mean())
    assert lr == LR and share <= 0.02 and abs(share - float(aux["noise_share"])) < 1e-12
    args, buf, mac, learner, logger = build(case, optimizer="adam")
    np.random.seed(case.sampler_seed)
    rec, bad, after = [], [], []
    for k in range(case.steps):
        batch = buf.sample(case.B)
        assert np.array_equal(batch.ep_ids_np, z["ids"][k]), "sampler ids diverged from the reference"
        learner.train(batch[:, :batch.max_t_filled()], 1000 * k, case.episodes[k])
        after.append(flat_params(learner))
        st = learner.last_stats()
        r = dict(step=k)
        for s_ in P.STATS:
            ref = float(z["stat_" + s_][k])
            err = abs(st[s_] - ref) / max(abs(ref), 1e-12)
            tol = P.LOSS_RTOL + 1e-6 / max(abs(ref), 1e-6)
            r["rel_err_" + s_] = err
            print("adam golden step {} {}: {:.7g} vs {:.7g} (rel {:.3g}, tol {:.3g})".format(k, s_, st[s_], ref, err,
                                                                                             tol))
            if not err <= tol:
                bad.append((k, s_, st[s_], ref))
        ref_p = z["step_params"][k].astype(np.float64)
        d = np.abs(flat_params(learner).astype(np.float64) - ref_p)
        steps = k + 1
        tol_noise = 2 * 3.2 * lr * steps
        tol_clear = 1e-4 * float(np.abs(ref_p).max()) + 0.02 * lr * steps
        r["noise_ratio"] = float(d[mask].max() / tol_noise)
        r["clear_ratio"] = float(d[~mask].max() / tol_clear)
        r["clear_over"] = int((d[~mask] > tol_clear).sum())
        print("adam golden step {} params: noise elements {:.3g} of their bound, the others {:.3g} of theirs".format(
            k, r["noise_ratio"], r["clear_ratio"]))
        if not (r["noise_ratio"] <= 1 and r["clear_ratio"] <= 1):
            bad.append((k, "params", r["noise_ratio"], r["clear_ratio"], r["clear_over"]))
        rec.append(r)
    m, v = moments(learner)
    out = dict(noise_share=share, worst_noise_ratio=max(r["noise_ratio"] for r in rec),
               worst_clear_ratio=max(r["clear_ratio"] for r in rec), exp_avg_final_rel=rel(m, aux["exp_avg_final"]),
               exp_avg_sq_final_rel=rel(v, z["sqavg_final"]), steps=rec)
    print("adam golden: mask share {:.3%}, final exp_avg rel {:.3g}, exp_avg_sq rel {:.3g}".format(
        share, out["exp_avg_final_rel"], out["exp_avg_sq_final_rel"]))
    if os.environ.get("MQ_PARITY_DIR"):
        os.makedirs(os.environ["MQ_PARITY_DIR"], exist_ok=True)
        with open(os.path.join(os.environ["MQ_PARITY_DIR"], "parity_adam.json"), "w") as f:
            json.dump(out, f, indent=1)
    assert not bad, bad
    # the update of step 2 (episode 200) ran, and step 3 moved on from it
    assert np.array_equal(flat_targets(learner), after[2]) and not np.array_equal(after[3], after[2])


# ---------------------------------------------------------------------------------------------- 5. composition
def outputs(learner):
    th.cuda.synchronize()
    m, v = moments(learner)
    return dict(grads=flat_grads(learner), params=flat_params(learner), m=m, v=v, stats=learner._stats.cpu().numpy())


def assert_bitwise(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def run_steps(case, steps, **over):
    args, buf, mac, learner, logger = build(case, optimizer="adam", **over)
    np.random.seed(case.sampler_seed)
    for k in range(steps):
        learner.train(sampled(buf, case, k), 1000 * k, case.episodes[k])
    return learner


def test_two_runs_are_bitwise_equal(cases):
    case = get_case(cases, "tiny_qmix")
    assert_bitwise(outputs(run_steps(case, 3)), outputs(run_steps(case, 3)))


def test_data_parallel_norm_path_single_rank(cases):
    """tests/test_gpu_parity.py's test of the same name, with Adam: the norm recomputed by sumsq_kernel."""
    case = get_case(cases, "tiny_qmix")
    outs = []
    for force in (False, True):
        args, buf, mac, learner, logger = build(case, optimizer="adam")
        learner.force_dp_norm = force
        np.random.seed(case.sampler_seed)
        for k in range(2):
            learner.train(sampled(buf, case, k), 1000 * k, case.episodes[k])
        outs.append((flat_params(learner), learner.last_stats()["grad_norm"]))
    assert rel(outs[1][0], outs[0][0]) < 1e-6
    assert abs(outs[1][1] - outs[0][1]) <= 1e-5 * abs(outs[0][1])


def test_native_communicator_world1_runs_the_adam_apply(cases, monkeypatch):
    """An attached RCCL communicator (world 1: the all-reduce is the identity) in front of the Adam apply."""
    from pymarl_amd.components.episode_buffer import SampledBatch
    from tests.test_gpu_native_comm import _unique_id
    monkeypatch.setenv("NCCL_SOCKET_IFNAME", "lo")
    case = get_case(cases, "tiny_qmix")
    args, buf, mac, learner, logger = build(case, optimizer="adam")
    gb = SampledBatch(buf, case.z["ids"][0])
    gb = gb[:, :gb.max_t_filled()]
    h = learner._get_handle(gb)
    assert h.lib.mq_comm_attach(h.h, _unique_id(h.lib), 0, 1) == 0, h.lib.mq_last_error()
    train_checked(learner, gb, 0, case.episodes[0], 0, "native comm world 1")
    assert h.lib.mq_comm_detach(h.h) == 0


def test_td_lambda_two_layer_hypernet_per_and_adam_together():
    from tests import hyper2_ref as R
    from tests.test_gpu_per import make_per_buffer
    case = R.GoldenCase2()
    args, buf, mac, learner, logger = build(case, optimizer="adam", q_targets="td_lambda", td_lambda=0.8,
                                            **case.over())
    pbuf = make_per_buffer(case, per_alpha=0.6, per_beta=0.4, per_eps=1e-6, seed=5)
    pbuf.load_arrays(case.data)
    prio0 = pbuf.prio.clone()
    train_checked(learner, pbuf.sample(case.B), 0, case.episodes[0], 0, "lambda + hyper2 + per + adam")
    plan = learner.last_plan()
    assert plan["per"] == 1 and plan["td_lambda"] == 1 and plan["hyper_layers"] == 2, plan
    assert not th.equal(pbuf.prio, prio0)   # the priority write-back ran
    assert np.isfinite(learner._stats.cpu().numpy()).all()


def test_checkpoint_and_handle_rebuild_keep_the_step_count_and_both_moments(cases, tmp_path):
    """Steps 1, 2, a target update, [save, load into a fresh learner,] step 3: bitwise the same with and without the
    bracket (load_models restores the target agent from agent.th, as the reference does, so both arms update the
    targets first). Then the same with a handle rebuild in front of step 3: a learner whose handle is rebuilt for a
    larger batch (step 3 on six episodes) against one whose handle had that size from the start."""
    from pymarl_amd.components.episode_buffer import SampledBatch
    case = get_case(cases, "tiny_qmix")
    ids = case.z["ids"]

    def step(learner, buf, k, which=None):
        b = SampledBatch(buf, ids[k] if which is None else which)
        learner.train(b[:, :b.max_t_filled()], 1000 * k, case.episodes[k])

    args, buf, mac, a, logger = build(case, optimizer="adam")
    step(a, buf, 0)
    step(a, buf, 1)
    a._update_targets()
    th.cuda.synchronize()
    a.save_models(str(tmp_path))
    sd = th.load(str(tmp_path / "opt.th"), weights_only=True)
    assert [float(sd["state"][i]["step"]) for i in sd["state"]] == [2.0] * len(a.params)
    assert list(sd["state"][0]) == ["step", "exp_avg", "exp_avg_sq"]
    step(a, buf, 2)
    want = outputs(a)

    _, buf2, _, b, _ = build(case, optimizer="adam")
    b.load_models(str(tmp_path))
    b.target_mixer.load_state_dict(b.mixer.state_dict())
    b.last_target_update_episode = a.last_target_update_episode
    assert b._opt_steps == 2 and b._handle is None
    step(b, buf2, 2)
    assert int(b._handle.lib.mq_opt_step(b._handle.h)) == 3
    assert_bitwise(outputs(b), want)

    # a handle rebuild: c's handle is sized for four episodes until step 3 arrives with six; d's had six all along
    every = np.arange(case.n_episodes)
    assert case.n_episodes > case.B
    outs = []
    for batch_size in (case.B, case.n_episodes):
        _, bufc, _, c, _ = build(case, optimizer="adam", batch_size=batch_size)
        step(c, bufc, 0)
        step(c, bufc, 1)
        first = c._handle
        step(c, bufc, 2, which=every)
        assert (c._handle is not first) == (batch_size == case.B)   # rebuilt only in the first arm
        assert int(c._handle.lib.mq_opt_step(c._handle.h)) == 3
        step(c, bufc, 3)
        outs.append(outputs(c))
    assert_bitwise(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------- data parallel
DP_STEPS = 2


def _dp_train(learner, buf, case, record):
    from pymarl_amd.components.episode_buffer import SampledBatch
    for k in range(DP_STEPS):
        gb = SampledBatch(buf, case.z["ids"][k])
        learner.train(gb[:, :gb.max_t_filled()], 1000 * k, case.episodes[k])
        record["stats"].append([learner.last_stats()[s] for s in P.STATS])
        record["grads"].append(flat_grads(learner))
        record["params"].append(flat_params(learner))
        m, v = moments(learner)
        record["m"].append(m)
        record["v"].append(v)


def _dp_worker(rank, world, port, backend, out_path):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), NCCL_SOCKET_IFNAME="lo")
    th.cuda.set_device(rank if backend == "nccl" else 0)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        case = Case("tiny_qmix")
        args, buf, mac, learner, logger = build(case, optimizer="adam", learner_dp=True)
        rec = {"stats": [], "grads": [], "params": [], "m": [], "v": []}
        _dp_train(learner, buf, case, rec)
        th.cuda.synchronize()
        rec["collective"] = [learner.collective()]
        if rank == 0:
            np.savez(out_path, **{k: np.asarray(v) for k, v in rec.items()})
    finally:
        dist.destroy_process_group()


def _two_rank_dp(cases, tmp_path, backend):
    """tests/test_gpu_dp.py's launcher: two ranks, each passing the global sample, against one process. Every rank
    steps from the same reduced gradient, so rank 0's step 0 is torch's Adam on it."""
    import torch.multiprocessing as mp
    from tests.test_gpu_dp import _free_port
    out = str(tmp_path / "dp.npz")
    mp.spawn(_dp_worker, args=(2, _free_port(), backend, out), nprocs=2, join=True)
    dp = np.load(out)
    case = get_case(cases, "tiny_qmix")
    args, buf, mac, learner, logger = build(case, optimizer="adam")
    ref = {"stats": [], "grads": [], "params": [], "m": [], "v": []}
    _dp_train(learner, buf, case, ref)
    assert str(dp["collective"][0]) == ("rccl-native" if backend == "nccl" else "torch.distributed")
    # step 0 from identical state: only the order the two shards' partial sums are added in differs
    assert rel(dp["grads"][0], ref["grads"][0]) < 1e-5
    assert rel(dp["stats"][0], ref["stats"][0]) < 1e-5
    p0 = np.concatenate([x.ravel() for x in list(case.agent_params.values()) + list(case.mixer_params.values())])
    zero = np.zeros_like(p0)
    gate("dp step 0", (dp["params"][0], dp["m"][0], dp["v"][0]), p0, dp["grads"][0], zero, zero, 1)
    gate("dp step 1", (dp["params"][1], dp["m"][1], dp["v"][1]), dp["params"][0], dp["grads"][1], dp["m"][0],
         dp["v"][0], 2)
    for k in range(DP_STEPS):
        assert rel(dp["stats"][k], ref["stats"][k]) < 1e-3, (k, dp["stats"][k], ref["stats"][k])
    assert np.abs(dp["params"][-1] - ref["params"][-1]).max() <= 2 * 3.2 * LR * DP_STEPS


def test_two_rank_dp_equals_single_process(cases, tmp_path):
    """Two ranks on one GPU (gloo on device tensors, as tests/test_gpu_dp.py runs them)."""
    _two_rank_dp(cases, tmp_path, "gloo")


@pytest.mark.skipif(th.cuda.device_count() < 2, reason="the two-rank RCCL case needs two devices")
def test_two_rank_rccl_dp_equals_single_process(cases, tmp_path):
    _two_rank_dp(cases, tmp_path, "nccl")
