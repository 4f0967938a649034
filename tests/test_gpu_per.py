"""GPU checks of prioritized episode replay: the sampler (mq_per_sample, per_sample_kernel), the weighted mixer tail
and the priority write-back (mq_set_per; pymarl_amd/csrc/per_kernels.hpp, mix_kernels.hpp MIX_PER), through the
product path PrioritizedReplayBuffer.sample -> QLearner.train -> libmq_learner.so.

A. the sampler on exact fixtures: ids equal the float64 sampler's, weights to 1e-5, beta = 0 gives exactly 1;
B. the sampler on inexact priorities: every id inside the interval its tau allows, at the kernel's stated chain length;
C. a PER step at weights == 1 is the uniform step on the same ids, bit for bit, for every mixer variant and pass;
D. the weighted step, teacher-forced against PEROracleQLearner (tests/per_oracle.py) in run_teacher_forced's bands;
E. the priority write-back against its float32 restatement applied to the GPU's own |td m| record;
F. a closed loop of sample -> train with an insert in between; G. determinism; H. refusals; I. PER is not sticky;
J. no host synchronisation on the sample / train path.
"""
from collections import OrderedDict

import numpy as np
import pytest
import torch as th

from pymarl_amd import _lib
from pymarl_amd.components.episode_buffer import EpisodeBatch, PrioritizedReplayBuffer, SampledBatch
from pymarl_amd.components.transforms import OneHot
from tests import test_gpu_parity as P
from tests.golden_utils import Case, SynthCase
from tests.gpu_helpers import build, flat_grads, flat_params, make_scheme, rel
from tests.per_oracle import (PEROracleQLearner, chain_len, exact_fixture, interval_violations, per_sample,
                              priority_update)
from tests.test_gpu_td_lambda import SYNTH, learner_mask

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return {}


def get_case(cases, name):
    if name not in cases:
        cases[name] = SynthCase(name, **SYNTH[name]) if name in SYNTH else Case(name)
    return cases[name]


def make_per_buffer(case, n_slots=None, device="cuda", **kw):
    pre = {"actions": ("actions_onehot", [OneHot(out_dim=case.A)])}
    return PrioritizedReplayBuffer(make_scheme(case), {"agents": case.n}, n_slots or case.n_episodes, case.T + 1,
                                   preprocess=pre, device=device, **kw)


def build_per(case, alpha=0.6, beta=0.4, eps=1e-6, seed=5, **over):
    """(args, uniform buffer, prioritized buffer, learner) on the case's replay and weights."""
    args, buf, mac, learner, logger = build(case, **over)
    pbuf = make_per_buffer(case, per_alpha=alpha, per_beta=beta, per_eps=eps, seed=seed)
    pbuf.load_arrays(case.data)
    return args, buf, pbuf, learner


def numpy_batch(case, ids, t_len):
    return OrderedDict((k, v[ids][:, :t_len]) for k, v in case.data.items())


def gpu_sample(prio, n_live, u, alpha, beta):
    lib = _lib.load()
    p = th.as_tensor(np.asarray(prio, np.float32), device="cuda")
    uu = th.as_tensor(np.asarray(u, np.float32), device="cuda")
    ids = th.full((len(u),), -1, dtype=th.int64, device="cuda")
    w = th.full((len(u),), float("nan"), dtype=th.float32, device="cuda")
    _lib.check(lib.mq_per_sample(_lib.ptr(p), n_live, _lib.ptr(uu), len(u), alpha, beta, _lib.ptr(ids), _lib.ptr(w),
                                 _lib.stream_ptr()))
    return ids.cpu().numpy(), w.cpu().numpy()


# ------------------------------------------------------------------------------------------- A. sampler, exact
@pytest.mark.parametrize("B", [1, 4, 32])
@pytest.mark.parametrize("N", [1, 7, 64, 1025, 5000])
def test_sampler_exact(N, B):
    """N = 5000 with B = 32 is the bench shape; every case carries stale slots >= N holding 1e6."""
    prio, u = exact_fixture(N, B, seed=100 * N + B, n_slots=N + 9, stale=1e6)
    ref_ids, _, s = per_sample(prio, N, u, 1.0, 0.0, np.float64)
    ids, w = gpu_sample(prio, N, u, 1.0, 0.0)
    assert np.array_equal(ids, ref_ids), (N, B, ids, ref_ids)
    assert ids.max() < N
    assert np.array_equal(w, np.ones(B, np.float32))   # beta = 0: exactly 1
    for beta in (0.4, 1.0):
        ids_b, w_b = gpu_sample(prio, N, u, 1.0, beta)
        _, w64, _ = per_sample(prio, N, u, 1.0, beta, np.float64)
        err = float((np.abs(w_b.astype(np.float64) - w64) / w64).max())
        print("sampler weights", N, B, beta, "max rel err", err, "min w", float(w64.min()))
        assert np.array_equal(ids_b, ref_ids)
        assert err <= 1e-5, (N, B, beta, err)


def test_sampler_tau_on_a_boundary_takes_the_next_episode():
    prio, u = exact_fixture(64, 4, seed=7, boundary=True)
    ref_ids, _, s = per_sample(prio, 64, u, 1.0, 0.0, np.float64)
    hit = np.nonzero(s["cum"] == s["tau"][0])[0]
    assert len(hit) == 1 and ref_ids[0] == hit[0] + 1
    ids, _ = gpu_sample(prio, 64, u, 1.0, 0.0)
    assert np.array_equal(ids, ref_ids)


# ----------------------------------------------------------------------------------------- B. sampler, inexact
@pytest.mark.parametrize("N,B", [(5, 4), (33, 32), (64, 4), (64, 32)])
def test_sampler_inexact_ids_lie_in_their_intervals(N, B):
    rng = np.random.RandomState(17 * N + B)
    prio = np.exp(rng.uniform(np.log(1e-6), np.log(1e3), size=N)).astype(np.float32)
    prio[0], prio[-1] = 1e-6, 1e3
    u = rng.random_sample(B).astype(np.float32)
    ids, w = gpu_sample(prio, N, u, 0.6, 0.4)
    bad = interval_violations(ids, prio, N, u, 0.6, chain_len(N))
    ref_ids, w64, _ = per_sample(prio, N, u, 0.6, 0.4, np.float64)
    print("sampler inexact", N, B, "ids differing from float64:", int((ids != ref_ids).sum()), "violations", bad)
    assert not bad
    # weights of the draws that agree with float64, in exact test A's band: two powf (2 ulp each), the total (D 2^-24),
    # two divisions and the normalisation by the maximum, which carries the same errors: < 3e-6 relative
    same = ids == ref_ids
    assert same.any()
    assert (np.abs(w[same].astype(np.float64) - w64[same]) / w64[same]).max() <= 1e-5
    assert w.max() == 1.0 and w.min() > 0.0


# --------------------------------------------------------------------- C. weights == 1 is the uniform step, bitwise
UNIT_CASES = [
    ("tiny_qmix", {}, "fast16", 0), ("tiny_vdn", {}, "fast16", 0), ("tiny_iql", {}, "fast16", 0),
    ("cfg2_qmix", {}, "fast16", 0), ("lam_fast32", {}, "fast32", 0), ("cfg3_vdn", {}, "stream", 0),
    ("lam_generic", {}, "generic", 0),
    ("tiny_qmix", dict(q_targets="td_lambda", td_lambda=0.8), "fast16", 1),
    ("tiny_qmix", dict(td_loss="huber", huber_delta=1.0), "fast16", 0),
]


def step_outputs(learner):
    th.cuda.synchronize()
    return dict(grads=flat_grads(learner), params=flat_params(learner), sq=learner._sq.cpu().numpy().copy(),
                stats=learner._stats.cpu().numpy().copy(), acts=learner.last_cur_max_actions().cpu().numpy().copy())


@pytest.mark.parametrize("name,over,mix,lam", UNIT_CASES, ids=[c[0] + ("_" + "_".join(c[1]) if c[1] else "")
                                                              for c in UNIT_CASES])
def test_unit_weights_are_the_uniform_step_bitwise(cases, name, over, mix, lam):
    case = get_case(cases, name)
    args, buf, pbuf, learner = build_per(case, beta=0.0, **over)
    pb = pbuf.sample(case.B)
    learner.train(pb, 0, case.episodes[0])
    got = step_outputs(learner)
    plan = learner.last_plan()
    assert plan["per"] == 1 and plan["mix"] == mix and plan["td_lambda"] == lam and plan["inline_ids"] == 0, plan
    assert np.array_equal(pb.weights.cpu().numpy(), np.ones(case.B, np.float32))
    ids = pb.ep_ids.cpu().numpy()   # read back in the test only
    assert pb.t_len == int(case.data["filled"].sum(1).max())

    _, buf2, _, uniform, _ = build(case, **over)
    uniform.train(SampledBatch(buf2, ids, pb.t_len), 0, case.episodes[0])
    ref = step_outputs(uniform)
    plan2 = uniform.last_plan()
    assert plan2["per"] == 0 and plan2["mix"] == mix, plan2
    assert np.isfinite(ref["grads"]).all() and np.abs(ref["grads"]).max() > 0
    for k in ref:
        assert np.array_equal(got[k], ref[k]), (name, k)


# --------------------------------------------------------------------------------- D. weighted step, teacher-forced
def run_teacher_forced_per(case, steps, lam=0.0):
    """tests/test_gpu_td_lambda.run_teacher_forced_lambda with PEROracleQLearner on the other side and the batch drawn
    by the sampler at beta = 1 from skewed priorities (one episode holds half of the mass)."""
    name = case.name
    over = dict(q_targets="td_lambda", td_lambda=lam) if lam else {}
    args, buf, pbuf, learner = build_per(case, alpha=1.0, beta=1.0, **over)
    o = PEROracleQLearner(case.agent_params, case.mixer_params, dict(case.cfg(), td_lambda=lam))
    N = case.n_episodes
    rec = []
    for k in range(steps):
        skew = th.ones(N, device="cuda")
        skew[k] = float(N)
        pbuf.prio[:N] = skew
        pb = pbuf.sample(case.B)
        ids, w = pb.ep_ids.cpu().numpy(), pb.weights.cpu().numpy()
        assert w.min() < 0.35 and w.max() == 1.0, (name, k, w)   # a kernel that ignored W would fail below
        nb = numpy_batch(case, ids, pb.t_len)
        P.set_state_from_oracle(learner, o)
        o.weights = w
        p_prev, sq_prev = o.flat("params").astype(np.float64), o.flat("sq").astype(np.float64)
        fw = o.forward(nb)
        learner.train(pb, 1000 * k, case.episodes[k])
        st = learner.last_stats()
        plan = learner.last_plan()
        assert plan["per"] == 1 and plan["td_lambda"] == int(lam > 0), (name, plan)
        r, got, on_gpu = P.classify_decisions(learner, o, nb, fw)
        r["step"] = k
        assert r["dq_flips_outside_ties"] == 0, (name, k, r)
        assert r["relu_flips_outside_ties"] == 0, (name, k, r)
        st_o = o.train(nb, 1000 * k, case.episodes[k], cur_max_override=got, relu_override=on_gpu)
        g_or = np.concatenate([v.ravel() for v in o.last["grads"].values()])
        g_gpu = flat_grads(learner)
        for s_ in P.STATS:
            r["err_" + s_] = abs(st[s_] - st_o[s_])
            r["band_" + s_] = 1e-5 * abs(st_o[s_]) + 1e-6
        r["grad_rel"] = rel(g_gpu, g_or)
        rec.append(r)
        print("teacher per", name, "step", k, "min w", float(w.min()),
              {kk: v for kk, v in r.items() if kk.startswith(("err_", "grad_"))})
        for s_ in P.STATS:
            assert r["err_" + s_] <= r["band_" + s_], (name, k, s_, st[s_], st_o[s_])
        assert r["grad_rel"] < 1e-4, (name, k)
        g64 = g_gpu.astype(np.float64)
        sq_exp = 0.99 * sq_prev + 0.01 * g64 * g64
        p_exp = p_prev - 5e-4 * g64 / (np.sqrt(sq_exp) + 1e-5)
        assert rel(learner._sq.cpu().numpy(), sq_exp) < 1e-5, (name, k)
        assert rel(flat_params(learner), p_exp) < 1e-6, (name, k)
        assert np.abs(flat_params(learner) - o.flat("params")).max() <= 20 * 5e-4, (name, k)
    P.write_record("teacher_per" + ("_lambda" if lam else ""), name, rec)


@pytest.mark.parametrize("name", ["tiny_qmix", "tiny_vdn", "tiny_iql", "cfg1_qmix", "cfg2_qmix"])
def test_per_teacher_forced(cases, name):
    run_teacher_forced_per(get_case(cases, name), 3)


def test_per_teacher_forced_lambda(cases):
    run_teacher_forced_per(get_case(cases, "tiny_qmix"), 3, lam=0.8)


# -------------------------------------------------------------------------------------- E. priority write-back
@pytest.mark.parametrize("name", ["tiny_qmix", "tiny_iql", "lam_short"])
def test_priority_write_back(cases, name):
    case = get_case(cases, name)
    eps = 1e-3
    args, buf, pbuf, learner = build_per(case, alpha=1.0, beta=0.4, eps=eps)
    N = case.n_episodes
    lens = case.data["filled"].sum(1).reshape(-1)
    hot = int(np.argmin(lens))   # lam_short: the episode of one transition
    if name == "lam_short":
        assert lens[hot] == 2
    # the hot episode holds 60 % of the mass and every draw sits in the middle of its stratum (u = 0.5): at least
    # floor(0.6 B) >= 2 draws fall into it and at least one outside
    start = np.linspace(0.5, 1.5, N).astype(np.float32)
    start[hot] = 0.0
    start[hot] = np.float32(1.5 * start.sum())
    pbuf.prio[:N] = th.from_numpy(start).cuda()
    pm0 = np.float32(1e6 if name == "tiny_iql" else 1e-4)   # above every new priority / below them all (eps = 1e-3)
    pbuf.prio_max.fill_(float(pm0))
    pb = pbuf.sample(case.B, u=np.full(case.B, 0.5, np.float32))
    ids = pb.ep_ids.cpu().numpy()
    assert (ids == hot).sum() >= 2 and len(set(ids.tolist())) >= 2, ids   # a forced duplicate id, and others
    learner.train(pb, 0, case.episodes[0])
    assert learner.last_plan()["per"] == 1
    tda = learner.last_intermediate(6).cpu().numpy()
    nb = numpy_batch(case, ids, pb.t_len)
    _, _, mask = learner_mask(nb)
    assert tda.shape == mask.shape == (case.B, pb.t_len - 1, 1)
    assert np.isfinite(tda).all() and (tda >= 0).all() and tda.max() > 0
    assert np.array_equal(tda[mask == 0], np.zeros_like(tda[mask == 0]))
    want = priority_update(tda[..., 0], mask[..., 0], eps, case.n if case.mixer == "none" else 1)
    after = pbuf.prio.cpu().numpy()
    print("write-back", name, "ids", ids, "new priorities", want)
    assert np.array_equal(after[ids], want)
    rest = np.setdiff1d(np.arange(N), ids)
    assert len(rest) > 0 and np.array_equal(after[rest], start[rest])
    assert np.float32(pbuf.prio_max.cpu().numpy()[0]) == max(pm0, want.max())
    assert (want.max() > pm0) == (name != "tiny_iql")   # the maximum moved in two of the cases, stayed in one


# ------------------------------------------------------------------------------------------------ F. closed loop
def test_closed_loop_with_insert(cases):
    case = get_case(cases, "lam_short")   # 14 episodes
    assert case.n_episodes == 14
    args, buf, mac, learner, logger = build(case)
    pbuf = make_per_buffer(case, n_slots=16, per_alpha=0.6, per_beta=0.4, seed=3)
    pbuf.load_arrays({k: v[:12] for k, v in case.data.items()}, n_episodes=12)
    rng = np.random.RandomState(5)
    run_max = np.float32(1.0)
    for k in range(3):
        N = pbuf.episodes_in_buffer
        before = pbuf.prio.cpu().numpy()
        u = rng.random_sample(case.B).astype(np.float32)
        pb = pbuf.sample(case.B, u=u)
        ids = pb.ep_ids.cpu().numpy()
        assert not interval_violations(ids, before, N, u, 0.6, chain_len(N)), (k, ids)
        assert pb.t_len == int(pbuf.episode_lengths[:N].max())
        learner.train(pb, 1000 * k, 8 * k)
        assert learner.last_plan()["per"] == 1
        after = pbuf.prio.cpu().numpy()
        rest = np.setdiff1d(np.arange(16), ids)
        assert np.array_equal(after[rest], before[rest]) and (after[ids] != before[ids]).all()
        run_max = max(run_max, after[ids].max())
        assert np.float32(pbuf.prio_max.cpu().numpy()[0]) == run_max
        if k == 0:   # two new episodes take the largest priority seen so far
            pre = {"actions": ("actions_onehot", [OneHot(out_dim=case.A)])}
            eb = EpisodeBatch(make_scheme(case), {"agents": case.n}, 2, case.T + 1, preprocess=pre, device="cuda")
            eb.update({k_: v[12:14] for k_, v in case.data.items() if k_ != "actions_onehot"})
            pbuf.insert_episode_batch(eb)
            assert pbuf.episodes_in_buffer == 14
            pm = float(pbuf.prio_max.cpu()[0])
            assert np.array_equal(pbuf.prio.cpu().numpy()[12:14], np.full(2, pm, np.float32))
            assert np.array_equal(pbuf.prio.cpu().numpy()[:12], after[:12])
    assert np.isfinite(flat_params(learner)).all()


# ----------------------------------------------------------------------------------------------- G. determinism
def test_per_loop_is_deterministic(cases):
    case = get_case(cases, "tiny_qmix")
    runs = []
    for _ in range(2):
        args, buf, pbuf, learner = build_per(case, seed=11)
        out = []
        for k in range(3):
            pb = pbuf.sample(case.B)
            learner.train(pb, 1000 * k, case.episodes[k])
            out += [pb.ep_ids.cpu().numpy(), pb.weights.cpu().numpy()]
        out += [pbuf.prio.cpu().numpy(), pbuf.prio_max.cpu().numpy(), flat_params(learner)]
        runs.append(out)
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# -------------------------------------------------------------------------------------------------- H. refusals
def test_refusals(cases):
    case = get_case(cases, "tiny_qmix")
    args, buf, pbuf, learner = build_per(case)
    # a uniform step has no |td m| record
    np.random.seed(case.sampler_seed)
    ub = buf.sample(case.B)
    learner.train(ub[:, :ub.max_t_filled()], 0, 0)
    assert learner.last_plan()["per"] == 0
    with pytest.raises(_lib.MQError, match="prioritized"):
        learner.last_intermediate(6)
    # bad alpha / beta at the draw, bad eps at the step
    for attr, v in (("alpha", -0.5), ("alpha", float("nan")), ("beta", 1.5), ("beta", -0.1)):
        good = getattr(pbuf, attr)
        setattr(pbuf, attr, v)
        with pytest.raises(_lib.MQError, match=attr):
            pbuf.sample(case.B)
        setattr(pbuf, attr, good)
    pb = pbuf.sample(case.B)
    pbuf.eps = 0.0
    with pytest.raises(_lib.MQError, match="eps"):
        learner.train(pb, 0, 0)
    pbuf.eps = 1e-6
    # more live episodes than one draw supports
    lib = _lib.load()
    t = th.ones(8, device="cuda")
    ids = th.zeros(2, dtype=th.int64, device="cuda")
    rc = lib.mq_per_sample(_lib.ptr(t), _lib.PER_MAX_LIVE + 1, _lib.ptr(t), 2, 0.6, 0.4, _lib.ptr(ids), _lib.ptr(t),
                           _lib.stream_ptr())
    with pytest.raises(_lib.MQError, match="n_live"):
        _lib.check(rc)
    # data parallelism
    args2, buf2, pbuf2, dp_learner = build_per(case, learner_dp=True)
    with pytest.raises(ValueError, match="learner_dp"):
        dp_learner.train(pbuf2.sample(case.B), 0, 0)
    with pytest.raises(ValueError):
        pb.shard(0, 2)
    with pytest.raises(ValueError):
        pb.to("cpu")
    # COMA is on-policy: it takes no PER batch (refused before it reads the batch)
    from tests.golden_utils import ComaCase
    from tests.gpu_helpers import build_coma
    coma = build_coma(ComaCase("coma_tiny"))[3]
    with pytest.raises(ValueError, match="on-policy"):
        coma.train(pb, 0, 0)
    # a host-resident buffer
    cpu = make_per_buffer(case, device="cpu")
    cpu.load_arrays(case.data)
    with pytest.raises(_lib.MQError, match="HIP device"):
        cpu.sample(case.B)
    # the refused step left nothing armed, and a good PER step still runs
    learner.train(pbuf.sample(case.B), 0, 0)
    assert learner.last_plan()["per"] == 1
    assert learner.last_intermediate(6).shape == (case.B, pb.t_len - 1, 1)


def test_batch_views(cases):
    """[:, :t] keeps a PER batch a PER batch; materialize() gathers with the device ids."""
    case = get_case(cases, "tiny_qmix")
    args, buf, pbuf, learner = build_per(case)
    pb = pbuf.sample(case.B)
    assert pb.ep_ids_np is None and pb.max_t_filled() == pb.t_len
    cut = pb[:, :pb.t_len - 1]
    assert type(cut) is type(pb) and cut.t_len == pb.t_len - 1 and cut.weights is pb.weights
    assert cut.ep_ids.data_ptr() == pb.ep_ids.data_ptr()
    ids = pb.ep_ids.cpu().numpy()
    mat = pb.materialize()
    assert np.array_equal(mat["obs"].cpu().numpy(), case.data["obs"][ids][:, :pb.t_len])
    assert np.array_equal(pb["reward"].cpu().numpy(), case.data["reward"][ids][:, :pb.t_len])


# ------------------------------------------------------------------------------------------------ I. not sticky
def test_per_is_not_sticky(cases):
    case = get_case(cases, "tiny_qmix")
    args, buf, pbuf, learner = build_per(case)
    learner.train(pbuf.sample(case.B), 0, 0)
    assert learner.last_plan()["per"] == 1
    _, buf2, _, fresh, _ = build(case)   # never saw PER: takes over the first learner's state, then the same step
    with th.no_grad():
        fresh._online.copy_(learner._online)
        fresh._target.copy_(learner._target)
        fresh._sq.copy_(learner._sq)
    np.random.seed(case.sampler_seed)
    ids = np.random.choice(case.n_episodes, case.B, replace=False)
    outs = []
    for lr, b in ((learner, buf), (fresh, buf2)):
        ub = SampledBatch(b, ids)
        lr.train(ub[:, :ub.max_t_filled()], 1000, 0)
        assert lr.last_plan()["per"] == 0
        outs.append(step_outputs(lr))
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k


# ----------------------------------------------------------------------------------------------- J. no host sync
def test_sample_and_train_do_not_synchronise(cases):
    case = get_case(cases, "tiny_qmix")
    args, buf, pbuf, learner = build_per(case, learner_log_interval=10 ** 9)
    learner.log_stats_t = 0
    learner.train(pbuf.sample(case.B), 1, 0)   # the handle and the workspaces exist from here on
    th.cuda.synchronize()
    prev = th.cuda.get_sync_debug_mode()
    th.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):   # the mode is honoured: a device-to-host read raises
            th.ones(1, device="cuda").item()
        for k in range(5):
            learner.train(pbuf.sample(case.B), 2 + k, 0)
    finally:
        th.cuda.set_sync_debug_mode(prev)
    th.cuda.synchronize()
    assert learner.last_plan()["per"] == 1 and np.isfinite(flat_params(learner)).all()
