"""epymarl's two learner keys on the GPU: soft / step-counted target updates (target_update_interval_or_tau;
soft_update_kernel, mq_soft_update, mq_set_soft_target) and reward standardisation (standardise_rewards;
reward_norm_kernel, mq_set_reward_norm, the MIX_RS tails and td_lambda_rs_kernel), through QLearner.train and the C ABI.

1. mq_soft_update bitwise against torch's CPU fp32 `t * (1.0 - tau) + p * tau`, over sizes and pointer alignments;
2. learner steps with tau: the targets after each step are that recurrence on the previous targets and the step's
   parameters, bitwise; 3. the hard update counted in training steps;
4. reward_norm_kernel against tests/reward_norm_ref.py (float64), under bounds derived below;
5. the MIX_RS tails per gradient block against float64 (tests/ref64.py), fed the GPU's own standardised rewards;
6. TD(lambda) on standardised rewards against tests/lambda_oracle.py; 7. every opt-in at once; 8. checkpoint and
   handle rebuild; 9. without the keys nothing is on.

The bounds of 4, for K successive updates of M rewards each, u = 2^-53:
* mean. The kernel and the reference both form bm = (sum x) / M in float64, in different orders. A float64 sum of M
  terms in any order is within (M - 1) u sum|x| <= (M - 1) M u max|r| of the exact sum, so each bm is within
  (M - 1) u max|r| (+ u for the division) of the exact mean and the two differ by at most 2 M u max|r|. The merge
  mean' = mean + (bm - mean) M / tot moves mean by a fraction M / tot <= 1 of that and adds four roundings of values
  bounded by max|r| on each side; one update therefore contributes at most 2 M u max|r| + 8 u max|r| <= 4 M u max|r|
  for M >= 4, and for M < 4 the two sides perform the same operations in the same order (a sum of at most three
  terms taken by at most three threads, each adding one term to 0) and agree exactly up to the final additions, far
  inside it. Errors of earlier updates are carried with weight count / tot < 1. Over K updates:
  |mean err| <= 4 K M u max|r|.
* var. bv = sum (x - bm)^2 / (M - 1): every term is at most (2 max|r|)^2, but |x - bm| <= max|r| when the rewards
  have one sign, as every case here has, so terms are bounded by max r^2; the sum of M terms in another order and
  the error of bm inside the square (first order: 2 |x - bm| |bm err|, which sums to zero around the exact mean and
  leaves a second-order term) give at most 2 (M - 1) u (M / (M - 1)) max r^2 <= 4 M u max r^2 between the two sides;
  the merge adds delta^2 count M / tot^2 <= max r^2 with relative error of a few u, and the mean error of the previous
  update enters delta^2 with 2 |delta| |mean err| <= 2 max|r| * 4 M u max|r| weighted by count M / tot^2 <= 1/4.
  One update: at most (4 + 2 + 2) M u max r^2. Over K updates: |var err| <= 8 K M u max r^2.
* r_std = (r - mean32) / sqrtf(var32) in fp32 with mean32 = fl(mean'), var32 = fl(var'): rounding mean' moves the
  numerator by at most 2^-24 |mean|, i.e. r_std by 2^-24 |mean| / sqrt(var); rounding var' moves sqrt(var) by a
  relative 2^-25; the subtraction, the square root and the division are correctly rounded, 2^-24 relative each. The
  relative terms add to (3 + 1/2) 2^-24 < 2 * 2^-23 of |r - mean| / sqrt(var):
  |r_std err| <= 2^-23 (|mean| + 2 |r - mean|) / sqrt(var). (The float64 errors above are 2^-29 of this and smaller.)
"""
import ctypes
from collections import OrderedDict

import numpy as np
import pytest
import torch as th

from pymarl_amd import _lib
from pymarl_amd.components.episode_buffer import SampledBatch
from tests import ref64
from tests import reward_norm_ref as R
from tests import test_gpu_parity as P
from tests.golden_utils import Case, SynthCase
from tests.gpu_helpers import build, flat_grads, flat_params, flat_targets, rel, set_switch
from tests.lambda_oracle import LambdaOracleQLearner, td_lambda_returns

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


@pytest.fixture(scope="module")
def cases():
    return {}


def get_case(cases, name):
    if name not in cases:
        cases[name] = Case(name)
    return cases[name]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def sampled(buf, case):
    batch = buf.sample(case.B)
    return batch[:, :batch.max_t_filled()]


def cpu_soft(t, p, tau):
    """The specification's recurrence as torch evaluates it on the CPU in fp32."""
    t, p = th.from_numpy(np.asarray(t, np.float32).copy()), th.from_numpy(np.asarray(p, np.float32).copy())
    return (t * (1.0 - tau) + p * tau).numpy()


# ---------------------------------------------------------------------------------------------- 1. mq_soft_update
SENTINEL = 12345.0
PAD = 8
SIZES = [1, 3, 4, 5, 255, 256, 257, 1027, 262144 + 259]
TAUS = [0.005, 0.25, 1.0]
# (target, online) offsets in floats past a 16-byte boundary: both views from element 1 of a padded buffer (a head
# before the float4 body), aligned, the last element before a boundary, and two that disagree modulo 16 bytes (scalar)
OFFSETS = [(1, 1), (0, 0), (3, 3), (0, 1), (2, 3)]


def gpu_soft(t, p, tau, offs):
    """mq_soft_update on device copies whose pointers sit `offs` floats past a 16-byte boundary; the floats around
    both buffers, and the online values, must come back untouched."""
    lib = _lib.load()
    n = len(t)
    bufs = []
    for a, o in zip((t, p), offs):
        d = th.full((n + 2 * PAD,), SENTINEL, dtype=th.float32, device="cuda")
        assert d.data_ptr() % 16 == 0
        d[4 + o:4 + o + n] = th.from_numpy(np.asarray(a, np.float32))
        bufs.append((d, 4 + o))
    ptr = [ctypes.c_void_p(d.data_ptr() + 4 * o) for d, o in bufs]
    omt, tau32 = float(np.float32(1.0 - tau)), float(np.float32(tau))
    _lib.check(lib.mq_soft_update(ptr[0], ptr[1], n, omt, tau32, _lib.stream_ptr()))
    th.cuda.synchronize()
    out = []
    for d, o in bufs:
        h = d.cpu().numpy()
        assert (h[:o] == SENTINEL).all() and (h[o + n:] == SENTINEL).all(), "a write outside the buffer"
        out.append(h[o:o + n].copy())
    assert same_bits(out[1], p), "the online parameters were written"
    return out[0]


def soft_inputs(n, seed):
    """Values over twelve decades of magnitude, exact zeros, and pairs that cancel."""
    rng = np.random.default_rng(seed)
    mag = lambda: 10.0 ** rng.uniform(-8, 4, n) * rng.choice([-1.0, 1.0], n)  # noqa: E731
    t, p = mag().astype(np.float32), mag().astype(np.float32)
    idx = np.arange(n)
    t[idx % 7 == 3] = 0.0
    p[idx % 11 == 5] = 0.0
    p[idx % 13 == 6] = -t[idx % 13 == 6]
    return t, p


@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("n", SIZES)
def test_soft_update_kernel_bitwise_vs_torch_cpu(n, tau):
    t, p = soft_inputs(n, seed=31 * n + int(1000 * tau))
    want = cpu_soft(t, p, tau)
    outs = [gpu_soft(t, p, tau, o) for o in OFFSETS + [OFFSETS[0]]]
    for o, got in zip(OFFSETS + [OFFSETS[0]], outs):
        assert same_bits(got, want), (n, tau, o, int((bits(got) != bits(want)).sum()))


# ---------------------------------------------------------------------------------------------- 2. learner, soft
@pytest.mark.parametrize("over", [{}, {"force_dp_norm": True}, {"optimizer": "adam"}],
                         ids=["rmsprop", "dp_norm", "adam"])
@pytest.mark.parametrize("name", ["tiny_qmix", "tiny_vdn"])
def test_learner_soft_updates_follow_the_recurrence_bitwise(cases, name, over):
    case = get_case(cases, name)
    tau = 0.25
    over = dict(over)
    force = over.pop("force_dp_norm", False)
    args, buf, mac, learner, logger = build(case, target_update_interval_or_tau=tau, target_update_interval=1, **over)
    learner.force_dp_norm = force
    np.random.seed(case.sampler_seed)
    for k in range(3):
        t0, p0 = flat_targets(learner), flat_params(learner)
        learner.train(sampled(buf, case), 1000 * k, case.episodes[k] + 1000)   # the episode rule would fire
        th.cuda.synchronize()
        p1, t1 = flat_params(learner), flat_targets(learner)
        assert not np.array_equal(p1, p0)
        assert same_bits(t1, cpu_soft(t0, p1, tau)), (name, k)
        assert not np.array_equal(t1, p1) and not np.array_equal(t1, t0)
        plan = learner.last_plan()
        assert plan["soft_target"] == 1 and plan["reward_norm"] == 0, plan
        assert learner.training_steps == k + 1 and learner.last_target_update_episode == 0


# ---------------------------------------------------------------------------------------------- 3. hard, by steps
def test_learner_hard_updates_count_training_steps(cases):
    case = get_case(cases, "tiny_qmix")
    args, buf, mac, learner, logger = build(case, target_update_interval_or_tau=2, target_update_interval=1)
    np.random.seed(case.sampler_seed)
    for k in range(5):
        t0 = flat_targets(learner)
        b = SampledBatch(buf, case.z["ids"][k % case.steps])
        learner.train(b[:, :b.max_t_filled()], 1000 * k, 1000 * (k + 1))   # the episode rule would fire every step
        th.cuda.synchronize()
        step = k + 1
        if step in (2, 4):
            assert same_bits(flat_targets(learner), flat_params(learner)), step
            assert not np.array_equal(flat_targets(learner), t0)
        else:
            assert same_bits(flat_targets(learner), t0), step
            assert not np.array_equal(flat_targets(learner), flat_params(learner))
        assert learner.last_plan()["soft_target"] == 0
    assert learner.training_steps == 5 and learner.last_target_update_step == 4
    assert learner.last_target_update_episode == 0


# ---------------------------------------------------------------------------------------------- 4. reward_norm_kernel
def shorten(data, e, L):
    """Episode e of a make_replay dict cut to L transitions, as make_replay writes a short episode."""
    T = data["reward"].shape[1] - 1
    assert 1 <= L < T
    data["terminated"][e] = 0
    data["terminated"][e, L - 1, 0] = 1
    data["reward"][e, L:] = 0.0
    data["filled"][e, L + 1:] = 0
    for k in ("obs", "state", "avail_actions", "actions", "actions_onehot"):
        data[k][e, L + 1:] = 0


# name: (SynthCase shape, mixer, the three updates' episode ids). Each batch is (B, t_len - 1) = (len(ids), T).
NORM_CASES = OrderedDict([
    ("M1", (dict(n=2, A=3, O=4, S=5, T=1, B=1, n_episodes=3), "vdn", [[0], [2], [1]])),
    ("ragged_3x5", (dict(n=3, A=5, O=6, S=7, T=5, B=3, n_episodes=4), "qmix", [[0, 1, 0], [3, 2, 1], [1, 3, 3]])),
    ("5x60", (dict(n=2, A=3, O=4, S=5, T=60, B=5, n_episodes=7), "vdn", [[0, 1, 2, 3, 4], [6, 5, 4, 3, 2],
                                                                         [1, 3, 5, 0, 6]])),
    ("9x130", (dict(n=2, A=3, O=4, S=5, T=130, B=9, n_episodes=11), "vdn",
               [list(range(9)), list(range(2, 11)), [10, 0, 9, 1, 8, 2, 7, 3, 6]])),
    # M = 8400 > RN_THREADS * RN_REG = 8192: past the kernel's register-cached form, the three re-reading passes
    ("70x120", (dict(n=2, A=3, O=4, S=5, T=120, B=70, n_episodes=72), "vdn",
                [list(range(70)), list(range(2, 72)), list(range(71, 1, -1))])),
])


def norm_case(name):
    shape, mixer, ids = NORM_CASES[name]
    case = SynthCase("norm_" + name, steps=3, mixer=mixer, ragged=False, **shape)
    if name == "ragged_3x5":
        shorten(case.data, 1, 2)   # one episode of length 2; id 0 (full length) is drawn twice in the first batch
        shorten(case.data, 2, 4)
    return case, ids


def run_norm(name):
    case, ids = norm_case(name)
    args, buf, mac, learner, logger = build(case, standardise_rewards=True)
    rec = []
    for k, e in enumerate(ids):
        b = SampledBatch(buf, np.asarray(e))
        b = b[:, :b.max_t_filled()]
        assert (b.batch_size, b.t_len - 1) == (len(e), case.T)
        learner.train(b, 1000 * k, 8 * k)
        assert learner.last_plan()["reward_norm"] == 1
        rs = learner.last_intermediate(8).cpu().numpy()
        rec.append((learner.reward_stats(), rs, learner._grad.cpu().numpy().copy()))
    return case, ids, rec


@pytest.mark.parametrize("name", list(NORM_CASES))
def test_reward_norm_kernel_vs_float64_reference(name):
    case, ids, rec = run_norm(name)
    T = case.T
    state = R.INIT
    rmax = float(np.abs(case.data["reward"]).max())
    assert (case.data["reward"] >= 0).all()   # one sign: the variance bound's |x - bm| <= max|r|
    for k, e in enumerate(ids):
        x = case.data["reward"][np.asarray(e)][:, :T]   # (B, T, 1) float32, padded steps included
        M = x.size
        assert M == len(e) * T
        state, want = R.standardise(state, x)
        got, rs, _ = rec[k]
        K = k + 1
        err_m, err_v = abs(got["mean"] - state[0]), abs(got["var"] - state[1])
        bound_m, bound_v = 4 * K * M * U * rmax, 8 * K * M * U * rmax * rmax
        bound_r = 2.0 ** -23 * (abs(state[0]) + 2 * np.abs(x.astype(np.float64) - state[0])) / np.sqrt(state[1])
        err_r = np.abs(rs.astype(np.float64) - want)
        print("reward_norm {} update {}: M {} mean err {:.3g} (bound {:.3g}) var err {:.3g} (bound {:.3g}) "
              "r_std err / bound {:.3g}".format(name, k, M, err_m, bound_m, err_v, bound_v,
                                                float((err_r / bound_r).max())))
        assert rs.shape == (len(e), T, 1) and rs.dtype == np.float32 and np.isfinite(rs).all()
        assert got["count"] == state[2]
        assert err_m <= bound_m, (name, k, got, state)
        assert err_v <= bound_v, (name, k, got, state)
        assert (err_r <= bound_r).all(), (name, k, float((err_r / bound_r).max()))
        assert got["var"] > 0
    if name == "ragged_3x5":
        assert int(case.data["filled"][1].sum()) == 3 and ids[0].count(0) == 2
        assert (case.data["reward"][1, 2:] == 0).all()   # the padded steps' zeros were counted (M is B T)
    if name == "M1":
        assert rec[0][0]["count"] == 1e-4 + 1


def test_reward_norm_two_runs_are_bitwise_equal():
    for name in ("ragged_3x5", "9x130"):
        _, _, a = run_norm(name)
        _, _, b = run_norm(name)
        for (sa, ra, ga), (sb, rb, gb) in zip(a, b):
            assert sa == sb and same_bits(ra, rb) and same_bits(ga, gb), name


# ---------------------------------------------------------------------------------------------- 5. the MIX_RS tails
def with_rewards(nb, rs):
    """A copy of the numpy batch whose reward[:, :-1] is `rs` (B, T, 1) and whose last step is 0."""
    out = OrderedDict(nb)
    r = np.zeros_like(nb["reward"])
    r[:, :-1] = rs
    out["reward"] = r
    return out


# row: (ref64 shape, mixer, MQ_PLAN switches, the mixer-tail kernel the plan must report)
TAIL_ROWS = OrderedDict([
    ("base_qmix", ("base", "qmix", {}, "fast16")),
    ("base_vdn", ("base", "vdn", {}, "fast16")),
    ("base_iql", ("base", "none", {}, "fast16")),
    ("fast32", ("fast32", "qmix", {}, "fast32")),
    ("stream", ("stream", "qmix", {}, "stream")),
    # n = 3, A = 9 is a fast-mixer shape and mix_generic only replaces the staged (stream) mixer, so this row's plan
    # stays fast16, as tests/test_gpu_grad_blocks.py's base_generic row notes; the row after it reaches mix_kernel<false>
    ("base_mix_generic", ("base", "qmix", {"mix_generic": True}, "fast16")),
    ("generic", ("stream", "qmix", {"mix_generic": True}, "generic")),
])


@pytest.fixture(scope="module")
def synth_cases():
    return {}


@pytest.mark.parametrize("row", list(TAIL_ROWS))
def test_standardised_tails_grad_blocks_vs_ref64(synth_cases, row, monkeypatch):
    """tests/test_gpu_grad_blocks.py's procedure and tolerance, min(1e-5, 16 max(e32, 2e-7)) per block, on steps that
    standardise: the float64 reference and the fp32 oracle train on a copy of the batch whose rewards are the GPU's own
    standardised rewards (intermediate 8, gated by the tests of 4)."""
    from oracle.qlearner_np import OracleQLearner
    from tests.test_gpu_grad_blocks import oracle_clipped
    shape, mixer, switches, mix = TAIL_ROWS[row]
    if (shape, mixer) not in synth_cases:
        synth_cases[shape, mixer] = ref64.synth_case(shape, mixer)
    case = synth_cases[shape, mixer]
    for key, v in switches.items():
        set_switch(monkeypatch, key, v)
    args, buf, mac, learner, logger = build(case, standardise_rewards=True)
    o = OracleQLearner(case.agent_params, case.mixer_params, case.cfg())
    np.random.seed(case.sampler_seed)
    bad = []
    for k in range(2):
        batch = sampled(buf, case)
        nb0, _ = case.batch(k)
        P.oracle_from_learner(o, case, learner)
        params, targets = flat_params(learner), flat_targets(learner)
        learner.train(batch, 1000 * k, case.episodes[k])
        g_gpu = flat_grads(learner)
        plan = learner.last_plan()
        norm_gpu = learner.last_stats()["grad_norm"]
        assert plan["reward_norm"] == 1 and plan["mix"] == mix and plan["td_lambda"] == 0, (row, plan)
        assert np.isfinite(g_gpu).all(), (row, k)
        rs = learner.last_intermediate(8).cpu().numpy()
        assert not np.array_equal(rs, nb0["reward"][:, :-1])
        nb = with_rewards(nb0, rs)
        fw = o.forward(nb)
        r, got, on_gpu = P.classify_decisions(learner, o, nb, fw)
        assert r["dq_flips_outside_ties"] == 0, (row, k, r)
        assert r["relu_flips_outside_ties"] == 0, (row, k, r)
        ref = ref64.ref_step(case, params, targets, nb, cur_max_override=got, relu_override=on_gpu)
        if mixer == "qmix":
            ref64.assert_clear_of_kinks(ref, "{} step {}".format(row, k))
        e32 = ref64.block_errors(oracle_clipped(o, nb, got, on_gpu), ref.clipped, case)
        errs = ref64.block_errors(g_gpu, ref.clipped, case)
        tol = ref64.tolerances(e32)
        ratio = ref64.ratios(errs, e32)
        worst = max(ratio, key=ratio.get)
        norm_err = abs(norm_gpu - ref.norm) / ref.norm
        tm = learner.last_stats()["target_mean"]
        print("{} step {}: worst ratio {:.2f} at {} (err {:.3g}, e32 {:.3g}, tol {:.3g}); grad_norm rel {:.3g}; "
              "target_mean {:.6g} vs {:.6g}".format(row, k, ratio[worst], worst, errs[worst], e32[worst], tol[worst],
                                                    norm_err, tm, ref.stats["target_mean"]))
        bad += [(k, b, e, t) for b, (e, t) in ref64.failures(errs, tol).items()]
        assert norm_err <= 1e-5, (row, k, norm_gpu, ref.norm)
        # target_mean is logged on the standardised scale
        assert abs(tm - ref.stats["target_mean"]) <= 1e-5 * abs(ref.stats["target_mean"]) + 1e-6
    assert not bad, (row, bad)


# ---------------------------------------------------------------------------------------------- 6. TD(lambda)
@pytest.mark.parametrize("name", ["tiny_qmix", "tiny_iql"])
def test_lambda_on_standardised_rewards_teacher_forced(cases, name):
    """tests/test_gpu_td_lambda.run_teacher_forced_lambda's procedure and bands (stats 1e-5 relative + 1e-6, gradient
    1e-4 of the max) with the oracle on the substituted batch; the scan's output is the reference recurrence on RS,
    bit for bit."""
    case = get_case(cases, name)
    lam = 0.8
    args, buf, mac, learner, logger = build(case, q_targets="td_lambda", td_lambda=lam, standardise_rewards=True)
    o = LambdaOracleQLearner(case.agent_params, case.mixer_params, dict(case.cfg(), huber_delta=0.0, td_lambda=lam))
    np.random.seed(case.sampler_seed)
    for k in range(3):
        batch = P.sample_like_reference(buf, case, args, "view")
        nb0, _ = case.batch(k)
        P.set_state_from_oracle(learner, o)
        learner.train(batch, 1000 * k, case.episodes[k])
        st = learner.last_stats()
        plan = learner.last_plan()
        assert plan["td_lambda"] == 1 and plan["reward_norm"] == 1, plan
        rs = learner.last_intermediate(8).cpu().numpy()
        nb = with_rewards(nb0, rs)
        # intermediate 5 is the scan over RS: the reference recurrence on the GPU's own y' and RS, bitwise
        y = learner.last_intermediate(4).cpu().numpy()
        g = learner.last_intermediate(5).cpu().numpy()
        term = nb["terminated"][:, :-1].astype(np.float32)
        mask = nb["filled"][:, :-1].astype(np.float32).copy()
        mask[:, 1:] = mask[:, 1:] * (np.float32(1.0) - term[:, :-1])
        assert np.array_equal(g, td_lambda_returns(rs, term, mask, y, 0.99, lam)), (name, k)
        assert not np.array_equal(g, td_lambda_returns(nb0["reward"][:, :-1], term, mask, y, 0.99, lam))
        fw = o.forward(nb)
        r, got, on_gpu = P.classify_decisions(learner, o, nb, fw)
        assert r["dq_flips_outside_ties"] == 0 and r["relu_flips_outside_ties"] == 0, (name, k, r)
        st_o = o.train(nb, 1000 * k, case.episodes[k], cur_max_override=got, relu_override=on_gpu)
        g_or = np.concatenate([v.ravel() for v in o.last["grads"].values()])
        grad_rel = rel(flat_grads(learner), g_or)
        print("lambda + standardise", name, "step", k, {s_: abs(st[s_] - st_o[s_]) for s_ in P.STATS}, grad_rel)
        for s_ in P.STATS:
            assert abs(st[s_] - st_o[s_]) <= 1e-5 * abs(st_o[s_]) + 1e-6, (name, k, s_, st[s_], st_o[s_])
        assert grad_rel < 1e-4, (name, k)


# ---------------------------------------------------------------------------------------------- 7. together
def run_everything():
    from tests import hyper2_ref
    from tests.test_gpu_per import make_per_buffer
    case = hyper2_ref.GoldenCase2()
    args, buf, mac, learner, logger = build(case, optimizer="adam", q_targets="td_lambda", td_lambda=0.8,
                                            td_loss="huber", huber_delta=1.0, standardise_rewards=True,
                                            target_update_interval_or_tau=0.01, **case.over())
    pbuf = make_per_buffer(case, per_alpha=0.6, per_beta=0.4, per_eps=1e-6, seed=5)
    pbuf.load_arrays(case.data)
    prio0 = pbuf.prio.clone()
    t0 = flat_targets(learner)
    for k in range(3):
        learner.train(pbuf.sample(case.B), 1000 * k, 8 * k)
        plan = learner.last_plan()
        assert (plan["per"], plan["td_lambda"], plan["hyper_layers"], plan["reward_norm"], plan["soft_target"]) == \
            (1, 1, 2, 1, 1), plan
    th.cuda.synchronize()
    assert not th.equal(pbuf.prio, prio0) and not np.array_equal(flat_targets(learner), t0)
    assert int(learner._handle.lib.mq_opt_step(learner._handle.h)) == 3
    out = dict(params=flat_params(learner), targets=flat_targets(learner), grads=flat_grads(learner),
               m=learner._m.cpu().numpy(), v=learner._sq.cpu().numpy(), stats=learner._stats.cpu().numpy(),
               prio=pbuf.prio.cpu().numpy(), rew_ms=learner.rew_ms.cpu().numpy(),
               rs=learner.last_intermediate(8).cpu().numpy(), g=learner.last_intermediate(5).cpu().numpy())
    for k, v in out.items():
        assert np.isfinite(v).all(), k
    return out


def test_every_opt_in_together_is_finite_and_reproducible():
    a, b = run_everything(), run_everything()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------- 8. checkpoint
def test_checkpoint_and_handle_rebuild_keep_statistics_and_counters(cases, tmp_path, caplog):
    """Steps 1 and 2 (the step-counted hard update runs after step 2), [save, load into a fresh learner,] step 3 on
    six episodes where the handle was built for four: bitwise the same with and without the bracket. load_models
    restores the target agent from agent.th and leaves the target mixer alone, as the reference does, so the bracket
    sits where targets equal parameters and the target mixer is copied by hand, as tests/test_gpu_adam.py does."""
    case = get_case(cases, "tiny_qmix")
    ids = case.z["ids"]
    over = dict(standardise_rewards=True, target_update_interval_or_tau=2, target_update_interval=10 ** 9)

    def step(learner, buf, k, which=None):
        b = SampledBatch(buf, ids[k] if which is None else which)
        learner.train(b[:, :b.max_t_filled()], 1000 * k, case.episodes[k])

    def outputs(learner):
        th.cuda.synchronize()
        return dict(params=flat_params(learner), targets=flat_targets(learner), grads=flat_grads(learner),
                    sq=learner._sq.cpu().numpy(), stats=learner._stats.cpu().numpy(),
                    rew_ms=learner.rew_ms.cpu().numpy(),
                    steps=np.array([learner.training_steps, learner.last_target_update_step]))

    every = np.arange(case.n_episodes)
    assert case.n_episodes > case.B
    _, buf, _, a, _ = build(case, **over)
    step(a, buf, 0)
    step(a, buf, 1)
    assert same_bits(flat_targets(a), flat_params(a)) and a.last_target_update_step == 2
    a.save_models(str(tmp_path))
    ms = th.load(str(tmp_path / "rew_ms.th"), weights_only=True)
    assert ms == a.reward_stats() and ms["count"] > 2 * case.B
    first = a._handle
    step(a, buf, 2, which=every)
    assert a._handle is not first   # rebuilt for the larger batch: the statistics pointer was set again
    want = outputs(a)
    assert want["steps"].tolist() == [3, 2] and want["rew_ms"][2] > ms["count"]

    _, buf2, _, b, _ = build(case, **over)
    b.load_models(str(tmp_path))
    b.target_mixer.load_state_dict(b.mixer.state_dict())
    assert b.reward_stats() == ms and (b.training_steps, b.last_target_update_step) == (2, 2) and b._handle is None
    step(b, buf2, 2, which=every)
    got = outputs(b)
    for k in want:
        assert np.array_equal(want[k], got[k]), k
    assert b.reward_stats() == a.reward_stats()

    # a checkpoint without rew_ms.th: one warning, fresh statistics
    (tmp_path / "rew_ms.th").unlink()
    _, _, _, c, _ = build(case, **over)
    with caplog.at_level("WARNING"):
        c.load_models(str(tmp_path))
    assert c.reward_stats() == dict(mean=0.0, var=1.0, count=1e-4)
    assert len([r_ for r_ in caplog.records if "rew_ms.th" in r_.getMessage()]) == 1


# ---------------------------------------------------------------------------------------------- 9. off means off
def test_without_the_keys_nothing_is_on(cases):
    case = get_case(cases, "tiny_qmix")
    args, buf, mac, learner, logger = build(case)
    np.random.seed(case.sampler_seed)
    t0 = flat_targets(learner)
    learner.train(sampled(buf, case), 0, case.episodes[0])
    plan = learner.last_plan()
    assert plan["reward_norm"] == 0 and plan["soft_target"] == 0, plan
    assert same_bits(flat_targets(learner), t0)
    with pytest.raises(_lib.MQError, match="standardise"):
        learner.last_intermediate(8)
    with pytest.raises(_lib.MQError, match="standardise_rewards"):
        learner.reward_stats()
    with pytest.raises(ValueError, match="learner_dp is not supported with standardise_rewards"):
        build(case, standardise_rewards=True, learner_dp=True)
    # the same through the norm path a data-parallel step takes, before any launch
    _, buf2, _, l2, _ = build(case, standardise_rewards=True)
    l2.force_dp_norm = True
    with pytest.raises(ValueError, match="learner_dp is not supported with standardise_rewards"):
        l2.train(sampled(buf2, case), 0, case.episodes[0])
    assert l2._handle is None and l2.reward_stats() == dict(mean=0.0, var=1.0, count=1e-4)
