"""The TD(lambda), prioritized-replay and Huber mixer tails of train(), every gradient block judged on its own scale
against the float64 autograd reference (tests/ref64.py), over all four mixer-tail kernels.

tests/test_gpu_grad_blocks.py's procedure, unchanged: two train() steps per row, step 1 from the GPU's own parameters
and targets after step 0; the GPU's double-Q argmax and fc1 relu decisions differ from the oracle's on near-ties only
(and are then followed), the mixer's abs / relu pre-activations of live rows keep clear of 0; then

    tol(block) = min(1e-5, 16 * max(e32(block), 2e-7))

with e32 the fp32 oracle's (tests/per_oracle.PEROracleQLearner: lambda targets, Huber and weights) clipped gradient
against ref64 on that block, from the same state with the same decisions, batch and weights; grad_norm to 1e-5
relative, the five stats to 1e-5 |ref| + 1e-6, and the plan items the row is there for.

ROWS crosses the kernels (mix_fast_kernel<16> at `base`, <32> at `fast32`, mix_kernel<true> at `stream`,
mix_kernel<false> at `stream` under mix_generic) with the tails of TAILS, and adds `base` with VDN and with no mixer
(the per-agent G layout and the lane-summed |td m| record) under `per` and `lam_per_huber`. Per tail:

* lambda rows: intermediate 5 (the lambda targets) against ref.targets over the live transitions, as one block of its
  own under the same rule, e32 from the oracle's targets. The case (ref64.lambda_case) has an episode of a single
  transition and an unterminated episode of the batch's full length, so the bootstrap y'[L-1] (1 - sum term) is not
  zero; both are asserted on the batch the step trained on.
* PER rows: alpha = 1, beta = 1, one episode holding at least half of the mass, explicit u (per_draw), so the ids and
  the weights are known beforehand; the ids read back equal them, the weights have w.min() < 0.35, w.max() == 1 and
  at least two values. Intermediate 6 (|td m|, summed over the agents without a mixer) against ref.abs_mtd as a block
  of its own, exactly 0 on padded entries.
* RS rows: the reference and the oracle train on the GPU's own standardised rewards (intermediate 8), as
  tests/test_gpu_epymarl_keys.test_standardised_tails_grad_blocks_vs_ref64 does.
* Huber rows: delta (HUBER_DELTA) sits near the median of |td| of the reference's step 0, and at least 10 % of the
  live transitions lie on either side of it at both steps. No margin around |x| = delta is kept: the loss term and
  its derivative clip(x, -delta, delta) are continuous there, so a transition the fp32 kernel puts on the other side
  moves the gradient by rounding only.

The measured err / max(e32, 2e-7) of every block goes to $MQ_PARITY_DIR/parity_tail64_<row>.json.
"""
from collections import OrderedDict

import numpy as np
import pytest

from tests import ref64
from tests import test_gpu_parity as P
from tests.per_oracle import PEROracleQLearner, per_sample

pytestmark = pytest.mark.gpu

LAM = 0.8
# kernel: (ref64 shape, MQ_PLAN switches); the name is what plan["mix"] must report
KERNELS = OrderedDict([
    ("fast16", ("base", {})),
    ("fast32", ("fast32", {})),
    ("stream", ("stream", {})),
    ("generic", ("stream", {"mix_generic": True})),
])
# tail: (lambda, PER, Huber, standardised rewards, the plan items the row must report besides its mix)
TAILS = OrderedDict([
    ("lam", (True, False, False, False, dict(td_lambda=1))),
    ("per", (False, True, False, False, dict(per=1))),
    ("huber", (False, False, True, False, dict())),
    ("lam_per_huber", (True, True, True, False, dict(td_lambda=1, per=1))),
    ("per_rs", (False, True, False, True, dict(per=1, reward_norm=1, td_lambda=0))),
    ("lam_rs", (True, False, False, True, dict(td_lambda=1, reward_norm=1))),
])
# row id: (shape, mixer, switches, tail, mix)
ROWS = OrderedDict(("{}_{}".format(kern, tail), (shape, "qmix", sw, tail, kern))
                   for kern, (shape, sw) in KERNELS.items() for tail in TAILS)
for _mixer, _tag in (("vdn", "vdn"), ("none", "iql")):
    for _tail in ("per", "lam_per_huber"):
        ROWS["{}_{}".format(_tag, _tail)] = ("base", _mixer, {}, _tail, "fast16")
# Rows whose replay is drawn from another seed than the shape's own (SynthCase's 11; ref64.LAMBDA_SEEDS for the lambda
# rows), because at that one a hypernet output of a live row lies within ref64.KINK_EPS of 0 at step 1.
DATA_SEEDS = {"fast16_huber": 12}
# Huber's delta per row: the median of |td mask| over the live transitions of ref_step's step 0 at the case's initial
# weights, unweighted (tests/test_ref64_host.py::test_tail_rows_hold_their_preconditions recomputes it), rounded to a
# multiple of 1/16 so that float32 carries it exactly.
HUBER_DELTA = {
    "fast16_huber": 2.1875, "fast16_lam_per_huber": 3.125,    # medians 2.205, 3.140
    "fast32_huber": 3.3125, "fast32_lam_per_huber": 3.875,    # 3.324, 3.882
    "stream_huber": 5.8125, "stream_lam_per_huber": 6.0625,   # 5.799, 6.078
    "generic_huber": 5.8125, "generic_lam_per_huber": 6.0625,
    "vdn_lam_per_huber": 1.875, "iql_lam_per_huber": 1.6875,  # 1.897, 1.679
}


def case_key(row):
    shape, mixer, _, tail, _ = ROWS[row]
    return shape, mixer, TAILS[tail][0], DATA_SEEDS.get(row)


def tail_case(row):
    """The row's case: ref64.lambda_case for the lambda rows (a copy the one-step rows do not share)."""
    shape, mixer, lam, seed = case_key(row)
    if lam:
        return ref64.lambda_case(shape, mixer, data_seed=seed)
    return ref64.synth_case(shape, mixer) if seed is None else ref64.synth_case(shape, mixer, data_seed=seed)


def per_draw(case, k, need=()):
    """Step k's draw, decided on the CPU: priorities (episode k holds max(N, 4) against 1 each, at least half of the
    mass) and u, multiples of 2^-8 from the first seed at which the float64 sampler draws every episode of `need` and
    at least two different weights. Everything the sampler computes from them is exact in float32, so the GPU's ids
    must equal the ones returned here. Returns (prio, u, ids, weights)."""
    N, B = case.n_episodes, case.B
    prio = np.ones(N, np.float32)
    prio[k % N] = max(N, 4)
    for seed in range(256):
        u = (np.random.RandomState(seed).randint(0, 256, size=B) / 256.0).astype(np.float32)
        ids, w, _ = per_sample(prio, N, u, 1.0, 1.0, np.float64)
        if w.min() < 0.35 and w.max() == 1.0 and all(e in ids for e in need):
            return prio, u, ids, w
    raise AssertionError("no draw of {} with episodes {} at step {}".format(case.name, need, k))


def lambda_needs(case):
    """(the episode of one transition, the unterminated episode of full length) of a ref64.lambda_case."""
    lens = case.data["filled"].sum(1).reshape(-1)
    short, full = int(np.argmin(lens)), int(np.argmax(lens))
    assert lens[short] == 2 and case.data["terminated"][full].sum() == 0
    return short, full


def one_block(got, ref, live):
    """max|got - ref| / max|ref| over the live entries: a record judged as one block."""
    return float(np.abs(np.asarray(got, np.float64) - ref)[live].max() / np.abs(ref[live]).max())


def preconditions(ref, nb, lam, huber, what):
    """What keeps a row from passing vacuously, on the float64 reference of the batch the step trained on."""
    live = ref.mask > 0
    if lam:
        assert int(nb["filled"].sum(1).min()) == 2, what        # an episode of a single transition
        assert np.abs(ref.bootstrap).max() > 1e-3, what         # an unterminated episode of full length
    if huber:
        below = float((np.abs(ref.mtd)[live] <= huber).mean())
        assert 0.1 <= below <= 0.9, (what, below)               # both regimes are live


@pytest.fixture(scope="module")
def tail_cases():
    return {}


@pytest.mark.parametrize("row", list(ROWS))
def test_tail_blocks_vs_ref64(tail_cases, row, monkeypatch):
    import torch as th
    from tests.gpu_helpers import build, flat_grads, flat_params, flat_targets, set_switch
    from tests.test_gpu_epymarl_keys import with_rewards
    from tests.test_gpu_per import build_per, numpy_batch
    from oracle.qlearner_np import clip_grad_norm
    shape, mixer, switches, tail, mix = ROWS[row]
    lam, per, hub, rs, want = TAILS[tail]
    if case_key(row) not in tail_cases:
        tail_cases[case_key(row)] = tail_case(row)
    case = tail_cases[case_key(row)]
    delta = HUBER_DELTA[row] if hub else 0.0
    for key, v in switches.items():   # read once, at handle creation
        set_switch(monkeypatch, key, v)
    over = {}
    if lam:
        over.update(q_targets="td_lambda", td_lambda=LAM)
    if hub:
        over.update(td_loss="huber", huber_delta=delta)
    if rs:
        over.update(standardise_rewards=True)
    if per:
        args, buf, pbuf, learner = build_per(case, alpha=1.0, beta=1.0, **over)
    else:
        args, buf, mac, learner, logger = build(case, **over)
    o = PEROracleQLearner(case.agent_params, case.mixer_params,
                          dict(case.cfg(), td_lambda=LAM if lam else 0.0, huber_delta=delta))
    tails = dict(td_lambda=LAM if lam else None, huber_delta=delta)
    need = lambda_needs(case) if lam else ()
    np.random.seed(case.sampler_seed)
    rec, bad = [], []
    for k in range(2):
        what = "{} step {}".format(row, k)
        w = None
        if per:
            prio, u, want_ids, want_w = per_draw(case, k, need)
            pbuf.prio[:case.n_episodes] = th.from_numpy(prio).cuda()
            batch = pbuf.sample(case.B, u=u)
            ids, w = batch.ep_ids.cpu().numpy(), batch.weights.cpu().numpy()
            assert np.array_equal(ids, want_ids), (what, ids, want_ids)
            assert w.min() < 0.35 and w.max() == 1.0 and len(set(w.tolist())) >= 2, (what, w)
            assert np.abs(w - want_w).max() <= 1e-5, (what, w, want_w)
            nb = numpy_batch(case, ids, batch.t_len)
        else:
            batch = buf.sample(case.B)
            batch = batch[:, :batch.max_t_filled()]
            nb, _ = case.batch(k)
        P.oracle_from_learner(o, case, learner)   # step 1: the GPU's own parameters and targets after step 0
        o.weights = w
        params, targets = flat_params(learner), flat_targets(learner)
        learner.train(batch, 1000 * k, case.episodes[k])
        g_gpu = flat_grads(learner)
        plan = learner.last_plan()
        st = learner.last_stats()
        assert np.isfinite(g_gpu).all(), what
        assert plan["mix"] == mix, (row, plan)
        for key, v in want.items():
            assert plan[key] == v, (row, key, plan)
        if rs:
            r8 = learner.last_intermediate(8).cpu().numpy()
            assert not np.array_equal(r8, nb["reward"][:, :-1])
            nb = with_rewards(nb, r8)
        fw = o.forward(nb)
        r, got, on_gpu = P.classify_decisions(learner, o, nb, fw)
        assert r["dq_flips_outside_ties"] == 0, (what, r)
        assert r["relu_flips_outside_ties"] == 0, (what, r)
        ref = ref64.ref_step(case, params, targets, nb, cur_max_override=got, relu_override=on_gpu, weights=w, **tails)
        if mixer == "qmix":
            ref64.assert_clear_of_kinks(ref, what)
        preconditions(ref, nb, lam, delta, what)
        ag, mg, fwo = o.gradients(nb, cur_max_override=got, relu_override=on_gpu)
        g_or = OrderedDict(list(ag.items()) + list(mg.items()))
        clip_grad_norm(g_or, o.cfg["grad_norm_clip"])
        e32 = ref64.block_errors(np.concatenate([v.ravel() for v in g_or.values()]), ref.clipped, case)
        errs = ref64.block_errors(g_gpu, ref.clipped, case)
        live = ref.mask > 0
        if lam:   # the lambda targets, one block of their own
            tg = learner.last_intermediate(5).cpu().numpy()
            assert tg.shape == ref.targets.shape, (what, tg.shape)
            e32["<lambda targets>"] = one_block(fwo["targets"], ref.targets, live)
            errs["<lambda targets>"] = one_block(tg, ref.targets, live)
        if per:   # the |td m| record of the priority write-back, likewise
            tda = learner.last_intermediate(6).cpu().numpy()
            assert tda.shape == ref.abs_mtd.shape, (what, tda.shape)
            live1 = live.any(2, keepdims=True)
            assert np.array_equal(tda[~live1], np.zeros_like(tda[~live1])), what
            o_tda = np.abs(fwo["td"] * fwo["mask"]).sum(2, keepdims=True)
            e32["<|td m|>"] = one_block(o_tda, ref.abs_mtd, live1)
            errs["<|td m|>"] = one_block(tda, ref.abs_mtd, live1)
        tol = ref64.tolerances(e32)
        ratio = ref64.ratios(errs, e32)
        worst = max(ratio, key=ratio.get)
        norm_err = abs(st["grad_norm"] - ref.norm) / ref.norm
        stat_err = {s_: abs(st[s_] - ref.stats[s_]) for s_ in P.STATS}
        print("{}: worst ratio {:.2f} at {} (err {:.3g}, e32 {:.3g}, tol {:.3g}); grad_norm rel {:.3g}; stats {}; "
              "dq ties/flips {}/{}, relu ties/flips {}/{}".format(
                  what, ratio[worst], worst, errs[worst], e32[worst], tol[worst], norm_err,
                  {s_: "{:.2g}".format(v) for s_, v in stat_err.items()}, r["dq_ties"], r["dq_flips"],
                  r["relu_ties"], r["relu_flips"]))
        rec.append(dict(step=k, plan=plan, decisions=r, grad_norm=st["grad_norm"], ref_grad_norm=ref.norm,
                        worst_block=worst, worst_ratio=ratio[worst], weights=None if w is None else w.tolist(),
                        huber_delta=delta, stats={s_: (st[s_], ref.stats[s_]) for s_ in P.STATS},
                        kinks=ref64.kink_minima(ref) if mixer == "qmix" else None,
                        blocks={b: dict(err=errs[b], e32=e32[b], tol=tol[b], ratio=ratio[b]) for b in errs}))
        bad += [(k, b, e, t) for b, (e, t) in ref64.failures(errs, tol).items()]
        assert norm_err <= 1e-5, (what, st["grad_norm"], ref.norm)
        for s_ in P.STATS:
            assert stat_err[s_] <= 1e-5 * abs(ref.stats[s_]) + 1e-6, (what, s_, st[s_], ref.stats[s_])
    P.write_record("tail64", row, rec)
    assert not bad, (row, bad)
