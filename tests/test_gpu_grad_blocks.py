"""Every gradient tensor of train() judged on its own scale against the float64 autograd reference (tests/ref64.py).

The teacher-forced tests gate the gradient with one number, rel(flat) < 1e-4 on the max over all tensors, which is
always fc2.bias's: a tensor a hundred to a thousand times smaller (the hypernet's, V's, fc1's one-hot columns) may
be wrong by per cent under it. Here every block of tests/ref64.grad_blocks (each tensor, fc1.weight by input kind,
the GRU's tensors by gate, hyper_w_1 by agent) is judged on its own max against ref64, with the tolerance

    tol(block) = min(1e-5, 16 * max(e32(block), 2e-7))

where e32 is the fp32 numpy oracle's own error against ref64 on that block, from the same state with the same
decisions (ref64 module docstring). Two train() steps per row: step 0 from the case's weights, step 1 from the GPU's
own parameters after step 0. Before each comparison: the GPU's double-Q argmax and fc1 relu decisions differ from the
oracle's on near-ties only (and are then followed), and the mixer's abs / relu pre-activations of live rows keep
clear of 0 (they cannot be read back). After it: the plan the row is there for, and grad_norm to 1e-5 relative.

Each row is the smallest ragged shape (episodes from one step on) at which its path still has the thing that can go
wrong; the wide rows are VDN because 2e5 hypernet outputs cannot all keep clear of the kinks. The measured
err / max(e32, 2e-7) of every block goes to $MQ_PARITY_DIR/parity_grad64_<row>.json.
"""
from collections import OrderedDict

import numpy as np
import pytest

from tests import ref64
from tests import test_gpu_parity as P
from tests.gpu_helpers import build, flat_grads, flat_params, flat_targets, set_switch

pytestmark = pytest.mark.gpu

BASE = dict(fused_fwd=2, fused_bwd=1, bwd_lean=1, hyper="ws", mix="fast16", tiles=0, rows=12)
# row id: (shape, mixer, MQ_PLAN switches, the plan items the row must report)
ROWS = OrderedDict([
    ("base", ("base", "qmix", {}, BASE)),
    ("base_classic", ("base", "qmix", {"bwd_lean": 0}, dict(BASE, bwd_lean=0))),
    ("base_onerow", ("base", "qmix", {"fwd_pair": 0}, dict(BASE, fused_fwd=1, bwd_lean=0))),
    ("base_hyp_after", ("base", "qmix", {"fwd_pair": 0, "hyp_in_fwd": 0}, dict(BASE, fused_fwd=1, bwd_lean=0))),
    # beyond the hypernet after the forward: appended to the one-row forward's grid, and as the pair kernel's epilogue
    ("base_hyp_grid", ("base", "qmix", {"hyp_in_fwd": 1}, dict(BASE, fused_fwd=1, bwd_lean=0))),
    ("base_hyp_epi", ("base", "qmix", {"pair_hyp_epi": True}, BASE)),
    ("base_dwh_grid",("base", "qmix", {"dwh_in_bwd": 1}, dict(BASE, dwh="bptt_grid"))),
    ("base_unfused", ("base", "qmix", {"unfused_fwd": True, "unfused_bwd": True},
                      dict(fused_fwd=0, fused_bwd=0, tiles=0, rw_fwd=1, rw_bwd=1, hyper="ws"))),
    ("base_tiles", ("base", "qmix", {"row_tiles": 1}, dict(tiles=1, fused_fwd=0, fused_bwd=0, rows=12))),
    # n = 3, A = 9 is a fast-mixer shape: mix_generic only replaces the staged (stream) mixer, so the plan stays fast16
    ("base_generic", ("base", "qmix", {"mix_generic": True}, BASE)),
    ("base_vdn", ("base", "vdn", {}, dict(BASE, hyper="none"))),
    ("base_iql", ("base", "none", {}, dict(BASE, hyper="none"))),
    ("lds", ("lds", "qmix", {}, dict(hyper="lds", fused_fwd=2, fused_bwd=1))),
    ("gemm", ("gemm", "qmix", {}, dict(hyper="gemm", fused_fwd=2, fused_bwd=1))),
    ("fast32", ("fast32", "qmix", {}, dict(fused_fwd=0, fused_bwd=0, tiles=0, mix="fast32"))),
    ("stream", ("stream", "qmix", {}, dict(mix="stream"))),
    ("generic", ("stream", "qmix", {"mix_generic": True}, dict(mix="generic"))),
    ("tiles_r21", ("tiles_r21", "qmix", {"row_tiles": 1}, dict(tiles=1, rows=21))),
    ("tiles_kq40", ("tiles_kq40", "qmix", {"row_tiles": 1}, dict(tiles=1))),   # gru_*_tile / split kernels <40>
    ("tiles_kq80", ("tiles_kq80", "qmix", {"row_tiles": 1}, dict(tiles=1))),   # <80>
    ("wide_tiles", ("wide", "vdn", {}, dict(tiles=1, rows=576, fused_fwd=0, fused_bwd=0))),
    ("wide_rw", ("wide", "vdn", {"row_tiles": 0}, dict(tiles=0, rows=576, rw_fwd=2, rw_bwd=2, fused_fwd=0,
                                                       fused_bwd=0))),
])


@pytest.fixture(scope="module")
def synth_cases():
    return {}


def oracle_clipped(o, nb, got, on_gpu):
    """The fp32 oracle's clipped gradient at its state, following the decisions `got` / `on_gpu`."""
    from oracle.qlearner_np import clip_grad_norm
    ag, mg, _ = o.gradients(nb, cur_max_override=got, relu_override=on_gpu)
    g = OrderedDict(list(ag.items()) + list(mg.items()))
    clip_grad_norm(g, o.cfg["grad_norm_clip"])
    return np.concatenate([v.ravel() for v in g.values()])


@pytest.mark.parametrize("row", list(ROWS))
def test_grad_blocks_vs_ref64(synth_cases, row, monkeypatch):
    from oracle.qlearner_np import OracleQLearner
    shape, mixer, switches, want = ROWS[row]
    if (shape, mixer) not in synth_cases:
        synth_cases[shape, mixer] = ref64.synth_case(shape, mixer)
    case = synth_cases[shape, mixer]
    for key, v in switches.items():   # read once, at handle creation
        set_switch(monkeypatch, key, v)
    args, buf, mac, learner, logger = build(case)
    o = OracleQLearner(case.agent_params, case.mixer_params, case.cfg())
    np.random.seed(case.sampler_seed)
    rec, bad = [], []
    for k in range(2):
        batch = buf.sample(case.B)
        batch = batch[:, :batch.max_t_filled()]
        nb, _ = case.batch(k)
        P.oracle_from_learner(o, case, learner)   # step 1: the GPU's own parameters and targets after step 0
        params, targets = flat_params(learner), flat_targets(learner)
        fw = o.forward(nb)
        learner.train(batch, 1000 * k, case.episodes[k])
        g_gpu = flat_grads(learner)
        plan = learner.last_plan()
        norm_gpu = learner.last_stats()["grad_norm"]
        assert np.isfinite(g_gpu).all(), (row, k)
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
        print("{} step {}: worst ratio {:.2f} at {} (err {:.3g}, e32 {:.3g}, tol {:.3g}); grad_norm rel {:.3g}; "
              "dq ties/flips {}/{}, relu ties/flips {}/{}".format(
                  row, k, ratio[worst], worst, errs[worst], e32[worst], tol[worst], norm_err, r["dq_ties"],
                  r["dq_flips"], r["relu_ties"], r["relu_flips"]))
        rec.append(dict(step=k, plan=plan, decisions=r, grad_norm=norm_gpu, ref_grad_norm=ref.norm,
                        worst_block=worst, worst_ratio=ratio[worst],
                        kinks=ref64.kink_minima(ref) if mixer == "qmix" else None,
                        blocks={b: dict(err=errs[b], e32=e32[b], tol=tol[b], ratio=ratio[b]) for b in errs}))
        bad += [(k, b, e, t) for b, (e, t) in ref64.failures(errs, tol).items()]
        for key, v in want.items():
            assert plan[key] == v, (row, key, plan)
        assert norm_err <= 1e-5, (row, k, norm_gpu, ref.norm)
    P.write_record("grad64", row, rec)
    assert not bad, (row, bad)
