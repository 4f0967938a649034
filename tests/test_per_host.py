"""CPU checks of the prioritized-replay test infrastructure (tests/per_oracle.py) and of the C boundary the feature
adds (include/mq_learner.h: mq_per_sample, mq_set_per). The kernels themselves are checked in tests/test_gpu_per.py.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle.qlearner_np import F32, OracleQLearner
from pymarl_amd import _lib
from tests.golden_utils import Case
from tests.per_oracle import (PEROracleQLearner, chain_len, exact_fixture, interval_violations, per_sample,
                              priority_update)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = [(N, B) for N in (1, 7, 64, 1025, 5000) for B in (1, 4, 32)]


@pytest.mark.parametrize("N,B", GRID)
def test_exact_fixtures_give_the_same_ids_in_float32_and_float64(N, B):
    """The exactness condition is met by the fixture alone: every prefix sum, total / B and tau is the same number in
    both precisions, so the float32 sampler draws the float64 sampler's ids whatever the order of its scan."""
    prio, u = exact_fixture(N, B, seed=100 * N + B)
    i64, w64, s64 = per_sample(prio, N, u, 1.0, 1.0, np.float64)
    i32, w32, s32 = per_sample(prio, N, u, 1.0, 1.0, np.float32)
    assert np.array_equal(s32["cum"].astype(np.float64), s64["cum"])
    assert np.array_equal(s32["tau"].astype(np.float64), s64["tau"])
    assert np.array_equal(i32, i64)
    assert i64.min() >= 0 and i64.max() < N
    assert np.abs(w32 - w64).max() <= 1e-6 and w64.max() == 1.0
    assert not interval_violations(i64, prio, N, u, 1.0, 0)
    # a reversed (pairwise-free) scan order gives the same prefix sums too: the sums are exact
    rev = np.cumsum(prio[:N][::-1].astype(np.float32), dtype=np.float32)[-1]
    assert float(rev) == float(s64["total"])


def test_boundary_fixture_draws_the_next_episode():
    prio, u = exact_fixture(64, 4, seed=7, boundary=True)
    ids, _, s = per_sample(prio, 64, u, 1.0, 0.0, np.float64)
    hit = np.nonzero(s["cum"] == s["tau"][0])[0]
    assert len(hit) == 1 and ids[0] == hit[0] + 1
    i32, _, _ = per_sample(prio, 64, u, 1.0, 0.0, np.float32)
    assert np.array_equal(i32, ids)


def test_stale_slots_are_never_drawn_and_beta_zero_is_one():
    prio, u = exact_fixture(7, 32, seed=3, n_slots=16, stale=1e6)
    ids, w, _ = per_sample(prio, 7, u, 1.0, 0.0, np.float32)
    assert ids.max() < 7 and np.array_equal(w, np.ones(32, np.float32))


def test_chain_length_formula():
    assert chain_len(1) == chain_len(64) == chain_len(1024) == 12
    assert chain_len(1025) == 14 and chain_len(5000) == 20 and chain_len(32768) == 74
    text = open(os.path.join(ROOT, "pymarl_amd", "csrc", "per_kernels.hpp")).read()
    assert "constexpr int PER_THREADS = 1024;" in text and "constexpr int PER_SCAN_DEPTH = 10;" in text
    assert "return 2 * per_chunk(n) + PER_SCAN_DEPTH;" in text


def test_priority_update_restatement():
    tda = np.array([[0.5, 0.25, 0.0], [1.0, 2.0, 4.0], [0.0, 0.0, 0.0]], F32)
    mask = np.array([[1, 1, 0], [1, 1, 1], [0, 0, 0]], F32)
    p = priority_update(tda, mask, 1e-6)
    assert np.array_equal(p, (np.array([0.375, 7.0 / 3.0, 0.0], F32) + F32(1e-6)).astype(F32))
    p3 = priority_update(tda, mask, 1e-6, n_agents_div=3)
    assert np.array_equal(p3[:1], (F32(0.75) / F32(6.0) + F32(1e-6)).astype(F32).reshape(1))


def flat(grads):
    return np.concatenate([v.ravel() for v in grads.values()])


def all_grads(o, nb):
    ag, mg, fw = o.gradients(nb)
    return flat(dict(list(ag.items()) + list(mg.items()))), fw


@pytest.mark.parametrize("name", ["tiny_qmix", "tiny_vdn", "tiny_iql"])
def test_unit_weights_equal_the_parent_oracle_bitwise(name):
    case = Case(name)
    nb, _ = case.batch(0)
    o = OracleQLearner(case.agent_params, case.mixer_params, case.cfg())
    po = PEROracleQLearner(case.agent_params, case.mixer_params, case.cfg())
    po.weights = np.ones(case.B, F32)
    g0, fw0 = all_grads(o, nb)
    g1, fw1 = all_grads(po, nb)
    assert fw0["loss"] == fw1["loss"]
    assert np.array_equal(g0, g1)
    st0, st1 = o.train(nb, 0, 0), po.train(nb, 0, 0)
    assert st0 == st1
    assert np.array_equal(o.flat("params"), po.flat("params")) and np.array_equal(o.flat("sq"), po.flat("sq"))


@pytest.mark.parametrize("huber", [0.0, 1.0])
@pytest.mark.parametrize("name", ["tiny_qmix", "tiny_vdn", "tiny_iql"])
def test_weighted_gradient_is_the_weighted_sum_of_episode_gradients(name, huber):
    """loss = sum_b w_b S_b / msum with S_b = msum_b L_b, L_b the parent's loss of episode b alone, so the gradient is
    sum_b w_b (msum_b / msum) g_b."""
    case = Case(name)
    nb, _ = case.batch(0)
    cfg = dict(case.cfg(), huber_delta=huber)
    w = np.array([1.0, 0.3, 0.05, 0.6], F32)[:case.B]
    po = PEROracleQLearner(case.agent_params, case.mixer_params, cfg)
    po.weights = w
    g, fw = all_grads(po, nb)
    msum = float(fw["mask_sum"])
    want = np.zeros(g.shape, np.float64)
    loss = 0.0
    for b in range(case.B):
        one = {k: v[b:b + 1] for k, v in nb.items()}
        gb, fwb = all_grads(OracleQLearner(case.agent_params, case.mixer_params, cfg), one)
        want += float(w[b]) * (float(fwb["mask_sum"]) / msum) * gb.astype(np.float64)
        loss += float(w[b]) * (float(fwb["mask_sum"]) / msum) * fwb["loss"]
    err = np.abs(g - want).max() / np.abs(want).max()
    print("weighted gradient", name, huber, "rel err", err, "loss", fw["loss"], loss)
    assert err < 1e-5
    assert abs(fw["loss"] - loss) <= 1e-5 * abs(loss)


def test_new_exports_are_declared_bound_and_validated():
    text = open(os.path.join(ROOT, "include", "mq_learner.h")).read()
    for name in ("mq_per_sample", "mq_set_per"):
        assert re.search(r"^int {}\(".format(name), text, flags=re.M), name
        assert name in _lib.EXPORTS
    assert "int32_t per;" in text and _lib.MQPlan._fields_[-1][0] == "per"
    assert re.search(r"MQ_PER_MAX_LIVE = (\d+)", text).group(1) == str(_lib.PER_MAX_LIVE)
    lib = _lib.load()
    # argument checks come before any HIP call: they run without a GPU (the pointers are never dereferenced)
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    bad = [dict(alpha=-0.1), dict(alpha=float("nan")), dict(beta=-0.1), dict(beta=1.5), dict(n_live=0),
           dict(n_live=_lib.PER_MAX_LIVE + 1), dict(batch=0)]
    for over in bad:
        a = dict(n_live=4, batch=2, alpha=0.6, beta=0.4)
        a.update(over)
        rc = lib.mq_per_sample(p, a["n_live"], p, a["batch"], a["alpha"], a["beta"], p, p, None)
        assert rc == 1, over
        with pytest.raises(_lib.MQError):
            _lib.check(rc)
    assert lib.mq_set_per(None, None) == 1
