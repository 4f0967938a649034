"""tests/act_ref64.py pinned on the CPU: every float64 reference of the acting path against torch's own float64
nn.Linear / nn.GRUCell / softmax / elu / max(dim), assembled separately (act_ref64.ModAgent / ModMixer / policy_mod,
ref64.unroll, the reference's masked max), so that a typo in a reference cannot become the standard; and the inputs
of tests/test_gpu_acting.py hold what its rows are there for."""
import copy

import numpy as np
import pytest
import torch as th

from tests import act_ref64 as R
from tests import ref64

F64 = th.float64
PIN = 1e-12   # float64 against float64, another operation order: relative to the output's max


def close(a, b, tol=PIN):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


# ------------------------------------------------------------------------------------------------------ the agent
@pytest.mark.parametrize("I,A,rows", R.AGENT_SHAPES)
def test_agent_step_is_torchs_modules(I, A, rows):
    mod, x, h = R.agent_case(I, A, rows)
    m64 = copy.deepcopy(mod).double()
    p = R.named64({k: v.detach().numpy() for k, v in mod.state_dict().items()})
    q, h1, aux = R.agent_step(p, x.double(), h.double())
    with th.no_grad():
        qm, hm = m64(x.double(), h.double())
    assert q.shape == (rows, A) and h1.shape == (rows, R.H)
    assert close(q, qm) and close(h1, hm)
    if rows > 1:
        assert not x[-1].any() and not h[0].any() and x[0].any() and h[-1].any()


def test_agent_inputs_have_both_relu_signs_and_saturated_gates():
    for I, A, rows in R.AGENT_SHAPES[1:]:
        mod, x, h = R.agent_case(I, A, rows)
        p = R.named64({k: v.detach().numpy() for k, v in mod.state_dict().items()})
        _, _, aux = R.agent_step(p, x.double(), h.double())
        assert (aux.pre > 0).any() and (aux.pre < 0).any(), (I, A, rows)
        sat = min(float(th.minimum(g, 1 - g).min()) for g in (aux.r, aux.z))
        assert sat < 1e-3, (I, A, rows, sat)   # a gate within 1e-3 of 0 or 1


def test_agent_chain_is_the_modules_chain():
    I, A, rows = R.CHAIN_SHAPE
    mod, _, h = R.agent_case(I, A, rows)
    xs = R.chain_inputs(I, rows, R.CHAIN_STEPS)
    p = R.named64({k: v.detach().numpy() for k, v in mod.state_dict().items()})
    out = R.agent_chain(p, [x.double() for x in xs], h.double())
    m64, hm = copy.deepcopy(mod).double(), h.double()
    assert len(out) == R.CHAIN_STEPS
    with th.no_grad():
        for x, (q, hh) in zip(xs, out):
            qm, hm = m64(x.double(), hm)
            assert close(q, qm) and close(hh, hm)


# ------------------------------------------------------------------------------------------------------ the MAC case
def test_mac_case_has_the_episodes_it_is_there_for():
    case = R.mac_case((True, True))
    lens = case.data["filled"].sum(1).reshape(-1) - 1
    assert case.data["filled"].shape == (6, R.MAC["T"] + 1, 1)
    assert 1 in lens and R.MAC["T"] in lens, lens          # one of length 1 (slots 2.. unfilled), one full
    assert len(set(lens.tolist())) >= 3, lens
    assert [R.mac_case(f).I for f in R.MAC_FLAGS] == [15, 12, 10, 7]
    e = int(np.argmax(lens == 1))   # an unvalidated slot would read action 0 there: the one-hot must still be zero
    x = R.build_inputs(case.data["obs"], case.data["actions"], case.data["filled"], 3, case.A, (True, False))
    assert not x.reshape(6, case.n, -1)[e, :, case.O:].any()
    assert x.reshape(6, case.n, -1)[int(np.argmax(lens == R.MAC["T"])), :, case.O:].sum() == case.n


@pytest.mark.parametrize("flags", R.MAC_FLAGS)
@pytest.mark.parametrize("n", [3, 2])
def test_mac_chain_is_ref64_unroll_and_the_reference_builder(flags, n):
    """build_inputs (raw actions / filled) against the reference's recipe on the preprocessed actions_onehot, the chain
    against ref64.unroll and against torch's modules."""
    case = R.mac_case(flags, n)
    d, Tp = case.data, R.MAC["T"] + 1
    for t in range(Tp):
        parts = [th.as_tensor(d["obs"][:, t], dtype=F64)]
        if flags[0]:
            oh = th.as_tensor(d["actions_onehot"][:, t - 1], dtype=F64) if t else th.zeros(6, n, case.A, dtype=F64)
            parts.append(oh)
        if flags[1]:
            parts.append(th.eye(n, dtype=F64).unsqueeze(0).expand(6, -1, -1))
        want = th.cat([p.reshape(6 * n, -1) for p in parts], dim=1)
        got = R.build_inputs(d["obs"], d["actions"], d["filled"], t, case.A, flags)
        assert got.shape == (6 * n, case.I) and th.equal(got, want), (flags, t)
    p = R.named64(case.agent_params)
    q, h = R.mac_chain(p, d, case.A, flags, Tp)
    assert q.shape == (Tp, 6 * n, case.A) and h.shape == (Tp, 6 * n, R.H)
    Q, pre, _ = ref64.unroll(p, th.as_tensor(d["obs"], dtype=F64), th.as_tensor(d["actions_onehot"], dtype=F64), flags,
                              F64)
    assert close(q, Q.permute(1, 0, 2, 3).reshape(Tp, 6 * n, case.A))
    assert (pre > 0).any() and (pre < 0).any()
    mod = R.ModAgent(case.I, case.A).double()
    mod.load_state_dict({k: th.as_tensor(v, dtype=F64) for k, v in case.agent_params.items()})
    hm = th.zeros(6 * n, R.H, dtype=F64)
    with th.no_grad():
        for t in range(Tp):
            qm, hm = mod(R.build_inputs(d["obs"], d["actions"], d["filled"], t, case.A, flags), hm)
            assert close(q[t], qm) and close(h[t], hm)


# ------------------------------------------------------------------------------------------------------ greedy
def torch_greedy(q, avail):
    """The reference selector's greedy branch on (rows, A)."""
    m = th.as_tensor(q).clone().unsqueeze(0)
    m[th.as_tensor(avail).unsqueeze(0) == 0.0] = -float("inf")
    return m.max(dim=2)[1][0].numpy()


@pytest.mark.parametrize("A", R.GREEDY_A)
@pytest.mark.parametrize("rows", R.GREEDY_ROWS)
def test_greedy_is_torchs_masked_max(rows, A):
    q, avail = R.greedy_case(rows, A)
    got = R.greedy(q, avail)
    assert got.dtype == np.int64 and np.array_equal(got, torch_greedy(q, avail))
    assert np.array_equal(R.greedy(q.astype(np.float64), avail), got)


def test_greedy_hand_cases():
    nan, inf = float("nan"), float("inf")
    q = np.array([[1, nan, 5, 0], [3, 3, 1, 3], [5, 1, 1, 1], [-inf, -inf, 2, 2], [nan, 7, nan, 1], [1, 2, 3, 4]],
                 np.float32)
    av = np.array([[1, 1, 1, 1], [0, 2, 1, -1], [0, 1, 1, 0], [1, 1, 0, 0], [0, 1, 1, 1], [0, 0, 0, 0]], np.int32)
    want = [1, 1, 1, 0, 2, 0]
    assert R.greedy(q, av).tolist() == want == torch_greedy(q, av).tolist()


def test_greedy_inputs_hold_ties_empty_rows_and_nans():
    for rows in R.GREEDY_ROWS[1:]:
        for A in R.GREEDY_A[1:]:
            q, avail = R.greedy_case(rows, A)
            m = np.where(avail == 0, -np.inf, q)
            top = np.nanmax(np.where(np.isnan(m), -np.inf, m), axis=1, keepdims=True)
            ties = ((m == top).sum(1) > 1) & np.isfinite(top[:, 0])
            assert ties.any(), (rows, A)                                  # an exact tie at a finite maximum
            assert (avail == 0).all(1).any(), (rows, A)                   # an all-unavailable row
            assert (np.isneginf(q) & (avail != 0)).any(), (rows, A)       # -inf at an available action
            assert (avail == 2).any() and (avail == -1).any(), (rows, A)
            assert (np.isnan(q[:, 1:]) & (avail[:, 1:] != 0)).any(), (rows, A)   # NaN, available, not first
            assert (np.isnan(q) & (avail == 0)).any(), (rows, A)                 # NaN, unavailable
            plain = np.nan_to_num(m, nan=-np.inf).argmax(1)
            assert (plain != R.greedy(q, avail)).any(), (rows, A)   # a loop that skips NaN answers differently
    q, avail = R.greedy_case(1000, 9, nans=False)
    assert not np.isnan(q).any()


# ------------------------------------------------------------------------------------------------------ pi_logits
@pytest.mark.parametrize("mbs", [0, 1])
@pytest.mark.parametrize("test_mode", [0, 1])
def test_policy_is_torchs_softmax(mbs, test_mode):
    for A in R.POLICY_A:
        for rows in R.POLICY_ROWS:
            lg, av = R.policy_case(rows, A)
            for eps in R.POLICY_EPS:
                got = R.policy(lg, av, eps, mbs, test_mode).numpy()
                want = R.policy_mod(lg, av, eps, mbs, test_mode, F64).numpy()
                assert np.array_equal(np.isnan(got), np.isnan(want)), (A, rows, eps)
                ok = np.isfinite(want)
                assert np.array_equal(got[~ok & ~np.isnan(want)], want[~ok & ~np.isnan(want)])
                assert np.abs(got[ok] - want[ok]).max() <= PIN, (A, rows, eps)
                if mbs and not test_mode:
                    assert not got[av == 0].any()


def test_policy_inputs_hold_their_edges():
    for A in R.POLICY_A[1:]:
        for rows in R.POLICY_ROWS:
            lg, av = R.policy_case(rows, A)
            assert av[0].sum() == 1
            assert rows == 1 or av[-1].sum() == 0
            assert set(np.unique(av).tolist()) <= {0, 1}
    lg, av = R.policy_case(1023, 64)
    assert (lg == 80.0).any() and (lg == -80.0).any()
    assert ((lg == 80.0) & (av == 0)).any() and ((lg == 80.0) & (av == 1)).any()
    # the all-unavailable row under masking: zeros with the floor on, uniform in test mode
    assert not R.policy(lg, av, 0.3, 1, 0)[-1].any()
    assert close(R.policy(lg, av, 0.3, 1, 1)[-1], np.full(64, 1 / 64))


# ------------------------------------------------------------------------------------------------------ the mixer
@pytest.mark.parametrize("n,S,E,rows", R.MIXER_SHAPES)
def test_qmix_is_torchs_modules(n, S, E, rows):
    mod, qs, st = R.mixer_case(n, S, E, rows)
    mp = R.named64({k: v.detach().numpy() for k, v in mod.state_dict().items()})
    y, pre = R.qmix(mp, qs.double(), st.double())
    with th.no_grad():
        want = copy.deepcopy(mod).double()(qs.double().unsqueeze(1), st.double().unsqueeze(1))
    assert y.shape == (rows,) and pre.shape == (rows, E)
    assert close(y, want.reshape(-1))
    assert (qs > 0).any() or n * rows == 1
    if rows * E > 1:
        assert (pre > 0).any() and (pre < 0).any(), (n, S, E, rows)   # both branches of the elu


def test_ref64_qmix_keeps_its_learner_shape():
    """ref64.qmix now reads the embed dim from the parameters: the learner cases' E = 32 is unchanged."""
    mod, qs, st = R.mixer_case(3, 48, ref64.E, 8)
    mp = R.named64({k: v.detach().numpy() for k, v in mod.state_dict().items()})
    y, hw1, hwf, hv, _ = ref64.qmix(mp, qs.double().reshape(2, 4, 3), st.double().reshape(2, 4, 48), 3)
    assert y.shape == (2, 4, 1) and hw1.shape == (8, 3 * ref64.E) and hwf.shape == hv.shape == (8, ref64.E)


# ------------------------------------------------------------------------------------------------------ the gate
def test_ratio_is_the_stated_rule():
    ref = np.array([1.0, -4.0, 0.5])
    r, err, e32, scale = R.ratio(ref + [0, 8e-7, 0], ref, ref + [1e-7, 0, 0])
    assert scale == 4.0 and abs(err - 8e-7) < 1e-15 and abs(e32 - 1e-7) < 1e-15
    assert abs(r - 8e-7 / (2e-7 * 4.0)) < 1e-6 and R.passes(r)            # the floor: 2e-7 * scale
    r = R.ratio(ref + [0, 2e-5, 0], ref, ref + [1e-6, 0, 0])[0]
    assert abs(r - 20.0) < 1e-6 and not R.passes(r)                         # 16 * e32 is the bound
    with pytest.raises(AssertionError):
        R.ratio(np.array([np.nan, 1.0]), np.array([0.0, 1.0]), np.array([0.0, 1.0]))
