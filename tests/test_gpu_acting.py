"""The acting path and the standalone module forwards on the GPU against tests/act_ref64.py (DESIGN.md "Parity").

* a. RNNAgent.forward / mq_agent_forward: five shapes, a 20-call chain, and through ctypes the target parameters
  (which = 1), aliased hidden buffers and rows = 0.
* b. BasicMAC.forward / mq_mac_forward: the four obs_last_action x obs_agent_id combinations stepped over every slot
  of ragged episodes (padded steps included), then the same rows through the dense, inline-id, device-id and
  host-resident routes, bitwise; the two refusals of ids outside the storage.
* c. mq_greedy_actions / greedy_actions / EpsilonGreedyActionSelector: exact against the reference's masked max.
* d. mc_policy: the pi_logits post-processing in its four modes.
* e. One-layer QMixer.forward / mq_qmix_forward on six shapes, the one past 64 KB of LDS included.

Values are judged per output (per step of a chain) by err <= 16 * max(e32, 2e-7 * scale) with e32 the error of torch's
own modules in float32 on the same inputs; err / max(e32, 2e-7 * scale) of every row goes to
$MQ_PARITY_DIR/parity_act64_<row>.json. Actions compare exactly.
"""
import copy
import ctypes
from types import SimpleNamespace as SN

import numpy as np
import pytest
import torch as th

from tests import act_ref64 as R
from tests import test_gpu_parity as P

pytestmark = pytest.mark.gpu

MQ_OK, MQ_ERR_ARG, MQ_ERR_STATE = 0, 1, 3


def lib_():
    from pymarl_amd import _lib
    return _lib, _lib.load()


def judge(rec, bad, name, got, ref, c32):
    """One output against its float64 reference: recorded, printed, and listed in `bad` when over the bound."""
    got = got.detach().cpu().numpy() if th.is_tensor(got) else got
    ref = ref.detach().numpy() if th.is_tensor(ref) else ref
    c32 = c32.detach().numpy() if th.is_tensor(c32) else c32
    r, err, e32, scale = R.ratio(got, ref, c32)
    rec[name] = dict(ratio=r, err=err, e32=e32, scale=scale)
    print("{}: ratio {:.3g} (err {:.3g}, e32 {:.3g}, max|ref| {:.3g})".format(name, r, err, e32, scale))
    if not R.passes(r):
        bad.append((name, r, err, e32, scale))


def finish(row, rec, bad):
    worst = max(rec, key=lambda k: rec[k]["ratio"])
    P.write_record("act64", row, dict(worst=worst, worst_ratio=rec[worst]["ratio"], outputs=rec))
    assert not bad, (row, bad)


def sd64(mod):
    return R.named64({k: v.detach().numpy() for k, v in mod.state_dict().items()})


# ------------------------------------------------------------------------------------------------------ a. the agent
def make_agent(mod, I, A):
    from pymarl_amd.modules.agents.rnn_agent import RNNAgent
    agent = RNNAgent(I, SN(rnn_hidden_dim=R.H, n_actions=A, n_agents=1, obs_last_action=False,
                           obs_agent_id=False)).cuda()
    agent.load_state_dict(mod.state_dict())
    return agent


@pytest.mark.parametrize("I,A,rows", R.AGENT_SHAPES)
def test_agent_forward(I, A, rows):
    mod, x, h = R.agent_case(I, A, rows)
    agent = make_agent(mod, I, A)
    q, h1 = agent(x.cuda(), h.cuda())
    assert q.shape == (rows, A) and h1.shape == (rows, R.H)
    q64, h64, _ = R.agent_step(sd64(mod), x.double(), h.double())
    with th.no_grad():
        q32, h32 = mod(x, h)
    rec, bad = {}, []
    judge(rec, bad, "q", q, q64, q32)
    judge(rec, bad, "h_out", h1, h64, h32)
    finish("agent_I{}_A{}_r{}".format(I, A, rows), rec, bad)


def test_agent_chain():
    I, A, rows = R.CHAIN_SHAPE
    mod, _, h = R.agent_case(I, A, rows)
    xs = R.chain_inputs(I, rows, R.CHAIN_STEPS)
    agent = make_agent(mod, I, A)
    ref = R.agent_chain(sd64(mod), [x.double() for x in xs], h.double())
    hg, h32 = h.cuda(), h
    rec, bad = {}, []
    for t, x in enumerate(xs):
        q, hg = agent(x.cuda(), hg)
        with th.no_grad():
            q32, h32 = mod(x, h32)
        judge(rec, bad, "q[{}]".format(t), q, ref[t][0], q32)
        judge(rec, bad, "h_out[{}]".format(t), hg, ref[t][1], h32)
    finish("agent_chain", rec, bad)


def test_agent_forward_ctypes_target_alias_and_empty():
    from pymarl_amd.learners.q_learner import make_config
    _lib, lib = lib_()
    I, A, rows = R.CHAIN_SHAPE
    mod, x, h = R.agent_case(I, A, rows)
    other, _, _ = R.agent_case(I, A, rows, seed=1)
    on, tg = make_agent(mod, I, A), make_agent(other, I, A)
    hd = _lib.Handle(make_config(on.args, mixer=_lib.MIXER_NONE, input_dim=I))
    _lib.check(lib.mq_bind(hd.h, _lib.ptr(on._flat), _lib.ptr(tg._flat), None, None, None, None))
    xg, hg, s = x.cuda(), h.cuda(), _lib.stream_ptr()

    def run(which, h_in, h_out, n=rows, handle=hd):
        q = th.full((rows, A), -7.0, device="cuda")
        rc = lib.mq_agent_forward(handle.h, _lib.ptr(xg), n, _lib.ptr(h_in), _lib.ptr(h_out), _lib.ptr(q), which, s)
        th.cuda.synchronize()
        return rc, q

    # which = 1 reads the target parameters: the module built from them, and not the online ones
    q_on, h_on = on(xg, hg)
    q_tg, h_tg = tg(xg, hg)
    ho = th.empty_like(hg)
    rc, q1 = run(1, hg, ho)
    assert rc == MQ_OK and th.equal(q1, q_tg) and th.equal(ho, h_tg) and not th.equal(q1, q_on)
    q64, h64, _ = R.agent_step(sd64(other), x.double(), h.double())
    with th.no_grad():
        q32, h32 = other(x, h)
    rec, bad = {}, []
    judge(rec, bad, "q", q1, q64, q32)
    judge(rec, bad, "h_out", ho, h64, h32)
    rc, q0 = run(0, hg, ho)
    assert rc == MQ_OK and th.equal(q0, q_on) and th.equal(ho, h_on)
    # an inference-only handle has no target
    rc, q = run(1, hg, ho, handle=on.handle())
    assert rc == MQ_ERR_STATE and "target parameters not bound" in lib.mq_last_error().decode()
    assert (q == -7.0).all()
    # h_in == h_out
    hh = hg.clone()
    rc, qa = run(0, hh, hh)
    assert rc == MQ_OK and th.equal(qa, q_on) and th.equal(hh, h_on)
    # rows = 0: MQ_OK, nothing written
    ho.fill_(-3.0)
    rc, q = run(0, hg, ho, n=0)
    assert rc == MQ_OK and (q == -7.0).all() and (ho == -3.0).all()
    finish("agent_target", rec, bad)


# ------------------------------------------------------------------------------------------------------ b. the MAC
def build_mac(case, device="cuda", spare=1, **over):
    """The case's replay in a buffer with `spare` more episodes of room than it holds (zeros), and a BasicMAC with the
    case's agent parameters."""
    from pymarl_amd.components.episode_buffer import ReplayBuffer
    from pymarl_amd.components.transforms import OneHot
    from pymarl_amd.controllers import REGISTRY as mac_REGISTRY
    from tests.gpu_helpers import make_args, make_scheme
    args = make_args(case, **over)
    groups = {"agents": case.n}
    buf = ReplayBuffer(make_scheme(case), groups, case.n_episodes + spare, case.T + 1,
                       preprocess={"actions": ("actions_onehot", [OneHot(out_dim=case.A)])}, device=device)
    buf.load_arrays(case.data)
    mac = mac_REGISTRY["basic_mac"](buf.scheme, groups, args)
    mac.cuda()
    mac.agent.load_state_dict({k: th.from_numpy(v) for k, v in case.agent_params.items()})
    return buf, mac


def mac_steps(mac, batch, steps):
    """mac.forward for t = 0 .. steps - 1 from init_hidden: q (steps, bs, n, A), hidden (steps, bs, n, 64)."""
    mac.init_hidden(batch.batch_size)
    qs, hs = [], []
    for t in range(steps):
        q = mac.forward(batch, t)
        assert mac.hidden_states.shape == (batch.batch_size, mac.n_agents, R.H)
        qs.append(q.clone())
        hs.append(mac.hidden_states.clone())
    return th.stack(qs), th.stack(hs)


def mac_reference(case, flags, steps):
    q64, h64 = R.mac_chain(R.named64(case.agent_params), case.data, case.A, flags, steps)
    mod = R.ModAgent(case.I, case.A)
    mod.load_state_dict({k: th.from_numpy(v) for k, v in case.agent_params.items()})
    h = th.zeros(case.n_episodes * case.n, R.H)
    q32, h32 = [], []
    with th.no_grad():
        for t in range(steps):
            x = R.build_inputs(case.data["obs"], case.data["actions"], case.data["filled"], t, case.A, flags,
                               dtype=th.float32)
            q, h = mod(x, h)
            q32.append(q)
            h32.append(h)
    return q64, h64, th.stack(q32), th.stack(h32)


def judged_dense_chain(case, flags, buf, mac, row):
    """The dense device route, every step judged against the float64 chain; returns its q and hidden states."""
    N, n, steps = case.n_episodes, case.n, case.T + 1
    qd, hd = mac_steps(mac, buf[0:N], steps)
    q64, h64, q32, h32 = mac_reference(case, flags, steps)
    rec, bad = {}, []
    for t in range(steps):
        judge(rec, bad, "q[{}]".format(t), qd[t].reshape(N * n, -1), q64[t], q32[t])
        judge(rec, bad, "h[{}]".format(t), hd[t].reshape(N * n, -1), h64[t], h32[t])
    finish(row, rec, bad)
    return qd, hd


@pytest.mark.parametrize("flags", R.MAC_FLAGS, ids=lambda f: "la{}_id{}".format(int(f[0]), int(f[1])))
def test_mac_forward_flags_and_routes(flags):
    from pymarl_amd.components.episode_buffer import SampledBatch
    from pymarl_amd.learners.q_learner import replay_view
    tag = "la{}_id{}".format(int(flags[0]), int(flags[1]))
    case = R.mac_case(flags)
    N, steps = case.n_episodes, case.T + 1
    buf, mac = build_mac(case)
    assert mac.agent.input_dim == case.I == case.O + flags[0] * case.A + flags[1] * case.n
    qd, hd = judged_dense_chain(case, flags, buf, mac, "mac_" + tag)

    # inline host ids, permuted and duplicated
    ids = np.array([3, 0, 5, 5, 1, 2, 4, 0])
    sb = SampledBatch(buf, ids)
    assert replay_view(sb)[0].ep_ids_host and not replay_view(sb)[0].ep_ids
    qi, hi = mac_steps(mac, sb, steps)
    assert th.equal(qi, qd[:, ids]) and th.equal(hi, hd[:, ids])

    # a host-resident batch: the step's two slots go to the device as a dense batch
    cbuf, _ = build_mac(case, device="cpu")
    for t in (0, 1, steps - 1):
        if t == 0:
            mac.init_hidden(N)
        else:
            mac.hidden_states = hd[t - 1].clone()
        q = mac.forward(cbuf[0:N], t)
        assert q.device.type == "cpu" and mac.hidden_states.shape == (N, case.n, R.H)
        assert th.equal(q, qd[t].cpu()) and th.equal(mac.hidden_states, hd[t]), t

    # device ids: B = 257 > MQ_INLINE_IDS episodes of the two-agent sibling (R = 514 rows)
    case2 = R.mac_case(flags, n=2)
    buf2, mac2 = build_mac(case2)
    qd2, hd2 = judged_dense_chain(case2, flags, buf2, mac2, "mac_n2_" + tag)
    ids2 = np.random.Generator(np.random.PCG64(3)).integers(0, N, size=257)
    sb2 = SampledBatch(buf2, ids2)
    rep = replay_view(sb2)[0]
    assert rep.ep_ids and not rep.ep_ids_host and rep.batch_size * case2.n == 514
    q2, h2 = mac_steps(mac2, sb2, steps)
    assert th.equal(q2, qd2[:, ids2]) and th.equal(h2, hd2[:, ids2])


def test_mac_forward_refuses_ids_outside_the_storage():
    """mq_mac_forward validates the ids it copies into the kernel arguments, and a dense batch against n_episodes, as
    mq_train_step does. The replay tensors have one spare episode of room, so the refused reads would have stayed
    inside the allocation."""
    from pymarl_amd.components.episode_buffer import SampledBatch
    from pymarl_amd.learners.q_learner import replay_view
    _lib, lib = lib_()
    case = R.mac_case((True, True))
    N, n = case.n_episodes, case.n
    buf, mac = build_mac(case, spare=1)
    assert buf["obs"].shape[0] == N + 1
    rows = (N + 1) * n
    h_in = th.zeros(rows, R.H, device="cuda")
    h_out = th.full((rows, R.H), -3.0, device="cuda")
    q = th.full((rows, case.A), -7.0, device="cuda")
    hd = mac.agent.handle()

    def call(rep):
        rc = lib.mq_mac_forward(hd.h, rep, 1, _lib.ptr(h_in), _lib.ptr(h_out), _lib.ptr(q), 0, _lib.stream_ptr())
        th.cuda.synchronize()
        return rc, lib.mq_last_error().decode()

    rep, keep = replay_view(SampledBatch(buf, np.array([0, N - 1])))
    rep.n_episodes = N
    assert call(rep)[0] == MQ_OK and (q[:2 * n] != -7.0).all() and (q[2 * n:] == -7.0).all()
    q.fill_(-7.0)
    h_out.fill_(-3.0)
    host = np.array([0, N], np.int64)   # one past the end
    rep.ep_ids_host = host.ctypes.data
    rc, msg = call(rep)
    assert rc == MQ_ERR_ARG and "episode id {} outside [0, n_episodes)".format(N) in msg, (rc, msg)
    rep.ep_ids_host = None   # dense, one episode more than the storage is said to hold
    rep.batch_size = N + 1
    rc, msg = call(rep)
    assert rc == MQ_ERR_ARG and "batch_size exceeds n_episodes with no episode ids" in msg, (rc, msg)
    assert (q == -7.0).all() and (h_out == -3.0).all()   # nothing was launched
    rep.batch_size = N
    assert call(rep)[0] == MQ_OK and (q[:N * n] != -7.0).all()
    del keep


# ------------------------------------------------------------------------------------------------------ c. greedy
def gpu_greedy(q, avail):
    from pymarl_amd.components.action_selectors import greedy_actions
    return greedy_actions(th.as_tensor(q).cuda(), th.as_tensor(avail).cuda()).cpu().numpy()


@pytest.mark.parametrize("A", R.GREEDY_A)
@pytest.mark.parametrize("rows", R.GREEDY_ROWS)
def test_greedy_actions(rows, A):
    """Ties, empty rows, -inf at available actions, avail values 2 and -1, the last partial block."""
    q, avail = R.greedy_case(rows, A, nans=False)
    got = gpu_greedy(q, avail)
    assert got.dtype == np.int64 and got.shape == (rows,)
    assert np.array_equal(got, R.greedy(q, avail)), np.nonzero(got != R.greedy(q, avail))[0][:8]


@pytest.mark.parametrize("A", R.GREEDY_A)
@pytest.mark.parametrize("rows", R.GREEDY_ROWS)
def test_greedy_actions_nan(rows, A):
    """torch's max(dim): a NaN at an available action wins (first such index); at an unavailable one it is masked."""
    q, avail = R.greedy_case(rows, A, nans=True)
    got = gpu_greedy(q, avail)
    want = R.greedy(q, avail)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


def test_greedy_actions_hand_cases_and_ctypes():
    _lib, lib = lib_()
    nan, inf = float("nan"), float("inf")
    q = th.tensor([[1, nan, 5, 0], [3, 3, 1, 3], [5, 1, 1, 1], [-inf, -inf, 2, 2], [nan, 7, nan, 1], [1, 2, 3, 4]]).cuda()
    av = th.tensor([[1, 1, 1, 1], [0, 2, 1, -1], [0, 1, 1, 0], [1, 1, 0, 0], [0, 1, 1, 1], [0, 0, 0, 0]],
                   dtype=th.int32).cuda()
    out = th.full((8,), -5, dtype=th.int64, device="cuda")
    assert lib.mq_greedy_actions(_lib.ptr(q), _lib.ptr(av), _lib.ptr(out), 6, 4, _lib.stream_ptr()) == MQ_OK
    assert out.tolist() == [1, 1, 1, 0, 2, 0, -5, -5]
    assert lib.mq_greedy_actions(_lib.ptr(q), _lib.ptr(av), _lib.ptr(out), 0, 4, _lib.stream_ptr()) == MQ_OK
    assert lib.mq_greedy_actions(_lib.ptr(q), _lib.ptr(av), _lib.ptr(out), 6, 0, _lib.stream_ptr()) == MQ_ERR_ARG


def test_greedy_actions_noncontiguous_3d():
    from pymarl_amd.components.action_selectors import greedy_actions
    B, n, A = 250, 4, 9
    q, avail = R.greedy_case(B * n, A)
    want = R.greedy(q, avail).reshape(B, n)
    q3 = th.as_tensor(q).reshape(B, n, A).permute(1, 0, 2).contiguous().cuda().permute(1, 0, 2)
    a3 = th.as_tensor(avail).reshape(B, n, A).permute(2, 0, 1).contiguous().cuda().permute(1, 2, 0)
    assert not q3.is_contiguous() and not a3.is_contiguous() and q3.shape == a3.shape == (B, n, A)
    got = greedy_actions(q3, a3)
    assert got.shape == (B, n) and np.array_equal(got.cpu().numpy(), want)


def selector(**over):
    from pymarl_amd.components.action_selectors import EpsilonGreedyActionSelector
    return EpsilonGreedyActionSelector(SN(**dict(dict(epsilon_start=1.0, epsilon_finish=0.05,
                                                      epsilon_anneal_time=50000), **over)))


def test_epsilon_greedy_selector():
    from torch.distributions import Categorical
    B, n, A = 64, 3, 9
    g = np.random.Generator(np.random.PCG64(5))
    q = th.as_tensor(g.integers(0, 4, size=(B, n, A)).astype(np.float32)).cuda()   # ties
    avail = th.as_tensor((g.random((B, n, A)) < 0.6).astype(np.int32))
    avail[..., 1] = 1
    avail = avail.cuda()
    ref = th.as_tensor(R.greedy(q.cpu().numpy(), avail.cpu().numpy())).cuda()
    sel = selector()
    # test mode: the greedy actions
    assert th.equal(sel.select_action(q, avail, 25000, test_mode=True), ref) and sel.epsilon == 0.0
    # the selector's formula restated around the reference greedy, under the same seed: same draws, same order
    th.manual_seed(11)
    got = sel.select_action(q, avail, 25000, test_mode=False)
    eps = sel.schedule.eval(25000)
    assert sel.epsilon == eps and 0.4 < eps < 0.6
    th.manual_seed(11)
    pick = (th.rand_like(q[:, :, 0]) < eps).long()
    rand = Categorical(avail.float()).sample().long()
    assert th.equal(got, pick * rand + (1 - pick) * ref)
    assert 0 < int(pick.sum()) < B * n and not th.equal(got, ref)
    # test mode draws too: the RNG stream moves as in the reference
    th.manual_seed(11)
    sel.select_action(q, avail, 25000, test_mode=True)
    after = th.rand(4, device="cuda")
    th.manual_seed(11)
    th.rand_like(q[:, :, 0])
    Categorical(avail.float()).sample()
    assert th.equal(after, th.rand(4, device="cuda"))
    # epsilon 1: every action random, every one available
    got = sel.select_action(q, avail, 0, test_mode=False)
    assert sel.epsilon == 1.0 and (th.gather(avail, 2, got.unsqueeze(2)) != 0).all()


# ------------------------------------------------------------------------------------------------------ d. pi_logits
def gpu_policy(lg, av, eps, mbs, test_mode):
    _lib, lib = lib_()
    x = th.as_tensor(lg).cuda().clone()
    a = th.as_tensor(av).cuda()
    rc = lib.mc_policy(_lib.ptr(x), _lib.ptr(a), x.shape[0], x.shape[1], eps, mbs, test_mode, _lib.stream_ptr())
    assert rc == MQ_OK, lib.mq_last_error()
    return x.cpu().numpy()


@pytest.mark.parametrize("test_mode", [0, 1])
@pytest.mark.parametrize("mbs", [0, 1])
@pytest.mark.parametrize("A", R.POLICY_A)
def test_mc_policy(A, mbs, test_mode):
    rec, bad = {}, []
    for rows in R.POLICY_ROWS:
        lg, av = R.policy_case(rows, A)
        for eps in R.POLICY_EPS:
            name = "r{}_eps{}".format(rows, eps)
            got = gpu_policy(lg, av, eps, mbs, test_mode)
            ref = R.policy(lg, av, eps, mbs, test_mode).numpy()
            c32 = R.policy_mod(lg, av, eps, mbs, test_mode, th.float32).numpy()
            judge(rec, bad, name, got, ref, c32)
            ones = np.abs(ref.sum(1) - 1.0) <= 1e-12   # the rows that are distributions in the reference
            assert ones.any() or rows == 1
            if ones.any():
                judge(rec, bad, name + "_rowsum", got[ones].astype(np.float64).sum(1), ref[ones].sum(1),
                      c32[ones].astype(np.float64).sum(1))
            if mbs and not test_mode:
                assert not got[av == 0].any(), name   # exactly zero
    finish("policy_A{}_mbs{}_tm{}".format(A, mbs, test_mode), rec, bad)


def test_mc_policy_refuses_65_actions():
    _lib, lib = lib_()
    x = th.zeros(4, 65, device="cuda")
    a = th.ones(4, 65, dtype=th.int32, device="cuda")
    assert lib.mc_policy(_lib.ptr(x), _lib.ptr(a), 4, 65, 0.1, 1, 0, _lib.stream_ptr()) == MQ_ERR_ARG
    th.cuda.synchronize()
    assert not x.any()
    assert lib.mc_policy(_lib.ptr(x), _lib.ptr(a), 4, 64, 0.1, 1, 0, _lib.stream_ptr()) == MQ_OK


def test_mac_forward_pi_logits_test_mode():
    flags = (True, True)
    case = R.mac_case(flags)
    N, n = case.n_episodes, case.n
    buf, mac = build_mac(case, agent_output_type="pi_logits")
    mac.action_selector.epsilon = 0.3   # test mode: no floor, so it must not matter
    q64, _, q32, _ = mac_reference(case, flags, 2)
    rec, bad = {}, []
    mac.init_hidden(N)
    for t in range(2):
        got = mac.forward(buf[0:N], t, test_mode=True)
        av = case.data["avail_actions"][:, t].reshape(N * n, -1)
        ref = R.policy(q64[t].numpy(), av, 0.3, 1, 1)
        c32 = R.policy_mod(q32[t].numpy(), av, 0.3, 1, 1, th.float32)
        assert got.shape == (N, n, case.A)
        judge(rec, bad, "pi[{}]".format(t), got.reshape(N * n, -1), ref, c32)
    finish("policy_mac_test_mode", rec, bad)


# ------------------------------------------------------------------------------------------------------ e. the mixer
@pytest.mark.parametrize("n,S,E,rows", R.MIXER_SHAPES)
def test_qmixer_forward(n, S, E, rows):
    from pymarl_amd.modules.mixers.qmix import QMixer
    mod, qs, st = R.mixer_case(n, S, E, rows)
    m = QMixer(SN(n_agents=n, state_shape=S, mixing_embed_dim=E)).cuda()
    m.load_state_dict(mod.state_dict())
    y64, _ = R.qmix(sd64(mod), qs.double(), st.double())
    with th.no_grad():
        y32 = mod(qs.unsqueeze(1), st.unsqueeze(1)).reshape(-1)
    got = m(qs.cuda().unsqueeze(1), st.cuda().unsqueeze(1))
    th.cuda.synchronize()
    assert got.shape == (rows, 1, 1)
    rec, bad = {}, []
    judge(rec, bad, "q_tot", got.reshape(-1), y64, y32)
    finish("qmix_n{}_S{}_E{}_r{}".format(n, S, E, rows), rec, bad)


def test_qmix_forward_refuses_a_state_past_the_lds():
    _lib, lib = lib_()
    S = 10240   # 4 rows * (S + 4) floats = 163904 B > 160 KB
    w = th.zeros(4 * S + 16, device="cuda")
    qs, st = th.zeros(2, 1, device="cuda"), th.zeros(2, S, device="cuda")
    out = th.full((2,), -7.0, device="cuda")
    rc = lib.mq_qmix_forward(_lib.ptr(w), 1, S, 1, _lib.ptr(qs), _lib.ptr(st), _lib.ptr(out), 2, _lib.stream_ptr())
    th.cuda.synchronize()
    assert rc == MQ_ERR_ARG and (out == -7.0).all(), lib.mq_last_error()
