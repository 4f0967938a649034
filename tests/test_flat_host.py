"""The learners' shared flat-buffer plumbing (pymarl_amd/modules/flat.py: link, load_state, written_by,
state_dict_own_steps) on two tiny nn.Linear modules, on the CPU."""
import pytest
import torch as th
from torch.optim import Adam, RMSprop

from pymarl_amd.modules.flat import link, load_state, pack, state_buffers, state_dict_own_steps, written_by

OPTS = {"rmsprop": lambda ps: RMSprop(ps, lr=0.01, alpha=0.99, eps=1e-5), "adam": lambda ps: Adam(ps, lr=0.01)}


def build(name, shared):
    """Two Linears packed into one flat buffer, their optimiser linked to flat grad / state buffers."""
    th.manual_seed(3)
    mods = [th.nn.Linear(3, 2), th.nn.Linear(2, 1)]
    flat, P = pack(mods)
    params = [p for m in mods for p in m.parameters()]
    opt = OPTS[name](params)
    grad, sq = th.zeros(P + 4), th.zeros(P)
    m = th.zeros(P) if name == "adam" else None
    step = th.tensor(0.0) if shared else None
    state = state_buffers(name, sq, m)
    link(params, opt, grad, dict(step=step, **state) if shared else state)
    return params, opt, grad, state, step, P


@pytest.mark.parametrize("shared", [True, False], ids=["shared_step", "own_steps"])
@pytest.mark.parametrize("name", ["rmsprop", "adam"])
def test_link_writes_through_the_flat_buffers(name, shared):
    params, opt, grad, state, step, P = build(name, shared)
    assert P == 11 and list(state) == {"adam": ["exp_avg", "exp_avg_sq"], "rmsprop": ["square_avg"]}[name]
    grad[:P] = th.arange(P, dtype=th.float32)
    for i, buf in enumerate(state.values()):
        buf.copy_(th.arange(P, dtype=th.float32) + 100.0 * (i + 1))
    o = 0
    for p in params:
        n = p.numel()
        assert p.grad.shape == p.shape and th.equal(p.grad.reshape(-1), grad[o:o + n])
        assert p.grad.data_ptr() == grad[o:o + n].data_ptr()
        for i, key in enumerate(state):
            got = opt.state[p][key]
            assert got.shape == p.shape and th.equal(got.reshape(-1), th.arange(o, o + n) + 100.0 * (i + 1))
        o += n
    steps = [opt.state[p]["step"] for p in params]
    if shared:
        assert all(s is step for s in steps)
        step += 2
        assert [float(s) for s in steps] == [2.0] * 4
    else:
        assert len({id(s) for s in steps}) == 4 and [float(s) for s in steps] == [0.0] * 4
        steps[1] += 3   # a second link keeps the steps it finds
        link(params, opt, grad, state)
        assert [float(opt.state[p]["step"]) for p in params] == [0.0, 3.0, 0.0, 0.0]
    opt.step()   # torch's own update runs on the views: the flat state moved, the grads did not
    assert all(float(buf.abs().sum()) > 0 for buf in state.values())


@pytest.mark.parametrize("name", ["rmsprop", "adam"])
def test_load_state_copies_back_after_a_round_trip(name):
    params, opt, grad, state, step, P = build(name, True)
    for i, buf in enumerate(state.values()):
        buf.copy_(th.arange(P, dtype=th.float32) * 0.5 + i)
    step += 7
    sd = state_dict_own_steps(opt)
    saved_steps = [v["step"] for v in sd["state"].values()]
    assert len({id(s) for s in saved_steps}) == 4 and all(float(s) == 7.0 and s is not step for s in saved_steps)
    assert written_by(sd) == name
    want = {k: b.clone() for k, b in state.items()}

    params2, opt2, grad2, state2, step2, _ = build(name, True)
    assert load_state(opt2, sd, params2, state2) == 7
    for k in state:
        assert th.equal(state2[k], want[k])
    # load_state_dict replaced the linked views (the caller re-links): the buffers hold the values all the same
    assert opt2.state[params2[0]][next(iter(state))].data_ptr() != next(iter(state2.values())).data_ptr()
    assert load_state(OPTS[name](params2), dict(sd, state={}), params2, state2) is None   # a file without steps


def test_refusal_of_the_other_optimisers_file_is_a_switch():
    params, opt, *_ = build("rmsprop", True)
    sd = state_dict_own_steps(opt)
    pa, oa, ga, sa, *_ = build("adam", True)
    with pytest.raises(ValueError, match=r"^dir/opt\.th was written by rmsprop, but this learner runs optimizer: adam\.$"):
        load_state(oa, sd, pa, sa, expect="adam", what="dir/opt.th")
    with pytest.raises(ValueError, match=r"^dir/opt\.th was written by RMSprop, but"):
        load_state(oa, sd, pa, sa, expect="adam", what="dir/opt.th", names={"rmsprop": "RMSprop"}.get)
    # switched off (the COMA learner): torch checks only the group sizes, so the file loads; no Adam key is in it
    assert load_state(oa, sd, pa, sa) == 0
    assert all(float(b.abs().sum()) == 0.0 for b in sa.values())
    # its own optimiser's file passes the switched-on check, and so does one whose groups name neither
    assert load_state(opt, sd, params, {"square_avg": th.zeros(11)}, expect="rmsprop", what="x") == 0
    assert written_by({"param_groups": [{"lr": 0.1}]}) is None and written_by({}) is None
