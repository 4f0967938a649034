"""The COMA critic and actor of train() judged per block against the float64 reference (tests/coma_ref64.py).

tests/test_gpu_coma.py gates the critic parameters with an absolute band of twenty learning rates, which a first
RMSprop step fills whatever the gradient's size, and the agent's gradient as one flat vector, which is fc2.bias's; the
critic's last gradient and its square_avg it compares with nothing. Here, per row and critic path, two train() calls
(step 0 from the case's weights and zero optimiser state, step 1 from the GPU's own parameters, target critic and both
square_avg after step 0, read back and given to the reference and to the fp32 oracle alike), and per step:

1. the reference's kink_minima are above the row's margin, before train() runs (the relus' decisions cannot be read
   back; coma_ref64.SHAPES has the margins and how the seeds were found);
2. `_cgrad[:Pc]` against the reference's last live step's clipped gradient per critic block, `_cgrad[Pc]` that step's
   mask sum;
3. `_csq` per critic block: it holds every live step's g^2, so a wrong magnitude at any step shows;
4. the critic update p_after - p_before per block on the scale of max|update|, with the floor
   max(2e-7, 2^-24 max|p| / max|update|) that fp32 storage of the parameters sets and the cap 1e-3;
5. the agent's clipped gradient per agent block; its norm and the mean of the live steps' critic norms (all the
   learner reports of them; `_csq` holds each step's magnitude) to 1e-5 relative;
6. Q values, targets and pi to 1e-5, the nine stats to 1e-4 |ref| + 1e-6, critic_steps exactly;
7. everything finite.

The tolerance of 2, 3 and 5 is ref64's min(1e-5, 16 max(e32, 2e-7)) with e32 the oracle's error on the same block from
the same state. Each row of coma_ref64.SHAPES is the smallest shape at which the edge it is named for exists (DESIGN.md
"Parity"); the rows the persistent chain accepts run through it and through the three launches (MQ_PLAN coma_chain=0),
the others must fall back to the three launches on their own. The per-block err / e32 / tol / ratio, the kink minima
and the path go to $MQ_PARITY_DIR/parity_coma64_<row>_<path>.json.
"""
import numpy as np
import pytest

from tests import coma_ref64 as C
from tests import test_gpu_parity as P
from tests.golden_utils import COMA_STATS
from tests.gpu_helpers import rel, set_switch

pytestmark = pytest.mark.gpu

# (row, the switch's value, the path the row must report): no switch wherever the shape alone decides
RUNS = [(r, None, "chain" if r in C.CHAIN_ROWS else "three_launch") for r in C.SHAPES] + \
       [(r, "0", "three_launch") for r in C.CHAIN_ROWS]


@pytest.fixture(scope="module")
def coma_rows():
    return {}


def learner_state(learner):
    """(agent, critic, target critic, agent square_avg, critic square_avg) as the learner holds them, flat float32."""
    Pa, Pc = learner.n_agent_params, learner.n_critic_params
    return tuple(t[:n].detach().cpu().numpy().copy() for t, n in (
        (learner._agent, Pa), (learner._critic, Pc), (learner._tcritic, Pc), (learner._asq, Pa), (learner._csq, Pc)))


@pytest.mark.parametrize("row,switch,path", RUNS, ids=["{}-{}".format(r, "forced3" if s else p) for r, s, p in RUNS])
def test_coma_blocks_vs_ref64(coma_rows, row, switch, path, monkeypatch):
    from tests.gpu_helpers import build_coma
    if row not in coma_rows:
        coma_rows[row] = C.synth_case(row)
    c = coma_rows[row]
    margin = C.SHAPES[row]["margin"]
    set_switch(monkeypatch, "coma_chain", switch)   # read once, at handle creation
    args, buf, mac, learner, logger = build_coma(c)
    Pa, Pc = learner.n_agent_params, learner.n_critic_params
    np.random.seed(c.sampler_seed)
    records, bad = [], []
    for k in range(2):
        batch = buf.sample(c.B)
        assert np.array_equal(batch.ep_ids_np, c.z["ids"][k])
        batch = batch[:, :batch.max_t_filled()]
        nb, _ = c.batch(k)
        state = learner_state(learner)
        r = C.coma_ref64_step(c, *state, nb, c.epsilon[k])
        for relu, v in r.kink_minima.items():   # 1, before the GPU runs
            assert v > margin, "{} step {}: min|{}| = {:.3g} over live rows is within the margin {:g} of the kink; " \
                "choose another seed for this row".format(row, k, relu, v, margin)
        if "live" in C.SHAPES[row]:   # the holes row: five steps, those at the two unwritten slots skipped
            assert nb["filled"].shape[1] == 6 and r.live_steps == C.SHAPES[row]["live"], (row, r.live_steps)
        mac.action_selector.epsilon = c.epsilon[k]
        learner.train(batch, 1000 * (k + 1), 8 * k)
        assert learner.critic_path() == path, (row, learner.critic_path())
        st = learner.last_stats()
        o = C.oracle_at(c, *state)
        o.train(nb, 1000 * (k + 1), 8 * k, c.epsilon[k])
        after = learner_state(learner)
        cgrad = learner._cgrad.detach().cpu().numpy()
        got = dict(cgrad_last=cgrad[:Pc], csq=after[4], cdelta=after[1].astype(np.float64) - state[1],
                   agrad=learner._agrad[:Pa].detach().cpu().numpy())
        for q, v in got.items():   # 7
            assert np.isfinite(v).all(), (row, k, q)
        assert all(np.isfinite(a).all() for a in after) and all(np.isfinite(st[s]) for s in COMA_STATS), (row, k)
        rec, bad_k = C.judge(c, r, got, C.oracle_quantities(o, state[1]))   # 2, 3, 4, 5
        bad += [(k,) + b for b in bad_k]
        w = C.worst(rec)
        qerr = {name: rel(learner.last_intermediate(i).cpu().numpy(), ref)
                for i, name, ref in ((0, "q_vals", r.q_vals), (1, "targets", r.targets), (2, "pi", r.pi))}
        cnorm = sum(r.critic_norms) / len(r.critic_norms)
        norm_err = dict(critic=abs(st["critic_grad_norm"] - cnorm) / cnorm,
                        agent=abs(st["agent_grad_norm"] - r.agent_norm) / r.agent_norm)
        print("{} {} step {}: live steps {}, worst ratio {:.2f} at {} {} (err {:.3g}, e32 {:.3g}, tol {:.3g}); worst "
              "update err {:.3g}; norms rel {:.2g} / {:.2g}; q / targets / pi {:.2g} / {:.2g} / {:.2g}; kinks {}"
              .format(
                  row, path, k, r.live_steps, w[2], w[0], w[1], rec[w[0]][w[1]]["err"], rec[w[0]][w[1]]["e32"],
                  rec[w[0]][w[1]]["tol"], max(v["err"] for v in rec["cdelta"].values()), norm_err["critic"],
                  norm_err["agent"], qerr["q_vals"], qerr["targets"], qerr["pi"],
                  {a: "{:.3g}".format(b) for a, b in r.kink_minima.items()}))
        records.append(dict(step=k, path=path, live_steps=r.live_steps, kink_minima=r.kink_minima, margin=margin,
                            worst=dict(quantity=w[0], block=w[1], ratio=w[2]), norm_err=norm_err, errors=qerr,
                            stats={s: (st[s], r.stats[s]) for s in COMA_STATS}, blocks=rec))
        assert cgrad[Pc] == r.mask_sums[-1], (row, k, cgrad[Pc], r.mask_sums[-1])   # 2
        assert norm_err["critic"] <= 1e-5 and norm_err["agent"] <= 1e-5, (row, k, norm_err)   # 5
        for name, e in qerr.items():   # 6
            assert e < 1e-5, (row, k, name, e)
        for s in COMA_STATS:
            assert abs(st[s] - r.stats[s]) <= 1e-4 * abs(r.stats[s]) + 1e-6, (row, k, s, st[s], r.stats[s])
        assert int(round(st["critic_steps"])) == r.stats["critic_steps"] == len(r.live_steps), (row, k)
    P.write_record("coma64", "{}_{}".format(row, path), records)
    assert not bad, (row, path, bad)
