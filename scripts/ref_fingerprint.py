"""sha256 digests of everything the float64 / float32 test references compute, on the CPU.

    python scripts/ref_fingerprint.py OUT.json [--fields]

The evidence that a change to tests/ref64.py, hyper2_ref.py, ffn_ref.py, a2c_ref.py or coma_ref64.py moved no number:
run it before and after with the same interpreter and compare the two files byte for byte (profiles/ref_merge/).
Every entry point is looked up by its current name first and by the name it had before the three Q-learner steps were
folded into ref64.ref_step, so the same file runs in both trees.

Rows: ref64.SHAPES under each mixer test_gpu_grad_blocks.ROWS pairs it with, hyper2_ref.ROW_SHAPES, ffn_ref.ROW_SHAPES,
the four FLAGS on `part`, a2c_ref.ROWS and coma_ref64.SHAPES. Per row and step (step 1 from the float64 run's own
update, stored as float32): the run without overrides and the run that follows the other precision's decisions, in
float64 and in float32. The other precision is the reference's own float32 run where the step took a dtype before the
fold (two-layer hypernet, feed-forward agent, actor-critic) and the fp32 numpy oracle where it did not (the GRU rows,
COMA). Digested: every array of the result, clipped_flat, the stats, the block table's names, `classify`, and
`block_errors` between the two precisions. OUT.json holds one digest per row for the block names and one per row
and step over all of that step's field digests; `--fields` writes every field's digest and the block names in clear
instead (2e5 bytes), to find the field when two outputs differ. Digests of torch's float arithmetic belong to one
environment: this is not a test.
"""
import hashlib
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import a2c_ref, coma_ref64, ffn_ref, hyper2_ref, ref64  # noqa: E402
from tests.test_gpu_grad_blocks import ROWS as GRU_ROWS, oracle_clipped  # noqa: E402

F32, F64 = th.float32, th.float64
NEW = hasattr(ref64, "ref_step")


def entry(kind, name):
    """`name` of tests/ref64.py, else of the module that held the copy for `kind` (gru / h2 / ffn) before the fold."""
    if NEW:
        return getattr(ref64, name)
    return getattr({"gru": ref64, "h2": hyper2_ref, "ffn": ffn_ref}[kind], name)


def digest(x):
    if isinstance(x, np.ndarray):
        h = hashlib.sha256("{}{}".format(x.dtype, x.shape).encode())
        h.update(np.ascontiguousarray(x).tobytes())
        return h.hexdigest()
    if isinstance(x, (float, np.floating)):
        return float(x).hex()
    if isinstance(x, (bool, int, np.integer, str)):
        return x if isinstance(x, (bool, str)) else int(x)
    if isinstance(x, dict):
        return OrderedDict((str(k), digest(v)) for k, v in x.items() if v is not None)
    if isinstance(x, (list, tuple)):
        return [digest(v) for v in x]
    raise TypeError(type(x))


def one(x):
    """One digest of anything `digest` takes: a nested value (per-tensor gradients, a `judge` record) is digested as the
    JSON of its parts' digests. The first 20 hex digits of the sha256 are kept, to keep the output small."""
    d = digest(x)
    return (d if isinstance(x, np.ndarray) else hashlib.sha256(json.dumps(d).encode()).hexdigest())[:20]


def fields(r):
    """One digest per field of a result namespace that holds something (a None field is a field not there)."""
    return OrderedDict((k, one(v)) for k, v in sorted(vars(r).items()) if v is not None)


# ---------------------------------------------------------------------------------------------- the Q-learner step
def decisions(r):
    d = dict(cur_max_override=r.cur_max_actions, relu_override=r.pre > 0)
    if getattr(r, "pre2", None) is not None:
        d["hid_relu_override"] = r.pre2 > 0
    if getattr(r, "a1", None) is not None:
        d["hyp_relu_override"] = r.a1 > 0
    return d


def classified(kind, own, dec):
    """`classify` with the kind's own third decision: the feed-forward agent's second relu, the hypernet's layer 1."""
    third = "hid_relu" if kind == "ffn" else "hyp_relu"
    if NEW:
        return ref64.classify(own, dec["cur_max_override"], dec["relu_override"],
                              **{"got_" + third: dec[third + "_override"]})
    return entry(kind, "classify")(own, dec["cur_max_override"], dec["relu_override"], dec[third + "_override"])


def q_row(kind, case):
    """A two-layer-hypernet or feed-forward row: float64 and float32, free and following each other."""
    step = entry(kind, "ref_step")
    out = OrderedDict(blocks=list(entry(kind, "grad_blocks")(case)))
    p = t = entry("h2", "flat_of")(case)
    sq = np.zeros_like(p, np.float64)
    for k in range(2):
        nb, _ = case.batch(k)
        r64, r32 = step(case, p, t, nb), step(case, p, t, nb, dtype=F32)
        f64, f32 = step(case, p, t, nb, **decisions(r32)), step(case, p, t, nb, dtype=F32, **decisions(r64))
        be = entry(kind, "block_errors")
        out["step{}".format(k)] = OrderedDict(
            r64=fields(r64), r32=fields(r32), r64_following_r32=fields(f64), r32_following_r64=fields(f32),
            e32=one(be(f32.clipped_flat, r64.clipped, case)), e32_free=one(be(r32.clipped_flat, f64.clipped, case)),
            classify=one(classified(kind, r64, decisions(r32))))
        p, sq = entry("h2", "rmsprop")(case, p, sq, r64.clipped_flat)
        p = p.astype(np.float32)
    return out


def gru_row(case):
    """A one-layer GRU row: float64, free and following the fp32 numpy oracle's decisions (the step took no dtype)."""
    from oracle.qlearner_np import OracleQLearner, fc1_preacts
    step = ref64.ref_step if NEW else ref64.ref64_step
    out = OrderedDict(blocks=list(ref64.grad_blocks(case)))
    o = OracleQLearner(case.agent_params, case.mixer_params, case.cfg())
    for k in range(2):
        nb, _ = case.batch(k)
        p, t = o.flat("params"), o.flat("targets")
        got = o.forward(nb)["cur_max_actions"]
        on = fc1_preacts(o.p, nb["obs"], nb["actions_onehot"], o.input_flags) > 0
        r, f = step(case, p, t, nb), step(case, p, t, nb, cur_max_override=got, relu_override=on)
        out["step{}".format(k)] = OrderedDict(
            r64=fields(r), r64_following_oracle=fields(f),
            e32=one(ref64.block_errors(oracle_clipped(o, nb, got, on), f.clipped, case)))
        o.train(nb, 1000 * k, case.episodes[k])
    return out


# ---------------------------------------------------------------------------------------------- actor-critic, COMA
def a2c_row(row):
    c = a2c_ref.A2CCase(row)
    b, st = c.batch(), c.init_state()
    bl = a2c_ref.blocks(c)
    out = OrderedDict(blocks={k: list(v) for k, v in bl.items()})
    for k in range(2):
        r64, r32 = a2c_ref.a2c_ref_step(c, st, b, F64), a2c_ref.a2c_ref_step(c, st, b, F32)
        f64 = a2c_ref.a2c_ref_step(c, st, b, F64, Vt_override=r32.Vt)
        f32 = a2c_ref.a2c_ref_step(c, st, b, F32, Vt_override=r64.Vt)
        rec = OrderedDict(r64=fields(r64), r32=fields(r32), r64_following_r32=fields(f64),
                          r32_following_r64=fields(f32))
        if r64.live:
            rec["judge"] = one(a2c_ref.judge(c, r64, r32, a2c_ref.quantities(r32))[0])
            rec["judge_updates"] = one(a2c_ref.judge_updates(
                c, st, dict(agent=r32.agent_grads, critic=r32.critic_grads), r32.new)[0])
        out["step{}".format(k)] = rec
        st = a2c_ref.to32(r32.new)
    return out


def coma_row(row):
    c = coma_ref64.synth_case(row)
    a, cr = coma_ref64.flat_of(c.agent_params), coma_ref64.flat_of(c.critic_params)
    state = (a, cr, cr.copy(), np.zeros_like(a), np.zeros_like(cr))
    out = OrderedDict(blocks={k: list(v) for k, v in coma_ref64.coma_blocks(c).items()})
    for k in range(2):
        nb, _ = c.batch(k)
        r = coma_ref64.coma_ref64_step(c, *state, nb, c.epsilon[k])
        o = coma_ref64.oracle_at(c, *state)
        o.train(nb, 1000 * (k + 1), 8 * k, c.epsilon[k])
        orc = coma_ref64.oracle_quantities(o, state[1])
        out["step{}".format(k)] = OrderedDict(r64=fields(r), judge=one(coma_ref64.judge(c, r, orc, orc)[0]))
        f = lambda d: coma_ref64.flat_of(d).astype(np.float32)   # noqa: E731
        state = (f(r.agent_params), f(r.critic_params), state[2], f(r.agent_sq), f(r.critic_sq))
    return out


def main(path, by_field=False):
    th.set_num_threads(1)
    out = OrderedDict()
    for shape, mixer in sorted({(v[0], v[1]) for v in GRU_ROWS.values()}):
        out["gru/{}_{}".format(shape, mixer)] = gru_row(ref64.synth_case(shape, mixer))
    for row in hyper2_ref.ROW_SHAPES:
        out["h2/" + row] = q_row("h2", hyper2_ref.synth_case2(row))
    for row in ffn_ref.ROW_SHAPES:
        out["ffn/" + row] = q_row("ffn", ffn_ref.synth_case(row))
    for flags in ffn_ref.FLAGS:
        out["ffn/part_flags{}{}".format(*map(int, flags))] = q_row("ffn", ffn_ref.synth_case("part", flags=flags))
    for row in a2c_ref.ROWS:
        out["a2c/" + row] = a2c_row(row)
    for row in coma_ref64.SHAPES:
        out["coma/" + row] = coma_row(row)
    if not by_field:
        out = OrderedDict((row, OrderedDict((k, one(v)) for k, v in rec.items())) for row, rec in out.items())
    with open(path, "w") as f:
        rows = ["{}: {}".format(json.dumps(k), json.dumps(v, indent=1 if by_field else None)) for k, v in out.items()]
        f.write("{\n" + ",\n".join(rows) + "\n}\n")   # a row a line, unless by field
    print("{} rows -> {}".format(len(out), path))


if __name__ == "__main__":
    main(sys.argv[1], "--fields" in sys.argv[2:])
