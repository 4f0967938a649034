"""Generate tests/golden/tiny_qmix_adam.npz (+ tiny_qmix_adam_state.npz): the REFERENCE's own CPU QLearner trained with
torch.optim.Adam.

    python tests/golden/make_golden_adam.py

Not part of the product and never run on the GPU box (it needs /root/reference, like make_golden.py, whose recipe and
file format this reuses unchanged). The reference builds `RMSprop(params=..., lr=..., alpha=..., eps=...)`
(q_learner.py:30), so the name `learners.q_learner.RMSprop` is rebound to a factory returning
torch.optim.Adam(params, lr=lr) (torch's betas, eps and weight_decay: what `optimizer: adam` selects by default) before
the learner is constructed, and `make_golden.flat_sqavg` to read exp_avg_sq. The loss, double-Q targets, masking,
clip_grad_norm_, the target update and the logged stats are the reference's own code.

The data and seeds are make_golden.py's `tiny_qmix` (TINY): four steps, a target update at step 2 (episode 200), no
initial parameters in the file (they are the seeded ones).

Adam divides by |g|: an element whose gradient is rounding noise moves by about +-lr in either implementation, whatever
the sign the noise gives it. So the optimiser's step is wrapped to see each step's clipped gradient, and the second
file records, beside Adam's final moments, a bit mask (`noise_mask`, np.packbits) of the elements whose reference
gradient at ANY step satisfied

    0 < |g| < NOISE_ROOM * tol(block) * max|ref64 block|

where tol(block) is what tests/ref64.tolerances grants the element's gradient block (its finest block of
ref64.grad_blocks) from the reference's own fp32 error against tests/ref64.ref_step at the same state with the same
double-Q decisions. tests/test_gpu_adam.py bounds those elements by Adam's worst-case step and every other one
tightly. The mask may cover at most MASK_MAX of the parameters: asserted here (change `data_seed` below if TINY's
seeds ever exceed it), with the share printed and stored.
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (puts the repository and the reference's src on sys.path)

import numpy as np  # noqa: E402
import torch as th  # noqa: E402

import learners.q_learner as ref_q_learner  # noqa: E402  (reference)

NAME = "tiny_qmix_adam"
NOISE_ROOM = 100.0
MASK_MAX = 0.02
CASE = dict(G.TINY, mixer="qmix", store_params=False)   # data_seed: TINY's

LEARNERS, SEEN = [], []


def adam_factory(params, lr, alpha=None, eps=None):
    """Stands in for the reference's RMSprop(params=, lr=, alpha=, eps=): Adam at torch's defaults, its step wrapped to
    record the state the step's forward ran from and the clipped gradient it applies."""
    opt = th.optim.Adam(params, lr=lr)
    step = opt.step

    def recording_step(*a, **k):
        learner = LEARNERS[-1]
        SEEN.append(dict(params=G.flat_params(learner), targets=G.flat_targets(learner), grads=G.flat_grads(learner)))
        return step(*a, **k)

    opt.step = recording_step
    return opt


def flat_state(learner, key):
    st = learner.optimiser.state
    return np.concatenate([st[p][key].cpu().numpy().ravel() for p in learner.params]).astype(np.float32)


def noise_mask(case):
    """The elements whose reference gradient was rounding noise at some step (module docstring), and the share."""
    from tests import ref64
    blocks = ref64.grad_blocks(case)
    names = list(case.agent_shapes) + list(case.mixer_shapes)
    mask = np.zeros(sum(int(np.prod(s)) for s in list(case.agent_shapes.values()) + list(case.mixer_shapes.values())),
                    bool)
    for k, seen in enumerate(SEEN):
        nb, _ = case.batch(k)
        acts = case.z["cur_max_actions"][k][:, :nb["obs"].shape[1] - 1].astype(np.int64)
        r = ref64.ref_step(case, seen["params"], seen["targets"], nb, cur_max_override=acts)
        e32 = ref64.block_errors(seen["grads"], r.clipped, case)
        tol = ref64.tolerances(e32)
        thr = {n_: np.zeros(r.clipped[n_].shape) for n_ in names}
        for whole in (True, False):   # every tensor's own block first, then its finer blocks over it
            for b, (n_, idx) in blocks.items():
                if (b == n_) != whole:
                    continue
                scale = float(np.abs(r.clipped[n_][idx]).max()) or float(np.abs(r.clipped[n_]).max())
                thr[n_][idx] = NOISE_ROOM * tol[b] * scale
        g = np.abs(seen["grads"].astype(np.float64))
        step_mask = (g > 0) & (g < np.concatenate([thr[n_].ravel() for n_ in names]))
        print("step {}: {} noise elements, worst block e32 {:.3g}".format(k, int(step_mask.sum()), max(e32.values())))
        mask |= step_mask
    return mask, float(mask.mean())


if __name__ == "__main__":
    ref_q_learner.RMSprop = adam_factory
    G.flat_sqavg = lambda learner: flat_state(learner, "exp_avg_sq")
    build = G.build

    def recording_build(case):
        out = build(case)
        LEARNERS.append(out[3])
        return out

    G.build = recording_build
    G.run_case(NAME, CASE)
    assert len(SEEN) == CASE["steps"] and type(LEARNERS[-1].optimiser) is th.optim.Adam

    from tests.golden_utils import Case  # noqa: E402
    case = Case(NAME)
    mask, share = noise_mask(case)
    print("noise mask: {} of {} parameters ({:.3%})".format(int(mask.sum()), mask.size, share))
    assert share <= MASK_MAX, "the noise mask covers {:.3%} > {:.0%}: change data_seed".format(share, MASK_MAX)
    path = os.path.join(HERE, NAME + "_state.npz")
    np.savez_compressed(path, exp_avg_final=flat_state(LEARNERS[-1], "exp_avg"), noise_mask=np.packbits(mask),
                        noise_share=np.array(share), noise_room=np.array(NOISE_ROOM), lr=np.array(CASE.get("lr", 5e-4)))
    for f in (NAME + ".npz", NAME + "_state.npz"):
        size = os.path.getsize(os.path.join(HERE, f))
        print(f, size // 1024, "KB")
        assert size < 1 << 20, f
