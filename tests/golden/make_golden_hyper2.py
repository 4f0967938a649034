"""Generate tests/golden/tiny_qmix_h2.npz: the REFERENCE's own CPU QLearner trained with a two-layer QMIX mixer.

    python tests/golden/make_golden_hyper2.py

Not part of the product and never run on the GPU box (it needs /root/reference, like make_golden.py, whose recipe and
file format this reuses unchanged). The reference fork's QMixer ignores hypernet_layers, so the name
`learners.q_learner.QMixer` is rebound to upstream PyMARL's two-layer module as restated in tests/hyper2_ref.py before
the learner is constructed: the mixer's arithmetic is the restatement's, while the loss, double-Q target, masking,
clip_grad_norm_, RMSprop, the target update and the logged stats are the reference's own code. The weights are
numpy-seeded (init_params over hyper2_ref.mixer2_shapes, seed weight_seed + 100) and loaded via load_state_dict.

The data and seeds are make_golden.py's `tiny_qmix` (TINY); hypernet_embed is 64. Two steps, the second with a target
update (episode 200), and no initial parameters in the file (they are the seeded ones): every stored vector has the
46058 parameters' length, and the file must stay under 1 MiB.
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (puts the repository and the reference's src on sys.path)

import numpy as np  # noqa: E402

import learners.q_learner as ref_q_learner  # noqa: E402  (reference)
from tests.hyper2_ref import RefQMixer2, mixer2_shapes  # noqa: E402

HE = 64


class TwoLayerQMixer(RefQMixer2):
    """RefQMixer2 behind the reference's QMixer(args) constructor."""

    def __init__(self, args):
        super().__init__(args.n_agents, int(np.prod(args.state_shape)), args.mixing_embed_dim, HE)


if __name__ == "__main__":
    ref_q_learner.QMixer = TwoLayerQMixer
    G.qmix_param_shapes = lambda S, n, E: mixer2_shapes(S, n, HE, E)   # the weights build() draws and loads
    G.run_case("tiny_qmix_h2", dict(G.TINY, mixer="qmix", hypernet_embed=HE, steps=2, episodes=[0, 200],
                                     record_actions_steps=2, store_params=False))
