"""ACCritic (epymarl's `ac_critic`): the decentralised V critic of IA2C. Per-row input: the row's own obs | one-hot
agent id; network, names and HIP paths as CentralVCritic (modules/critics/centralv.py)."""
import torch as th

from ... import _lib
from .centralv import VCritic


class ACCritic(VCritic):
    KIND = _lib.MA_CRITIC_AC

    def _input_dim(self):
        return self.obs_dim + self.n_agents

    def build_inputs(self, batch, t=None):
        """(bs, max_t, n_agents, K) in torch, on the batch's device."""
        bs = batch.batch_size
        max_t = batch.max_seq_length if t is None else 1
        ts = slice(None) if t is None else slice(t, t + 1)
        obs = batch["obs"][:, ts]
        return th.cat([obs.float(), self._ids(bs, max_t, obs.device)], dim=-1)
