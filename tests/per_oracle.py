"""ORACLE for prioritized episode replay (PrioritizedReplayBuffer; pymarl_amd/csrc/per_kernels.hpp) — test
infrastructure only.

`per_sample` restates the sampler in numpy, in float64 (the checker) or float32 (the arithmetic the kernel is specified
in: `tau = ((float)b + u[b]) * (total / (float)B)` with every operation rounded to f32; the order of the scan is not
fixed by the specification, so the float32 form is a check only where all prefix sums are exact, which
`exact_fixture` guarantees):

    q_i = p_i^alpha (alpha == 1: p_i), cum = inclusive scan of q over the N live slots, total = cum[N-1]
    id_b = min(N-1, #{i < N : cum[i] <= tau_b})
    w_b = (N q_{id_b} / total)^(-beta), divided by max_b w_b (beta == 0: exactly 1)

`priority_update` restates the write-back in float32 with the serial ascending-t sum of the kernel.

`PEROracleQLearner` is the numpy QLearner of oracle/qlearner_np.py (with tests/lambda_oracle.py's targets when
cfg["td_lambda"] > 0) whose loss carries the per-episode weights `self.weights` (B,):
loss = sum_b w_b sum_t l(td m) / sum m, so dLoss/dQ_tot of every row of episode b is the parent's times w_b. The
other stats stay unweighted. At weights == 1 every number equals the parent's, bit for bit.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from oracle.qlearner_np import F32, OracleQLearner, agent_backward, qmix_backward
from tests.lambda_oracle import LambdaOracleQLearner

PER_THREADS = 1024     # per_kernels.hpp
PER_SCAN_DEPTH = 10


def chain_len(n_live):
    """D of per_kernels.hpp: the longest addition chain behind any prefix sum the sampler compares against,
    2 * ceil(N / PER_THREADS) + PER_SCAN_DEPTH."""
    return 2 * (-(-int(n_live) // PER_THREADS)) + PER_SCAN_DEPTH


def per_sample(prio, n_live, u, alpha, beta, dtype=np.float64):
    """(ids int64 [B], weights [B], dict(cum, tau, total, q)) in `dtype` arithmetic."""
    dt = np.dtype(dtype).type
    N, B = int(n_live), len(u)
    p = np.asarray(prio)[:N].astype(dt)
    q = p if alpha == 1 else np.power(p, dt(alpha)).astype(dt)
    cum = np.cumsum(q, dtype=dt)
    total = cum[-1]
    seg = dt(total / dt(B))
    tau = ((np.arange(B).astype(dt) + np.asarray(u).astype(dt)).astype(dt) * seg).astype(dt)
    ids = np.minimum(N - 1, np.searchsorted(cum, tau, side="right")).astype(np.int64)   # #{cum <= tau}
    if beta == 0:
        w = np.ones(B, dt)
    else:
        w = np.power((dt(N) * q[ids]) / total, dt(-beta)).astype(dt)
    w = (w / w.max()).astype(dt)
    return ids, w, dict(cum=cum, tau=tau, total=total, q=q)


def interval_violations(ids, prio, n_live, u, alpha, tol_chain):
    """The draws whose id breaks  cum64[i-1] - tol <= tau64 <= cum64[i] + tol,  tol = tol_chain 2^-23 total."""
    _, _, s = per_sample(prio, n_live, u, alpha, 0.0, np.float64)
    cum, tau = s["cum"], s["tau"]
    tol = tol_chain * 2.0 ** -23 * float(s["total"])
    ids = np.asarray(ids)
    lo = np.where(ids > 0, cum[np.maximum(ids - 1, 0)], 0.0)
    bad = (ids < 0) | (ids >= n_live) | (lo - tol > tau) | (tau > cum[np.clip(ids, 0, n_live - 1)] + tol)
    return [(int(b), int(ids[b]), float(tau[b])) for b in np.nonzero(bad)[0]]


def exact_fixture(n_live, batch, seed, n_slots=None, boundary=False, stale=None):
    """(prio f32 [n_slots], u f32 [batch]) on which every prefix sum, total / batch and tau are exact in float32:
    priorities are multiples of 2^-10 in (0, 2], the last episode's is raised until the total is a multiple of
    batch * 2^-2 (so total / batch is a multiple of 2^-2 and every tau a multiple of 2^-10 below 2^14), u are multiples
    of 2^-8. boundary: u[0] = 0.5 and two neighbouring priorities are shifted so that a prefix sum ends exactly at
    tau_0 (the next episode must be drawn). stale: value of the slots >= n_live (never drawn)."""
    rng = np.random.RandomState(seed)
    n_slots = n_live if n_slots is None else n_slots
    k = rng.randint(1, 2049, size=n_live).astype(np.int64)   # priorities in units of 2^-10
    unit = batch * 256                                          # total in units of 2^-10: seg = total / batch is a
    rem = int(k.sum() % unit)                                   # multiple of 2^-2, so u * seg (u in 2^-8) is exact
    k[-1] += unit - rem                                         # k[-1] <= 2048 + unit: still exact (N * that < 2^24)
    assert k.sum() % unit == 0 and k.sum() < 2 ** 24
    prio = np.full(n_slots, 1.0 if stale is None else stale, np.float32)
    prio[:n_live] = (k / 1024.0).astype(np.float32)
    u = (rng.randint(0, 256, size=batch) / 256.0).astype(np.float32)
    if boundary:
        # tau_0 = seg / 2 with u[0] = 0.5; shift priority between two neighbours so that a prefix sum ends exactly
        # there (the total, and with it seg, stays as it is)
        half = int(k.sum() // batch) // 2                       # in units of 2^-10
        cum = np.cumsum(k)
        i = int(np.searchsorted(cum, half, side="left"))        # the first prefix sum >= half
        assert i < n_live - 1, "no room for a boundary in this fixture"
        k[i + 1] += cum[i] - half
        k[i] -= cum[i] - half                                   # still > 0: cum[i-1] < half
        assert (k > 0).all() and np.cumsum(k)[i] == half
        prio[:n_live] = (k / 1024.0).astype(np.float32)
        u[0] = np.float32(0.5)
    return prio, u


def priority_update(tda, mask, eps, n_agents_div=1):
    """tda (B, T) the tail's |td m| record, mask (B, T) the learner's mask -> p (B,) float32:
    a = serial ascending-t f32 sum of tda, c = sum of mask (x n_agents without a mixer), p = a / max(c, 1) + eps."""
    tda, mask = np.asarray(tda, F32), np.asarray(mask, F32)
    a = np.zeros(tda.shape[0], F32)
    c = np.zeros(tda.shape[0], F32)
    for t in range(tda.shape[1]):
        a = (a + tda[:, t]).astype(F32)
        c = (c + mask[:, t]).astype(F32)
    c = (c * F32(n_agents_div)).astype(F32)
    return ((a / np.maximum(c, F32(1.0))).astype(F32) + F32(eps)).astype(F32)


class PEROracleQLearner(LambdaOracleQLearner):
    """OracleQLearner (LambdaOracleQLearner's targets when cfg["td_lambda"] > 0) with the importance-weighted loss.
    Set `weights` (B,) before forward / gradients / train; None means 1."""

    weights = None

    def _w(self, B):
        w = np.ones(B, F32) if self.weights is None else np.asarray(self.weights, F32)
        assert w.shape == (B,)
        return w.reshape(B, 1, 1)

    def forward(self, batch, keep_cache=False, cur_max_override=None, relu_override=None):
        base = LambdaOracleQLearner if self.cfg.get("td_lambda", 0.0) > 0 else OracleQLearner
        fw = base.forward(self, batch, keep_cache, cur_max_override, relu_override)
        c = self.cfg
        mtd = fw["td"] * fw["mask"]
        w = np.broadcast_to(self._w(mtd.shape[0]), mtd.shape)
        hd = F32(c.get("huber_delta", 0.0))
        if hd > 0:
            ell = np.where(np.abs(mtd) <= hd, F32(0.5) * mtd * mtd, hd * (np.abs(mtd) - F32(0.5) * hd)).astype(F32)
        else:
            ell = mtd * mtd
        fw["loss"] = float(F32((w * ell).astype(F32).sum()) / fw["mask_sum"])
        fw["weights"] = w
        return fw

    def gradients(self, batch, fw=None, cur_max_override=None, relu_override=None):
        """OracleQLearner.gradients with dq_tot of every row multiplied by its episode's weight."""
        c = self.cfg
        fw = fw or self.forward(batch, keep_cache=True, cur_max_override=cur_max_override,
                                relu_override=relu_override)
        td, m, msum = fw["td"], fw["mask"], fw["mask_sum"]
        hd = F32(c.get("huber_delta", 0.0))
        if hd > 0:
            dq_tot = (np.clip(td * m, -hd, hd) * m * (F32(1.0) / msum)).astype(F32)
        else:
            dq_tot = ((F32(2.0) * (td * m)) * (F32(1.0) / msum)) * m
        dq_tot = (dq_tot * fw["weights"]).astype(F32)
        B, T = td.shape[:2]
        n = c["n_agents"]
        mg = OrderedDict()
        if c["mixer"] == "qmix":
            dchosen, mg = qmix_backward(self.mp, fw["mcache"], dq_tot.reshape(-1).astype(F32))
            dchosen = dchosen.reshape(B, T, n)
        elif c["mixer"] == "vdn":
            dchosen = np.broadcast_to(dq_tot, (B, T, n)).astype(F32)
        else:
            dchosen = dq_tot.astype(F32)
        A = fw["mac_out"].shape[-1]
        dmac = np.zeros_like(fw["mac_out"])
        oh = np.zeros((B, T, n, A), F32)
        np.put_along_axis(oh, fw["actions"], 1.0, axis=3)
        dmac[:, :-1] = oh * dchosen[..., None]
        ag = agent_backward(self.p, fw["acache"], dmac)
        return ag, mg, fw
