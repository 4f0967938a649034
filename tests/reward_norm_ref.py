"""Float64 numpy reference of reward standardisation with running statistics (standardise_rewards;
reward_norm_kernel, pymarl_amd/csrc/epymarl_kernels.hpp; the semantics are include/mq_learner.h's, mq_set_reward_norm).

    x = reward[:, :-1] of the batch, M values, unmasked
    bm = mean(x);  bv = sum (x - bm)^2 / (M - 1)          (M = 1: 0)
    delta = bm - mean;  tot = count + M
    mean' = mean + delta M / tot;  var' = (var count + bv M + delta^2 count M / tot) / tot;  count' = tot
    r_std = (r - mean') / sqrt(var')                       (the UPDATED statistics, no epsilon)

tests/test_epymarl_keys_host.py checks the merge against a torch transcription; tests/test_gpu_epymarl_keys.py checks the
kernel against this file.
"""
import numpy as np

INIT = (0.0, 1.0, 1e-4)   # (mean, var, count) of fresh statistics


def batch_moments(x):
    """(bm, bv, M) of the batch's rewards in float64; bv is the unbiased variance, 0 for a single value."""
    x = np.asarray(x, np.float64).reshape(-1)
    M = x.size
    bm = float(x.sum() / M)
    bv = float(((x - bm) ** 2).sum() / (M - 1)) if M > 1 else 0.0
    return bm, bv, M


def merge(state, x):
    """The running (mean, var, count) after the batch x."""
    mean, var, count = (float(v) for v in state)
    bm, bv, M = batch_moments(x)
    delta = bm - mean
    tot = count + M
    mean1 = mean + delta * M / tot
    var1 = (var * count + bv * M + delta * delta * count * M / tot) / tot
    return mean1, var1, tot


def standardise(state, x):
    """(new state, r_std): r_std in float64 and x's shape, from the statistics AFTER the merge."""
    new = merge(state, x)
    x = np.asarray(x, np.float64)
    return new, (x - new[0]) / np.sqrt(new[1])
