// PPO learner kernels (include/ma_a2c.h ma_set_ppo): epymarl's ppo_learner (MAPPO / IPPO) on the
// actor-critic learner's step. A train() runs E epochs over one batch; everything an epoch needs but the policy step
// and the per-epoch stats row is the actor-critic learner's (a2c_kernels.hpp), launched by a2c_host.hpp.
//
//   ppo_policy_kernel  softmax policy, entropy, the clipped-surrogate loss sums and dLoss/dlogits, a wave per row
//   ppo_stats_kernel   after both applies: the epoch's stats[MA_NSTATS] into its row of the caller's [E][MA_NSTATS]
//
// Bounds, from the code: the policy kernel tests its row tr against RT before the first access (old, ratio and td
// are [RT], dL [RT][Ap], pi [RT][A], part [gridDim.x][8]); the taken action is clamped to [0, A) before it selects a
// lane; the stats kernel is one wave, lane < MA_NSTATS.
#pragma once
#include "a2c_kernels.hpp"

namespace mq {

constexpr int PPO_SUM_CLIPPED = 5;    // column of the policy sums (agrad's tail): live rows whose gradient is cut
constexpr int PPO_STAT_CLIPPED = 15;  // where ppo_stats_kernel leaves that count in the epoch's stats row

// a2c_policy_kernel's shape and arithmetic (one wave per (t, row), lanes = actions, A <= 64) with the clipped
// surrogate in the log-probability's place. lp = log(pi_u + 1e-10); FIRST (epoch 0): old[tr] = lp is written, else
// read; ratio = exp(lp - old), adv = td (a constant), s1 = ratio adv, s2 = clamp(ratio, lo, hi) adv, the row's loss
// term -(min(s1, s2) + ec H) m. Autograd of min / clamp: w = 1 where lo <= ratio <= hi or s1 < s2, else 0 (the
// gradient is cut), c = (w ratio) adv, and down to the logits, live rows,
//   g_j = -m [c [j == u] / (p_j + 1e-10) - ec (log(p_j + 1e-10) + p_j / (p_j + 1e-10))]
//   dlogit_k = p_k (g_k - sum_j p_j g_j), zero at masked-before-softmax actions and on dead rows.
// ratio = 1 and w = 1 give c = adv bit for bit: epoch 0's dlogits are a2c_policy_kernel's. Writes dL [RT][Ap] (pad
// columns zero), pi [RT][A], ratio [RT], per-block sums part[b][0..5]: the loss terms, sum m, sum adv m,
// sum max(pi) m, sum H m, and the number of live rows with w = 0. No atomics.
template <bool FIRST>
__global__ __launch_bounds__(256) void ppo_policy_kernel(Dims d, Rep rp, const float* __restrict__ logits,
                                                         const float* __restrict__ td, float ec, float lo, float hi,
                                                         int mbs, int Ap, float* __restrict__ old_lp,
                                                         float* __restrict__ ratio_out, float* __restrict__ dL,
                                                         float* __restrict__ pi_out, float* __restrict__ part) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t tr = (int64_t)blockIdx.x * 4 + wv;
  const int A = d.A, n = d.n;
  const int64_t RT = d.RT();
  __shared__ float red[4][6];
  float s_loss = 0.0f, s_m = 0.0f, s_adv = 0.0f, s_pmax = 0.0f, s_ent = 0.0f, s_cut = 0.0f;
  if (tr < RT) {
    const int t = (int)fdiv((uint32_t)tr, d.dR), r = (int)(tr - (int64_t)t * d.R);
    const int b = (int)fdiv((uint32_t)r, d.dN), ag = r - b * n;
    const int64_t slot = rp.ep(b) * d.t_stride + t;
    const bool on = lane < A;
    const int av = on ? rp.avail[(slot * n + ag) * A + lane] : 0;
    float l = on ? logits[tr * A + lane] : -INFINITY;
    if (mbs && on && !av) l = -1e10f;
    const float mx = wave_max(l);
    const float ex = on ? expf(l - mx) : 0.0f;
    const float p = ex / wave_sum(ex);
    const float m = coma_mask(rp, slot, t);
    const bool live = m != 0.0f;
    const int at = min(max((int)rp.actions[slot * n + ag], 0), A - 1);   // clamped before it selects a lane
    const float pe = on ? (live ? p : 1.0f) : 0.0f;
    const float lg = on ? logf(pe + 1e-10f) : 0.0f;
    const float ent = -wave_sum(pe * lg);
    const float lp_u = __shfl(lg, at, 64);
    const float adv = td[tr];
    const float pmax = wave_max(on ? pe : -INFINITY);
    const float lp_old = FIRST ? lp_u : old_lp[tr];
    const float ratio = expf(lp_u - lp_old);
    const float s1 = ratio * adv, s2 = fminf(fmaxf(ratio, lo), hi) * adv;
    const bool keep = (ratio >= lo && ratio <= hi) || s1 < s2;
    const float c = ((keep ? 1.0f : 0.0f) * ratio) * adv;
    s_loss = -((fminf(s1, s2) + ec * ent) * m); s_m = m; s_adv = adv * m; s_pmax = pmax * m; s_ent = ent * m;
    s_cut = (live && !keep) ? 1.0f : 0.0f;
    float g = 0.0f;
    if (live && on) {
      const float den = p + 1e-10f;
      g = -m * ((lane == at ? c / den : 0.0f) - ec * (lg + p / den));
    }
    const float dot = wave_sum(on ? p * g : 0.0f);
    float dl = on ? p * (g - dot) : 0.0f;
    if (!live || (mbs && !av)) dl = 0.0f;
    if (lane < Ap) dL[tr * Ap + lane] = dl;
    if (on) pi_out[tr * A + lane] = p;
    if (lane == 0) {
      if (FIRST) old_lp[tr] = lp_u;
      ratio_out[tr] = ratio;
    }
  }
  if (lane == 0) {
    red[wv][0] = s_loss; red[wv][1] = s_m; red[wv][2] = s_adv; red[wv][3] = s_pmax; red[wv][4] = s_ent;
    red[wv][5] = s_cut;
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int k = threadIdx.x;
    part[(int64_t)blockIdx.x * 8 + k] = k < 6 ? ((red[0][k] + red[1][k]) + (red[2][k] + red[3][k])) : 0.0f;
  }
}

// One wave after both applies of an epoch: row[0..MA_NSTATS) = stats (what the two applies wrote, or the gate's zeros
// after an empty batch), with the count of live rows whose gradient was cut (asums[PPO_SUM_CLIPPED], an integer-valued
// float below 2^24) at row[PPO_STAT_CLIPPED]; the count is zero when the halt word is set.
__global__ __launch_bounds__(64) void ppo_stats_kernel(const float* __restrict__ stats, const float* __restrict__ asums,
                                                       const int* __restrict__ halt, float* __restrict__ row) {
  const int i = threadIdx.x;
  if (blockIdx.x != 0 || i >= MA_NSTATS) return;
  row[i] = i == PPO_STAT_CLIPPED ? (*halt != 0 ? 0.0f : asums[PPO_SUM_CLIPPED]) : stats[i];
}

}  // namespace mq
