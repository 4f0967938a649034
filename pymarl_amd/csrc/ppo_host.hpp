// Host side of the PPO step (include/ma_a2c.h ma_set_ppo): ma_train_step as E epochs over one batch,
// in one launch sequence. What does not change between the epochs is launched once: the critic inputs X, the target
// critic's V', the standardised rewards, the n-step returns, and the copies an empty batch puts back. An epoch is the
// actor-critic step's remainder (a2c_host.hpp) with ppo_policy_kernel in a2c_policy_kernel's place and the online
// critic's forward as one CLinProbT launch per layer: A2cLin2's tile code, so V is bitwise what that launch gives.
#pragma once
#include "a2c_host.hpp"

namespace {

int ma_ppo_train(ma_handle* h, const mq_replay* batch, int64_t adam_step, hipStream_t s) {
  mq_handle* ah = h->ah;
  const ma_config& c = h->cfg;
  const int n = c.n_agents, Hc = h->Hc, E = h->pp.epochs;
  const int B = batch->batch_size, Tp = batch->t_len, T = Tp - 1, R = B * n;
  const Rep rp = make_rep(batch);
  const ADims cd = ma_dims(c, B, Tp, batch->t_stride);
  ma_plan pl;
  ActorPlan ap;
  int rc, hoisted = 0;
  if ((rc = ma_step_plan(h, B, Tp, &pl, &ap))) return rc;
  const int64_t RT = (int64_t)T * R, RTp = (int64_t)Tp * R;
  const float lo = (float)(1.0 - (double)h->pp.eps_clip), hi = (float)(1.0 + (double)h->pp.eps_clip);

  // ---- once per train(): X, the target critic's fc1 / fc2 / V head over t <= T
  hipLaunchKernelGGL(a2c_xin_kernel, dim3((unsigned)((RTp + 3) / 4)), dim3(256), 0, s, cd, rp, h->X, 0, RTp);
  MQ_HIP(hipGetLastError());
  const float *tc = h->tcritic, *oc = h->critic;
  if ((rc = ma_critic_l12(tc, h->coff, cd, h->X, h->H1t, h->H2t, RTp, s))) return rc;
  hipLaunchKernelGGL(a2c_vhead_kernel, dim3((unsigned)((RTp + 3) / 4)), dim3(256), 0, s, (const float*)h->H2t,
                     (const float*)nullptr, tc, oc, h->coff[MA_P_FC3_W], h->coff[MA_P_FC3_B], Hc, RTp, (int64_t)0, h->Vt,
                     (float*)nullptr, R, n, 0);
  MQ_HIP(hipGetLastError());
  hoisted += 4;
  const Dims d = mq::make_dims(ah->cfg, B, T, batch->t_stride);   // d.Tp = T: d.RT() = T R
  // ---- once: the rewards standardised (the running statistics merge the batch once), the n-step returns
  if ((rc = ma_returns(h, cd, rp, pl, s))) return rc;
  hoisted += h->rew_state ? 2 : 0;
  // ---- once: both gradient buffers as the caller left them (an empty batch puts them back after every epoch)
  const int64_t na = h->Pa + MQ_NSUMS, nc = h->Pc + MA_NTAIL;
  MQ_HIP(hipMemcpyAsync(h->gbak, h->agrad, (size_t)na * sizeof(float), hipMemcpyDeviceToDevice, s));
  MQ_HIP(hipMemcpyAsync(h->gbak + na, h->cgrad, (size_t)nc * sizeof(float), hipMemcpyDeviceToDevice, s));
  hoisted += 3;

  const Lay L = make_lay(ah);
  Work w = ah->w;
  w.dHo = h->dHo;
  const int mbs = (int)(c.mask_before_softmax != 0);
  for (int k = 0; k < E; ++k) {
    // ---- critic: V of the current parameters over t < T, td against the fixed returns
    if ((rc = ma_critic_l12(oc, h->coff, cd, h->X, h->H1o, h->H2o, RT, s))) return rc;
    hipLaunchKernelGGL(a2c_vhead_kernel, dim3((unsigned)((RT + 3) / 4)), dim3(256), 0, s, (const float*)nullptr,
                       (const float*)h->H2o, tc, oc, h->coff[MA_P_FC3_W], h->coff[MA_P_FC3_B], Hc, (int64_t)0, RT,
                       (float*)nullptr, h->Vo, R, n, 0);
    MQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(a2c_dv_kernel, dim3(pl.dv_blocks), dim3(256), 0, s, cd, rp, (const float*)h->ret,
                       (const float*)h->Vo, (const float*)h->H2o, oc + h->coff[MA_P_FC3_W], h->td, h->dH2, h->slab_w3,
                       h->cpart);
    MQ_HIP(hipGetLastError());
    // ---- actor forward and the clipped surrogate (epoch 0 writes the old log-probabilities)
    if ((rc = actor_forward(h, ap, d, rp, L, w, RT, s))) return rc;
    if (k == 0)
      hipLaunchKernelGGL(ppo_policy_kernel<true>, dim3(pl.policy_blocks), dim3(256), 0, s, d, rp, (const float*)w.Q,
                         (const float*)h->td, c.entropy_coef, lo, hi, mbs, h->Ap, h->old_lp, h->ratio, h->dL, h->pi,
                         h->ppart);
    else
      hipLaunchKernelGGL(ppo_policy_kernel<false>, dim3(pl.policy_blocks), dim3(256), 0, s, d, rp, (const float*)w.Q,
                         (const float*)h->td, c.entropy_coef, lo, hi, mbs, h->Ap, h->old_lp, h->ratio, h->dL, h->pi,
                         h->ppart);
    MQ_HIP(hipGetLastError());
    // ---- both backwards, then both applies (Adam step number adam_step + k), then the epoch's stats row
    int nnorm_c, nnorm_a;
    if ((rc = ma_critic_dw(h, pl, RT, s)) || (rc = ma_critic_reduce(h, pl, s, &nnorm_c)) ||
        (rc = actor_backward(h, ap, d, rp, L, w, RT, pl.policy_blocks, s, &nnorm_a)) ||
        (rc = ma_gate_apply(h, nnorm_c, nnorm_a, adam_step + k, s)))
      return rc;
    hipLaunchKernelGGL(ppo_stats_kernel, dim3(1), dim3(64), 0, s, (const float*)h->stats,
                       (const float*)(h->agrad + h->Pa), (const int*)h->halt, h->pp.epoch_stats + (int64_t)k * MA_NSTATS);
    MQ_HIP(hipGetLastError());
  }
  pl.epochs = E;
  pl.hoisted = hoisted;
  h->last = pl;
  h->last_T = T;
  h->last_R = R;
  return MQ_OK;
}

}  // namespace

extern "C" {

int ma_set_ppo(ma_handle* h, const ma_ppo* p) {
  // the arguments first and the handle after them: none of this is a HIP call
  if (p) {
    if (p->epochs < 1) return set_err(MQ_ERR_ARG, "ma_set_ppo: epochs must be >= 1");
    if (!(p->eps_clip > 0.0f && p->eps_clip < 1.0f))
      return set_err(MQ_ERR_ARG, "ma_set_ppo: eps_clip must be in (0, 1)");
    if (!p->epoch_stats) return set_err(MQ_ERR_ARG, "ma_set_ppo: epoch_stats is NULL");
    if ((uintptr_t)p->epoch_stats & 3) return set_err(MQ_ERR_ARG, "ma_set_ppo: epoch_stats is not aligned to a float");
  }
  if (!h) return set_err(MQ_ERR_ARG, "ma_set_ppo: NULL handle");
  if (!p) {   // back to the one-step actor-critic
    h->ppo = false;
    h->pp = ma_ppo{};
    return MQ_OK;
  }
  h->pp = *p;
  h->ppo = true;
  return MQ_OK;
}

}  // extern "C"
