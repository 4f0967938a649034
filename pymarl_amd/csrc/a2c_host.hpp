// Host side of the actor-critic learner step (include/ma_a2c.h). As the COMA learner it keeps an
// internal mq_handle (no mixer) for the agent's workspace and kernels and shares the actor's forward and backward with
// it (coma_host.hpp actor_forward / actor_backward, launched from a2c_plan's ActorPlan); the critic has its own
// workspace, sized once at ma_create from max_batch / max_seq.
#pragma once
#include <cmath>

#include "../../include/ma_a2c.h"
#include "a2c_kernels.hpp"
#include "coma_host.hpp"
#include "optim_host.hpp"
#include "ppo_kernels.hpp"

struct ma_handle {
  ma_config cfg;
  mq_handle* ah = nullptr;   // agent workspace + kernels
  int K, Kp, Hc, Ap;
  int64_t aoff[MQ_P_COUNT + 1];
  int64_t coff[MA_P_COUNT + 1];
  int64_t Pa, Pc;
  float *agent = nullptr, *agrad = nullptr, *asq = nullptr, *critic = nullptr, *tcritic = nullptr, *cgrad = nullptr,
        *csq = nullptr, *stats = nullptr;
  DevBuf<float> ws;     // one allocation, carved by ma_create's table
  DevBuf<float> gpow;   // [q_nstep + 2] float32(gamma ** k)
  // critic workspace
  float *X, *H1t, *H2t, *H1o, *H2o, *Vt, *Vo, *RS, *ret, *td, *dH2, *dH1, *slab_w3, *cpart, *slab_w2, *slab_w1,
      *cred_tmp, *cnorm_part;
  int* halt;
  // actor workspace
  float *dL, *dHo, *pi, *ppart, *slab_fc2, *red_tmp, *norm_part;
  float *old_lp, *ratio;   // [T R] each, PPO: epoch 0's log-probabilities of the taken actions, the last epoch's ratio
  float* gbak;   // [Pa + MQ_NSUMS | Pc + MA_NTAIL] both gradient buffers before the reductions (a2c_gate_kernel)
  double* rbak;  // [3] the running reward statistics before reward_norm_kernel merged the batch into them
  int ns_max = 1, ndv_max = 1;   // slabs the workspace holds
  bool adam = false;
  ma_adam ad{};
  double* rew_state = nullptr;
  bool ppo = false;   // ma_set_ppo: ma_train_step runs pp.epochs epochs (ppo_host.hpp)
  ma_ppo pp{};
  ma_plan last{};
  int last_T = 0, last_R = 0;

  ~ma_handle() { mq_destroy(ah); }   // the buffers free themselves
};

namespace {

int ma_check_config(const ma_config& c, bool train) {
  if (c.critic_type != MA_CRITIC_CV && c.critic_type != MA_CRITIC_AC)
    return set_err(MQ_ERR_ARG, "critic_type " + std::to_string(c.critic_type) + " not recognised.");
  if (c.critic_hidden != 64 && c.critic_hidden != 128) return set_err(MQ_ERR_ARG, "critic hidden_dim must be 64 or 128");
  if (c.n_agents < 1 || c.n_agents > 64) return set_err(MQ_ERR_ARG, "n_agents must be in [1, 64]");
  if (c.n_actions < 1 || c.n_actions > 64) return set_err(MQ_ERR_ARG, "n_actions must be in [1, 64]");
  if (c.obs_dim < 1 || c.state_dim < 1) return set_err(MQ_ERR_ARG, "obs_dim / state_dim must be positive");
  if (!train) return MQ_OK;
  if (c.q_nstep < 1) return set_err(MQ_ERR_ARG, "q_nstep must be >= 1");
  if (!(c.entropy_coef >= 0.0f)) return set_err(MQ_ERR_ARG, "entropy_coef must be >= 0");
  if (!c.gamma_pow) return set_err(MQ_ERR_ARG, "ma_config.gamma_pow is NULL");
  if (a2c_nstep_lds_bytes(c.max_seq, c.n_agents) > kA2cNstepLdsMax)
    return set_err(MQ_ERR_ARG, "max_seq " + std::to_string(c.max_seq) + " needs more than " +
                                   std::to_string(kA2cNstepLdsMax) + " B of LDS for the n-step return pass");
  return MQ_OK;
}

ADims ma_dims(const ma_config& c, int B, int t_len, int t_stride) {
  ADims d{};
  d.n = c.n_agents; d.A = c.n_actions; d.O = c.obs_dim; d.S = c.state_dim;
  d.K = a2c_k(c); d.Kp = (d.K + 3) & ~3; d.Hc = c.critic_hidden;
  d.B = B; d.R = B * c.n_agents; d.Tp = t_len; d.T = t_len - 1; d.t_stride = t_stride;
  d.kind = c.critic_type; d.last_action = c.obs_last_action;
  d.dR = make_fastdiv((uint32_t)d.R);
  d.dN = make_fastdiv((uint32_t)d.n);
  return d;
}

void ma_offsets(const ma_config& c, int64_t* off) {
  const int64_t Hc = c.critic_hidden, K = a2c_k(c);
  const int64_t sz[MA_P_COUNT] = {Hc * K, Hc, Hc * Hc, Hc, Hc, 1};
  int64_t o = 0;
  for (int i = 0; i < MA_P_COUNT; ++i) { off[i] = o; o += sz[i]; }
  off[MA_P_COUNT] = o;
}

int ma_check_replay(const ma_config& c, const mq_replay* b, const char* who) {
  if (c.critic_type == MA_CRITIC_CV && !b->state) return set_err(MQ_ERR_ARG, std::string(who) + ": cv_critic needs batch.state");
  if (c.critic_type == MA_CRITIC_AC && !b->obs) return set_err(MQ_ERR_ARG, std::string(who) + ": ac_critic needs batch.obs");
  if (!b->actions || !b->filled) return set_err(MQ_ERR_ARG, std::string(who) + ": batch needs actions and filled");
  return MQ_OK;
}

// One optimiser step over a flat buffer with its [sums] tail behind the gradient: Adam (exp_avg given) or RMSprop.
int ma_apply(const ma_handle* h, float* p, float* g, float* m, float* v, int64_t n, const float* part, int npart,
             int64_t adam_step, float* stats, hipStream_t s) {
  const ma_config& c = h->cfg;
  if (m) {
    const AdamHP hp = make_adam_hp(c.lr, h->ad.beta1, h->ad.beta2, h->ad.eps, h->ad.weight_decay, adam_step,
                                   c.grad_norm_clip, 1);
    hipLaunchKernelGGL(apply_adam_kernel, dim3(vec4_blocks({p, g, m, v}, n)), dim3(256), 0, s, p, g, m, v, n, part,
                       npart, hp, stats, (const int*)h->halt);
  } else {
    const OptHP hp{c.lr, c.optim_alpha, c.optim_eps, c.grad_norm_clip, 1};
    hipLaunchKernelGGL(apply_kernel, dim3((int)std::min<int64_t>((n + 255) / 256, 1024)), dim3(256), 0, s, p, g, v, n,
                       part, npart, hp, stats, (const int*)h->halt);
  }
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

// The critic's backward GEMMs: dH1, then the split-K [dW2 | db2] and [dW1 | db1] slabs.
int ma_critic_dw(const ma_handle* h, const ma_plan& pl, int64_t RT, hipStream_t s) {
  const int Hc = h->Hc;
  const float* oc = h->critic;
  {
    A2cDh1Prob p{h->dH2, oc + h->coff[MA_P_FC2_W], h->H1o, h->dH1, RT, Hc};
    MQ_HIP(launch_gemm(p, (int)RT, Hc, 1, s));
  }
  {
    A2cDwProb<64> p{h->dH2, Hc, h->H1o, Hc, Hc, h->slab_w2, RT, pl.ns_cw2};
    MQ_HIP(launch_gemm(p, Hc, Hc, pl.ns_cw2, s));
  }
  {
    A2cDwProb<128> p{h->dH1, Hc, h->X, h->Kp, h->K, h->slab_w1, RT, pl.ns_cw1};
    MQ_HIP(launch_gemm(p, Hc, h->K, pl.ns_cw1, s));
  }
  return MQ_OK;
}

// The two-pass reduction of the critic's slabs and loss sums into cgrad [Pc | MA_NTAIL]; *nnorm = the norm partials
// it left in cnorm_part.
int ma_critic_reduce(const ma_handle* h, const ma_plan& pl, hipStream_t s, int* nnorm) {
  const int Hc = h->Hc;
  RedBuilder rb(h->cred_tmp);
  rb.add(h->slab_w1, pl.ns_cw1, (int64_t)Hc * h->K + Hc, h->cgrad + h->coff[MA_P_FC1_W], true);
  rb.add(h->slab_w2, pl.ns_cw2, (int64_t)Hc * Hc + Hc, h->cgrad + h->coff[MA_P_FC2_W], true);
  rb.add(h->slab_w3, pl.dv_blocks, Hc + 1, h->cgrad + h->coff[MA_P_FC3_W], true);
  rb.add(h->cpart, pl.dv_blocks, MA_NTAIL, h->cgrad + h->Pc, false);
  return launch_reduce(rb, h->cnorm_part, "critic", s, nnorm);
}

// fc1 and fc2 of one critic net with parameters P over `rows` rows of X, one CLinProbT launch per layer (A2cLin2's tile
// code: bitwise what the two-net launch gives).
int ma_critic_l12(const float* P, const int64_t* off, const ADims& d, const float* X, float* H1, float* H2, int64_t rows,
                  hipStream_t s) {
  const CLinProbT<64> l1 =
      CLinProbT<64>{X, d.Kp, P + off[MA_P_FC1_W], P + off[MA_P_FC1_B], H1, rows, d.Hc, d.K, 1}.with_vec();
  MQ_HIP(launch_gemm(l1, (int)rows, d.Hc, 1, s));
  const CLinProbT<64> l2 =
      CLinProbT<64>{H1, d.Hc, P + off[MA_P_FC2_W], P + off[MA_P_FC2_B], H2, rows, d.Hc, d.Hc, 1}.with_vec();
  MQ_HIP(launch_gemm(l2, (int)rows, d.Hc, 1, s));
  return MQ_OK;
}

// The returns: the rewards standardised first when asked for (reward[:, :T], all B T values; the statistics as they
// were go to rbak, since an empty batch puts them back and so merges nothing into them), then the n-step pass.
int ma_returns(const ma_handle* h, const ADims& cd, const Rep& rp, const ma_plan& pl, hipStream_t s) {
  const ma_config& c = h->cfg;
  if (h->rew_state) {
    MQ_HIP(hipMemcpyAsync(h->rbak, h->rew_state, 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
    const Dims dr = mq::make_dims(h->ah->cfg, cd.B, cd.Tp, cd.t_stride);   // dr.T = T, dr.M = T B
    hipLaunchKernelGGL(reward_norm_kernel, dim3(1), dim3(RN_THREADS), 0, s, dr, rp, h->rew_state, h->RS);
    MQ_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(a2c_nstep_kernel, dim3(cd.B), dim3(256), pl.nstep_lds, s, cd, rp, (const float*)h->Vt,
                     (const float*)(h->rew_state ? h->RS : nullptr), (const float*)h->gpow, (int)c.q_nstep,
                     (int)(c.add_value_last_step != 0), h->ret);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

// The step's plan and its actor's, checked against what ma_create allocated (max_batch / max_seq bound the slabs, and
// PPO's old_lp and ratio) and against the n-step pass's LDS.
int ma_step_plan(const ma_handle* h, int B, int Tp, ma_plan* pl, ActorPlan* ap) {
  *pl = a2c_plan(h->cfg, B, Tp, h->rew_state != nullptr, h->adam, ap);
  if (pl->ns_cw1 > h->ns_max || pl->ns_cw2 > h->ns_max || pl->dv_blocks > h->ndv_max || ap->ns_w2 > kNsplitMax)
    return set_err(MQ_ERR_STATE, "actor-critic plan exceeds the workspace");
  if (a2c_nstep_lds_bytes(Tp, h->cfg.n_agents) > kA2cNstepLdsMax)
    return set_err(MQ_ERR_ARG, "episode too long for the LDS n-step return pass");
  return MQ_OK;
}

// Both applies after both backwards; an empty batch (M = 0) halts both (a2c_gate_kernel).
int ma_gate_apply(const ma_handle* h, int nnorm_c, int nnorm_a, int64_t adam_step, hipStream_t s) {
  const int64_t na = h->Pa + MQ_NSUMS, nc = h->Pc + MA_NTAIL;
  hipLaunchKernelGGL(a2c_gate_kernel, dim3(1), dim3(A2C_GATE_THREADS), 0, s, (const float*)(h->cgrad + h->Pc), h->halt,
                     h->stats, (const float*)h->gbak, h->agrad, na, h->cgrad, nc, h->rew_state,
                     (const double*)h->rbak);
  MQ_HIP(hipGetLastError());
  int rc;
  if ((rc = ma_apply(h, h->critic, h->cgrad, h->adam ? h->ad.critic_exp_avg : nullptr, h->csq, h->Pc, h->cnorm_part,
                     nnorm_c, adam_step, h->stats, s)) ||
      (rc = ma_apply(h, h->agent, h->agrad, h->adam ? h->ad.agent_exp_avg : nullptr, h->asq, h->Pa, h->norm_part,
                     nnorm_a, adam_step, h->stats + 8, s)))
    return rc;
  return MQ_OK;
}

// ma_train_step after ma_set_ppo (ppo_host.hpp).
int ma_ppo_train(ma_handle* h, const mq_replay* batch, int64_t adam_step, hipStream_t s);

}  // namespace

extern "C" {

int64_t ma_critic_forward_workspace(const ma_config* cfg, int32_t batch_size, int32_t t_count) {
  if (!cfg || batch_size < 1 || t_count < 1) return -1;
  const int64_t Kp = (a2c_k(*cfg) + 3) & ~3;
  const int64_t M = (int64_t)t_count * batch_size * cfg->n_agents;
  return align_up(M * Kp) + 2 * align_up(M * cfg->critic_hidden);
}

int ma_critic_forward(const float* critic, const ma_config* cfg, const mq_replay* batch, int32_t t, float* v_out,
                      float* workspace, void* stream) {
  if (!critic || !cfg || !batch || !v_out || !workspace) return set_err(MQ_ERR_ARG, "ma_critic_forward: NULL pointer");
  int rc = ma_check_config(*cfg, false);
  if (rc || (rc = ma_check_replay(*cfg, batch, "ma_critic_forward"))) return rc;
  if (batch->batch_size < 1 || batch->t_len < 1 || batch->t_len > batch->t_stride)
    return set_err(MQ_ERR_ARG, "ma_critic_forward: bad batch dimensions");
  if (t >= batch->t_len) return set_err(MQ_ERR_ARG, "ma_critic_forward: t outside the batch");
  if ((int64_t)batch->t_len * batch->batch_size * cfg->n_agents >= (1LL << 31))
    return set_err(MQ_ERR_ARG, "ma_critic_forward: batch too large for 32-bit row indices");
  if ((rc = check_ids(batch))) return rc;
  if (batch->ep_ids_host && batch->batch_size > MQ_INLINE_IDS && !batch->ep_ids)
    return set_err(MQ_ERR_ARG, "ma_critic_forward: more than MQ_INLINE_IDS episodes need device ids");
  hipStream_t s = (hipStream_t)stream;
  const int Tq = t < 0 ? batch->t_len : 1, t0 = t < 0 ? 0 : t;
  const ADims d = ma_dims(*cfg, batch->batch_size, batch->t_len, batch->t_stride);
  const Rep rp = make_rep(batch);
  const int64_t M = (int64_t)Tq * d.R;
  const int Hc = d.Hc;
  float* X = workspace;
  float* H1 = X + align_up(M * d.Kp);
  float* H2 = H1 + align_up(M * Hc);
  int64_t off[MA_P_COUNT + 1];
  ma_offsets(*cfg, off);
  hipLaunchKernelGGL(a2c_xin_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, d, rp, X, t0, M);
  MQ_HIP(hipGetLastError());
  if ((rc = ma_critic_l12(critic, off, d, X, H1, H2, M, s))) return rc;
  hipLaunchKernelGGL(a2c_vhead_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, (const float*)H2,
                     (const float*)nullptr, critic, critic, off[MA_P_FC3_W], off[MA_P_FC3_B], Hc, M, (int64_t)0, v_out,
                     (float*)nullptr, d.R, d.n, Tq);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int ma_create(const ma_config* cfg, ma_handle** out) {
  if (!cfg || !out) return set_err(MQ_ERR_ARG, "NULL argument");
  const ma_config& c = *cfg;
  int rc = ma_check_config(c, true);
  if (rc) return rc;
  if (c.max_batch * c.n_agents > MQ_INLINE_IDS * 64) return set_err(MQ_ERR_ARG, "max_batch * n_agents too large");
  const mq_config ac = agent_config(c, c.gamma_pow[1]);   // (ma_check_config: gamma_pow is not NULL)
  mq_handle* ah = nullptr;
  if ((rc = mq_create(&ac, &ah))) return rc;
  std::unique_ptr<ma_handle> h(new ma_handle());   // owns ah from here: a failure below frees both
  h->cfg = c;
  h->cfg.gamma_pow = nullptr;   // the caller's table is copied below and not kept
  h->ah = ah;
  for (int i = 0; i <= MQ_P_COUNT; ++i) h->aoff[i] = ah->off[i];
  h->Pa = ah->P;
  const int n = c.n_agents, A = c.n_actions, Hc = c.critic_hidden;
  h->K = a2c_k(c);
  h->Kp = (h->K + 3) & ~3;
  h->Hc = Hc;
  h->Ap = (A + 3) & ~3;
  ma_offsets(c, h->coff);
  h->Pc = h->coff[MA_P_COUNT];

  const int64_t Tp = c.max_seq, R = (int64_t)c.max_batch * n, T = Tp - 1, RT = T * R;
  h->ns_max = a2c_ns_max(RT);
  h->ndv_max = (int)((RT + A2C_DV_ROWS - 1) / A2C_DV_ROWS);
  const int64_t lw1 = (int64_t)Hc * h->K + Hc, lw2 = (int64_t)Hc * Hc + Hc, lw3 = Hc + 1;
  const int64_t cred_tmp = kRedZ * (lw1 + lw2 + lw3 + 8);
  const int64_t red_tmp = kRedZ * ((int64_t)mq::H * ah->I + mq::H) + kRedZ * ah->len_rnn + kRedZ * (A * mq::H + A) +
                          kRedZ * 8;
  float* rbak_f = nullptr;
  const WsTable ws = {
      {"X", Tp * R * h->Kp, &h->X},
      {"H1t", Tp * R * Hc, &h->H1t}, {"H2t", Tp * R * Hc, &h->H2t},
      {"H1o", RT * Hc, &h->H1o}, {"H2o", RT * Hc, &h->H2o},
      {"Vt", Tp * R, &h->Vt}, {"Vo", RT, &h->Vo},
      {"RS", Tp * c.max_batch, &h->RS},
      {"ret", RT, &h->ret}, {"td", RT, &h->td},
      {"dH2", RT * Hc, &h->dH2}, {"dH1", RT * Hc, &h->dH1},
      {"slab_w3", h->ndv_max * lw3, &h->slab_w3}, {"cpart", (int64_t)h->ndv_max * 8, &h->cpart},
      {"slab_w2", h->ns_max * lw2, &h->slab_w2}, {"slab_w1", h->ns_max * lw1, &h->slab_w1},
      {"cred_tmp", cred_tmp, &h->cred_tmp}, {"cnorm_part", kNormPartMax, &h->cnorm_part},
      {"halt", 8, nullptr, &h->halt},
      {"dL", RT * h->Ap, &h->dL}, {"dHo", RT * mq::H, &h->dHo}, {"pi", RT * A, &h->pi},
      {"ppart", ((RT + 3) / 4) * 8, &h->ppart},
      {"slab_fc2", (int64_t)kNsplitMax * (A * mq::H + A), &h->slab_fc2},
      {"red_tmp", red_tmp, &h->red_tmp},
      {"norm_part", kNormPartMax, &h->norm_part},
      {"old_lp", RT, &h->old_lp}, {"ratio", RT, &h->ratio},
      {"gbak", h->Pa + MQ_NSUMS + h->Pc + MA_NTAIL, &h->gbak},
      {"rbak", 8, &rbak_f},   // three doubles (every row starts at a multiple of 64 floats: 8-byte aligned)
  };
  if ((rc = ws_carve(h->ws, ws, "actor-critic workspace hipMalloc"))) return rc;
  h->rbak = (double*)rbak_f;
  const int64_t ng = (int64_t)c.q_nstep + 2;
  if ((rc = h->gpow.alloc(ng, "n-step discount table hipMalloc"))) return rc;
  MQ_HIP(hipMemcpy(h->gpow, c.gamma_pow, (size_t)ng * sizeof(float), hipMemcpyHostToDevice));
  *out = h.release();
  return MQ_OK;
}

int ma_destroy(ma_handle* h) {
  delete h;
  return MQ_OK;
}

int ma_param_offsets(const ma_handle* h, int64_t* agent_offsets, int64_t* critic_offsets) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  if (agent_offsets)
    for (int i = 0; i <= MQ_P_COUNT; ++i) agent_offsets[i] = h->aoff[i];
  if (critic_offsets)
    for (int i = 0; i <= MA_P_COUNT; ++i) critic_offsets[i] = h->coff[i];
  return MQ_OK;
}

int ma_bind(ma_handle* h, float* agent, float* agent_grad, float* agent_sq, float* critic, float* target_critic,
            float* critic_grad, float* critic_sq, float* stats) {
  if (!h || !agent || !agent_grad || !agent_sq || !critic || !target_critic || !critic_grad || !critic_sq || !stats)
    return set_err(MQ_ERR_ARG, "ma_bind: NULL pointer");
  h->agent = agent; h->agrad = agent_grad; h->asq = agent_sq; h->critic = critic; h->tcritic = target_critic;
  h->cgrad = critic_grad; h->csq = critic_sq; h->stats = stats;
  // the agent handle: online = target = the agent params (the actor has no target net); its stats land at stats + 8
  return mq_bind(h->ah, agent, agent, agent_grad, agent_sq, stats + 8, nullptr);
}

int ma_set_adam(ma_handle* h, const ma_adam* a) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  if (!a) {   // back to RMSprop
    h->adam = false;
    h->ad = ma_adam{};
    return MQ_OK;
  }
  if (!a->agent_exp_avg || !a->critic_exp_avg) return set_err(MQ_ERR_ARG, "ma_set_adam: an exp_avg pointer is NULL");
  if (((uintptr_t)a->agent_exp_avg | (uintptr_t)a->critic_exp_avg) & 3)
    return set_err(MQ_ERR_ARG, "ma_set_adam: exp_avg is not aligned to a float");
  const int rc = check_adam("ma_set_adam", a->beta1, a->beta2, a->eps, a->weight_decay);
  if (rc) return rc;
  h->ad = *a;
  h->adam = true;
  return MQ_OK;
}

int ma_set_reward_norm(ma_handle* h, double* state) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  if (state && ((uintptr_t)state & 7)) return set_err(MQ_ERR_ARG, "ma_set_reward_norm: state is not aligned to a double");
  h->rew_state = state;
  return MQ_OK;
}

int ma_train_step(ma_handle* h, const mq_replay* batch, int64_t adam_step, void* stream) {
  if (!h || !h->agent) return set_err(MQ_ERR_STATE, "ma_train_step before ma_bind");
  mq_handle* ah = h->ah;
  int rc = check_batch(ah, batch);
  if (rc || (rc = ma_check_replay(h->cfg, batch, "ma_train_step"))) return rc;
  if (h->adam && adam_step < 1) return set_err(MQ_ERR_ARG, "ma_train_step: adam_step is the 1-based step number (>= 1)");
  hipStream_t s = (hipStream_t)stream;
  if (h->ppo) return ma_ppo_train(h, batch, adam_step, s);
  const ma_config& c = h->cfg;
  const int n = c.n_agents, Hc = h->Hc;
  const int B = batch->batch_size, Tp = batch->t_len, T = Tp - 1, R = B * n;
  const Rep rp = make_rep(batch);
  const ADims cd = ma_dims(c, B, Tp, batch->t_stride);
  ma_plan pl;
  ActorPlan ap;
  if ((rc = ma_step_plan(h, B, Tp, &pl, &ap))) return rc;
  pl.epochs = 1;
  const int64_t RT = (int64_t)T * R, RTp = (int64_t)Tp * R;

  // ---- critic forward: inputs, fc1 / fc2 of both nets (grid.z: 0 target over t <= T, 1 online over t < T), fc3
  hipLaunchKernelGGL(a2c_xin_kernel, dim3((unsigned)((RTp + 3) / 4)), dim3(256), 0, s, cd, rp, h->X, 0, RTp);
  MQ_HIP(hipGetLastError());
  const float *tc = h->tcritic, *oc = h->critic;
  {
    A2cLin2<64> p;
    p.net[0] = CLinProbT<64>{h->X, h->Kp, tc + h->coff[MA_P_FC1_W], tc + h->coff[MA_P_FC1_B], h->H1t, RTp, Hc, h->K, 1}
                   .with_vec();
    p.net[1] = CLinProbT<64>{h->X, h->Kp, oc + h->coff[MA_P_FC1_W], oc + h->coff[MA_P_FC1_B], h->H1o, RT, Hc, h->K, 1}
                   .with_vec();
    MQ_HIP(launch_gemm(p, (int)RTp, Hc, 2, s));
  }
  {
    A2cLin2<64> p;
    p.net[0] = CLinProbT<64>{h->H1t, Hc, tc + h->coff[MA_P_FC2_W], tc + h->coff[MA_P_FC2_B], h->H2t, RTp, Hc, Hc, 1}
                   .with_vec();
    p.net[1] = CLinProbT<64>{h->H1o, Hc, oc + h->coff[MA_P_FC2_W], oc + h->coff[MA_P_FC2_B], h->H2o, RT, Hc, Hc, 1}
                   .with_vec();
    MQ_HIP(launch_gemm(p, (int)RTp, Hc, 2, s));
  }
  hipLaunchKernelGGL(a2c_vhead_kernel, dim3(pl.vhead_blocks), dim3(256), 0, s, (const float*)h->H2t,
                     (const float*)h->H2o, tc, oc, h->coff[MA_P_FC3_W], h->coff[MA_P_FC3_B], Hc, RTp, RT, h->Vt, h->Vo, R,
                     n, 0);
  MQ_HIP(hipGetLastError());
  // ---- the agent's dims: the actor unrolls t < T only
  const Dims d = mq::make_dims(ah->cfg, B, T, batch->t_stride);   // d.Tp = T: d.RT() = T R
  if ((rc = ma_returns(h, cd, rp, pl, s))) return rc;
  hipLaunchKernelGGL(a2c_dv_kernel, dim3(pl.dv_blocks), dim3(256), 0, s, cd, rp, (const float*)h->ret,
                     (const float*)h->Vo, (const float*)h->H2o, oc + h->coff[MA_P_FC3_W], h->td, h->dH2, h->slab_w3,
                     h->cpart);
  MQ_HIP(hipGetLastError());
  // ---- actor forward and policy (reads the critic's td as the advantage)
  const Lay L = make_lay(ah);
  Work w = ah->w;
  w.dHo = h->dHo;
  if ((rc = actor_forward(h, ap, d, rp, L, w, RT, s))) return rc;
  hipLaunchKernelGGL(a2c_policy_kernel, dim3(pl.policy_blocks), dim3(256), 0, s, d, rp, (const float*)w.Q,
                     (const float*)h->td, c.entropy_coef, (int)(c.mask_before_softmax != 0), h->Ap, h->dL, h->pi,
                     h->ppart);
  MQ_HIP(hipGetLastError());
  // ---- critic backward: dH1, the split-K weight gradients, the two-pass reduction into cgrad [Pc | MA_NTAIL]
  if ((rc = ma_critic_dw(h, pl, RT, s))) return rc;
  // both gradient buffers as the caller left them: an empty batch puts them back (a2c_gate_kernel)
  const int64_t na = h->Pa + MQ_NSUMS, nc = h->Pc + MA_NTAIL;
  MQ_HIP(hipMemcpyAsync(h->gbak, h->agrad, (size_t)na * sizeof(float), hipMemcpyDeviceToDevice, s));
  MQ_HIP(hipMemcpyAsync(h->gbak + na, h->cgrad, (size_t)nc * sizeof(float), hipMemcpyDeviceToDevice, s));
  int nnorm_c;
  if ((rc = ma_critic_reduce(h, pl, s, &nnorm_c))) return rc;
  // ---- actor backward (the COMA learner's chain)
  int nnorm_a;
  if ((rc = actor_backward(h, ap, d, rp, L, w, RT, pl.policy_blocks, s, &nnorm_a))) return rc;
  // ---- both applies after both backwards; an empty batch (M = 0) halts both
  if ((rc = ma_gate_apply(h, nnorm_c, nnorm_a, adam_step, s))) return rc;
  h->last = pl;
  h->last_T = T;
  h->last_R = R;
  return MQ_OK;
}

int ma_update_targets(ma_handle* h, double tau, void* stream) {
  if (!h || !h->critic) return set_err(MQ_ERR_STATE, "ma_update_targets before ma_bind");
  if (!(tau >= 0.0)) return set_err(MQ_ERR_ARG, "ma_update_targets: tau must be >= 0");
  hipStream_t s = (hipStream_t)stream;
  if (tau == 0.0 || tau >= 1.0) {
    MQ_HIP(hipMemcpyAsync(h->tcritic, h->critic, h->Pc * sizeof(float), hipMemcpyDeviceToDevice, s));
    return MQ_OK;
  }
  hipLaunchKernelGGL(soft_update_kernel, dim3(vec4_blocks({h->tcritic, h->critic}, h->Pc)), dim3(256), 0, s,
                     h->tcritic, (const float*)h->critic, h->Pc, (float)(1.0 - tau), (float)tau, (const int*)nullptr);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int ma_copy_intermediate(ma_handle* h, int which, float* dst, int64_t* count, void* stream) {
  if (!h || h->last_T <= 0) return set_err(MQ_ERR_STATE, "no actor-critic train step has run");
  const int64_t TR = (int64_t)h->last_T * h->last_R;
  const float* src;
  int64_t cnt;
  switch (which) {
    case 0: src = h->Vt; cnt = TR + h->last_R; break;
    case 1: src = h->Vo; cnt = TR; break;
    case 2: src = h->ret; cnt = TR; break;
    case 3: src = h->pi; cnt = TR * h->cfg.n_actions; break;
    case 4: src = h->dL; cnt = TR * h->Ap; break;
    case 5: case 6:
      if (h->last.hoisted < 1) return set_err(MQ_ERR_STATE, "the last train step was not a PPO step");
      src = which == 5 ? h->old_lp : h->ratio; cnt = TR; break;
    default: return set_err(MQ_ERR_ARG, "unknown actor-critic intermediate id");
  }
  if (count) *count = cnt;
  if (dst) MQ_HIP(hipMemcpyAsync(dst, src, cnt * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MQ_OK;
}

int ma_last_plan(const ma_handle* h, ma_plan* out) {
  if (!h || !out) return set_err(MQ_ERR_ARG, "NULL argument");
  if (h->last_T <= 0) return set_err(MQ_ERR_STATE, "no actor-critic train step has run");
  *out = h->last;
  return MQ_OK;
}

}  // extern "C"
