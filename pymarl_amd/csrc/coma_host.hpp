// Host side of the COMA learner step (include/mc_coma.h). It shares the QMIX learner's error handling
// (host_util.hpp), replay plumbing (learner_handle.hpp) and agent kernels. The agent (RNNAgent) forward / BPTT reuses
// an internal mq_handle (no mixer) for its workspace; the critic has its own. What a step launches is coma_plan's
// answer (coma_plan.hpp), fixed before the first launch; ComaStep launches it phase by phase and decides nothing.
#pragma once
#include "../../include/mc_coma.h"
#include "coma_plan.hpp"
#include "gru_fwd_fused.hpp"
#include "gru_kernels.hpp"
#include "learner_handle.hpp"
#include "optim_host.hpp"

struct mc_handle {
  mc_config cfg;
  mq_handle* ah = nullptr;   // agent workspace + kernels
  int I, Kc, Kp, Ap;
  int64_t aoff[MQ_P_COUNT + 1];
  int64_t coff[MC_P_COUNT + 1];
  int64_t Pa, Pc;
  float *agent = nullptr, *agrad = nullptr, *asq = nullptr, *critic = nullptr, *tcritic = nullptr,
        *cgrad = nullptr, *csq = nullptr, *stats = nullptr;
  DevBuf<float> ws;   // one allocation, carved by mc_create's table
  // critic workspace
  float *X, *H1t, *H2t, *Qt, *tgt, *msum, *H1p, *H1c, *H2c, *dH1c, *dH2c, *dqc, *qvals, *cpart, *cnorm, *crec;
  float *Pshadow, *SQshadow;
  float* Pbak;   // [2][Pc] critic params / square_avg before the chain: restored if a hand-off times out
  int* actc;
  int* cstate;
  // actor workspace
  float *dL, *dHo, *pi, *ppart, *slab_fc2, *red_tmp, *norm_part;
  int last_T = 0, last_R = 0, last_Rc = 0;
  bool timing = false;
  // persistent critic chain (coma_chain.hpp): off with MQ_PLAN coma_chain=0, or where cc_ok rejects the shape
  bool chain_env = true;
  int num_cu = 0;
  bool chain_attr = false;
  int last_path = -1;
  DevBuf<unsigned long long> chain_trace;   // MQ_DIAG coma_trace: phase timestamps printed after each train
  // data parallel (mc_set_data_parallel)
  mc_allreduce_fn dp_fn = nullptr;
  void* dp_ctx = nullptr;
  int dp_rank = 0;
  float* dp_scratch = nullptr;
  int64_t dp_scratch_n = 0;
  std::vector<float> dp_msum;
  ncclComm_t comm = nullptr;   // mc_comm_attach: native RCCL exchange steps
  DevBuf<float> comm_scratch;   // [8 * max_seq], allocated by the first mc_comm_attach / mc_comm_use
  bool comm_owned = false;   // mc_comm_attach created it; mc_comm_use borrows the caller's
  // mc_set_actor_shard: replicated-critic data parallelism (every rank runs the critic on the whole batch, the actor
  // on episodes [shard_lo, shard_hi) with one all-reduce of the agent gradient); off while shard_hi <= shard_lo
  int shard_lo = 0, shard_hi = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};

  ~mc_handle() {   // the buffers free themselves
    if (comm && comm_owned) (void)ncclCommDestroy(comm);
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    mq_destroy(ah);
  }
};

namespace {

// One exchange step of the data-parallel mode: sum `n` floats at `buf` (caller-owned) over the ranks.
int mc_allreduce(mc_handle* h, float* buf, int64_t n, hipStream_t s) {
  if (h->dp_fn(buf, n, (void*)s, h->dp_ctx) != 0) return set_err(MQ_ERR_STATE, "data-parallel all-reduce callback failed");
  return MQ_OK;
}

// Library-owned arrays travel through the caller's scratch buffer.
int mc_allreduce_ws(mc_handle* h, float* ws_buf, int64_t n, hipStream_t s) {
  MQ_HIP(hipMemcpyAsync(h->dp_scratch, ws_buf, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  int rc = mc_allreduce(h, h->dp_scratch, n, s);
  if (rc) return rc;
  MQ_HIP(hipMemcpyAsync(ws_buf, h->dp_scratch, n * sizeof(float), hipMemcpyDeviceToDevice, s));
  return MQ_OK;
}

// Episodes [lo, hi) of a batch as a batch of their own: the id slice, or for a dense batch (no ids) every field
// pointer advanced by lo episodes.
mq_replay shard_replay(const mc_config& c, const mq_replay& b, int lo, int hi) {
  mq_replay s = b;
  s.batch_size = hi - lo;
  if (b.ep_ids_host) s.ep_ids_host = b.ep_ids_host + lo;
  if (b.ep_ids) s.ep_ids = b.ep_ids + lo;
  if (!b.ep_ids && !(b.ep_ids_host && b.batch_size <= MQ_INLINE_IDS)) {
    const int64_t e = (int64_t)lo * b.t_stride, n = c.n_agents;
    if (s.obs) s.obs += e * n * c.obs_dim;
    if (s.state) s.state += e * c.state_dim;
    if (s.actions) s.actions += e * n;
    if (s.avail_actions) s.avail_actions += e * n * c.n_actions;
    if (s.reward) s.reward += e;
    if (s.terminated) s.terminated += e;
    if (s.filled) s.filled += e;
    s.n_episodes = b.n_episodes - lo;
  }
  return s;
}

// The internal agent handle's config (no mixer) from a COMA or an actor-critic config `c`.
template <class C>
mq_config agent_config(const C& c, float gamma) {
  mq_config a{};
  a.n_agents = c.n_agents; a.n_actions = c.n_actions; a.obs_dim = c.obs_dim; a.state_dim = c.state_dim;
  a.rnn_hidden_dim = c.rnn_hidden_dim; a.mixer = MQ_MIXER_NONE;
  a.obs_last_action = c.obs_last_action; a.obs_agent_id = c.obs_agent_id; a.gamma = gamma; a.lr = c.lr;
  a.optim_alpha = c.optim_alpha; a.optim_eps = c.optim_eps; a.grad_norm_clip = c.grad_norm_clip;
  a.max_batch = c.max_batch; a.max_seq = c.max_seq;
  return a;
}

// The policy-gradient actor of the COMA and the actor-critic learners (a2c_host.hpp). `h` is either learner's handle:
// its agent handle h->ah lends the workspace `w` (w.dHo the learner's), h->agent are the agent's parameters, RT = T R
// the actor's rows. Which kernels and how many slices is ActorPlan's answer (actor_plan.hpp).
//
// The agent unroll over t < T, online net only: the logits land in w.Q.
template <class Hd>
int actor_forward(const Hd* h, const ActorPlan& ap, const Dims& d, const Rep& rpa, const Lay& L, const Work& w,
                  int64_t RT, hipStream_t st) {
  const mq_handle* ah = h->ah;
  const float* Pa = h->agent;
  if (ap.fused_fwd) {
    launch_fwd_fused(dim3(d.R, 1), st, d, rpa, Pa, Pa, L, w);
    MQ_HIP(hipGetLastError());
    return MQ_OK;
  }
  Fc1Prob p1{d, rpa, Pa, Pa, ah->off[MQ_P_FC1_W], ah->off[MQ_P_FC1_B], w.X1, w.XIN, RT};
  MQ_HIP(launch_gemm(p1, (int)RT, 2 * mq::H, 1, st));
  GiProb p2{w.X1, Pa, Pa, ah->off[MQ_P_RNN_W_IH], ah->off[MQ_P_RNN_B_IH], w.GI, RT};
  MQ_HIP(launch_gemm(p2, (int)RT, mq::G3, 1, st));
  const dim3 grid((d.R + ap.rw_fwd - 1) / ap.rw_fwd, 1);
  if (ap.rw_fwd == 1) hipLaunchKernelGGL((gru_fwd_kernel<1, 0>), grid, dim3(256), 0, st, d, Pa, Pa, L, w);
  else if (ap.rw_fwd == 2) hipLaunchKernelGGL((gru_fwd_kernel<2, 0>), grid, dim3(256), 0, st, d, Pa, Pa, L, w);
  else if (ap.rw_fwd == 4) hipLaunchKernelGGL((gru_fwd_kernel<4, 0>), grid, dim3(256), 0, st, d, Pa, Pa, L, w);
  else hipLaunchKernelGGL((gru_fwd_kernel<8, 0>), grid, dim3(256), 0, st, d, Pa, Pa, L, w);
  MQ_HIP(hipGetLastError());
  Fc2Prob p3{w.Hs, Pa, Pa, ah->off[MQ_P_FC2_W], ah->off[MQ_P_FC2_B], w.Q, RT, d.A};
  MQ_HIP(launch_gemm(p3, (int)RT, d.A, 1, st));
  return MQ_OK;
}

// From the policy kernel's h->dL [RT][Ap] (dense dLoss/dlogits) and its npol blocks of loss sums h->ppart: BPTT with
// the dense output gradient, the split-K weight gradients, and the two-pass reduction into h->agrad [Pa | MQ_NSUMS];
// *nnorm = the norm partials it left in h->norm_part.
template <class Hd>
int actor_backward(const Hd* h, const ActorPlan& ap, const Dims& d, const Rep& rpa, const Lay& L, const Work& w,
                   int64_t RT, int npol, hipStream_t s, int* nnorm) {
  const mq_handle* ah = h->ah;
  const float* Pa = h->agent;
  const int A = d.A;
  {
    DhoProb p{h->dL, h->Ap, A, Pa + ah->off[MQ_P_FC2_W], w.dHo, RT};
    MQ_HIP(launch_gemm(p, (int)RT, mq::H, 1, s));
  }
  const size_t dyn = ((size_t)2 * d.A * mq::H + d.A) * sizeof(float);
  if (ap.rw_bwd == 1)
    hipLaunchKernelGGL((gru_bwd_kernel<1, 0, true>), dim3(ap.nblk_bwd), dim3(512), dyn, s, d, rpa, Pa, L, w,
                       ah->len_rnn);
  else
    hipLaunchKernelGGL((gru_bwd_kernel<2, 0, true>), dim3(ap.nblk_bwd), dim3(512), dyn, s, d, rpa, Pa, L, w,
                       ah->len_rnn);
  MQ_HIP(hipGetLastError());
  {
    Dx1Prob p{w.dGI, Pa + ah->off[MQ_P_RNN_W_IH], w.X1, w.dP1, RT};
    MQ_HIP(launch_gemm(p, (int)RT, mq::H, 1, s));
  }
  {
    Dw1Prob p{d.I, w.dP1, w.XIN, w.slab_fc1, RT, ap.ns_w1};
    MQ_HIP(launch_gemm(p, mq::H, d.I, ap.ns_w1, s));
  }
  {
    Dw2Prob p{h->dL, h->Ap, A, w.Hs, h->slab_fc2, RT, ap.ns_w2};
    MQ_HIP(launch_gemm(p, A, mq::H, ap.ns_w2, s));
  }
  RedBuilder rb(h->red_tmp);
  rb.add(w.slab_fc1, ap.ns_w1, (int64_t)mq::H * d.I + mq::H, h->agrad + ah->off[MQ_P_FC1_W], true);
  // W_ih .. b_hh: the prefix of each BPTT slab (its fc2 part is unused in the dense-dy mode)
  rb.add(w.slab_rnn, ap.nblk_bwd, ah->off[MQ_P_FC2_W] - ah->off[MQ_P_RNN_W_IH], h->agrad + ah->off[MQ_P_RNN_W_IH],
         true, ah->len_rnn);
  rb.add(h->slab_fc2, ap.ns_w2, (int64_t)A * mq::H + A, h->agrad + ah->off[MQ_P_FC2_W], true);
  rb.add(h->ppart, npol, MQ_NSUMS, h->agrad + h->Pa, false);
  return launch_reduce(rb, h->norm_part, "agent", s, nnorm);
}

// The critic's three GEMMs over M rows of X [M][Kp] with parameters P at offsets `off` (mc_offsets): H1, H2, then
// Q [M][A]. The target pass of a train step and mc_critic_forward.
int critic_forward(const float* P, const int64_t* off, const CDims& cd, const float* X, float* H1, float* H2, float* Q,
                   int64_t M, hipStream_t s) {
  const CLinProbT<64> l1 =
      CLinProbT<64>{X, cd.Kp, P + off[MC_P_FC1_W], P + off[MC_P_FC1_B], H1, M, CH, cd.Kc, 1}.with_vec();
  MQ_HIP(launch_gemm(l1, (int)M, CH, 1, s));
  const CLinProbT<64> l2 = CLinProbT<64>{H1, CH, P + off[MC_P_FC2_W], P + off[MC_P_FC2_B], H2, M, CH, CH, 1}.with_vec();
  MQ_HIP(launch_gemm(l2, (int)M, CH, 1, s));
  const CLinProbT<64> l3 = CLinProbT<64>{H2, CH, P + off[MC_P_FC3_W], P + off[MC_P_FC3_B], Q, M, cd.A, CH, 0}.with_vec();
  MQ_HIP(launch_gemm(l3, (int)M, cd.A, 1, s));
  return MQ_OK;
}

OptHP critic_hp(const mc_config& c) { return OptHP{c.critic_lr, c.optim_alpha, c.optim_eps, c.grad_norm_clip, 1}; }

// The three-launch critic step's argument block.
CritArgs crit_args(const mc_handle* h, const ComaPlan& pl, const CDims& cd, const Rep& rp) {
  CritArgs a{};
  a.d = cd; a.rp = rp;
  a.P[0] = h->critic; a.P[1] = h->Pshadow; a.SQ[0] = h->csq; a.SQ[1] = h->SQshadow; a.G = h->cgrad;
  a.o_w1 = h->coff[MC_P_FC1_W]; a.o_b1 = h->coff[MC_P_FC1_B]; a.o_w2 = h->coff[MC_P_FC2_W];
  a.o_b2 = h->coff[MC_P_FC2_B]; a.o_w3 = h->coff[MC_P_FC3_W]; a.o_b3 = h->coff[MC_P_FC3_B]; a.Pc = h->Pc;
  a.X = h->X; a.tgt = h->tgt; a.msum = h->msum; a.H1p = h->H1p; a.KS = pl.KS;
  a.H1c = h->H1c; a.H2c = h->H2c; a.dH1c = h->dH1c; a.dH2c = h->dH2c; a.dqc = h->dqc; a.actc = h->actc;
  a.qvals = h->qvals; a.cpart = h->cpart; a.cnorm = h->cnorm; a.crec = h->crec; a.cstate = h->cstate;
  a.nhead = pl.nhead; a.nwgrad = pl.nwgrad;
  a.hp = critic_hp(h->cfg);
  return a;
}

// The persistent chain's argument block. cstate (zeroed by the step's first memset) carries its sync words; cnorm
// (zeroed before the launch): [0, 2 G) the norm granules, [512, 512 + G) flagA, [768, 768 + NHEAD) flagB.
CChain chain_args(const mc_handle* h, const ComaPlan& pl, const CDims& cd, const Rep& rp) {
  CChain a{};
  a.d = cd; a.rp = rp; a.P = h->critic; a.SQ = h->csq; a.G = h->cgrad;
  a.o_w1 = h->coff[MC_P_FC1_W]; a.o_b1 = h->coff[MC_P_FC1_B]; a.o_w2 = h->coff[MC_P_FC2_W];
  a.o_b2 = h->coff[MC_P_FC2_B]; a.o_w3 = h->coff[MC_P_FC3_W]; a.o_b3 = h->coff[MC_P_FC3_B]; a.Pc = h->Pc;
  a.X = h->X; a.tgt = h->tgt; a.msum = h->msum; a.H1p = h->H1p;
  a.H1x = h->H1c; a.H2x = h->H2c; a.dH2x = h->dH2c; a.dH1x = h->dH1c; a.dqx = h->dqc; a.actx = h->actc;
  a.part = h->cpart; a.normg = (unsigned long long*)h->cnorm; a.GW = h->Pshadow; a.qvals = h->qvals;
  a.crec = h->crec; a.cstate = h->cstate; a.sync = (unsigned*)(h->cstate + 2);
  a.flagA = (unsigned*)(h->cnorm + 512);
  a.flagB = (unsigned*)(h->cnorm + 768);
  a.NK = pl.NK; a.NG = pl.NG; a.NHEAD = pl.nhead;
  a.hp = critic_hp(h->cfg);
  a.trace = h->chain_trace;
  a.fault_wg = env_int("MQ_DIAG", "coma_fault", -1);   // test hook: a workgroup that stops flagging
  return a;
}

// debug (MQ_DIAG coma_trace): per-phase spans of the chain's workgroup 0 (100 MHz clock), averaged over <= 16 steps
int print_chain_trace(const mc_handle* h, hipStream_t s) {
  unsigned long long hb[16 * 8];
  MQ_HIP(hipMemcpyAsync(hb, h->chain_trace, sizeof(hb), hipMemcpyDeviceToHost, s));
  MQ_HIP(hipStreamSynchronize(s));
  double acc[8] = {0};
  for (int i = 1; i < 15; ++i)
    for (int k = 0; k < 8; ++k) acc[k] += 10.0 * (double)((k < 7 ? hb[i * 8 + k + 1] : hb[(i + 1) * 8]) - hb[i * 8 + k]);
  std::fprintf(stderr, "coma_chain ns/step: A %.0f bar1 %.0f B %.0f bar2 %.0f C %.0f bar3 %.0f D %.0f next %.0f\n",
               acc[0] / 14, acc[1] / 14, acc[2] / 14, acc[3] / 14, acc[4] / 14, acc[5] / 14, acc[6] / 14, acc[7] / 14);
  return MQ_OK;
}

// One COMA train step's launches, phase by phase in stream order (mc_train_step calls them in this order). Which
// kernels run, on which grids and streams, is the plan `pl`, fixed before the first launch.
struct ComaStep {
  mc_handle* h;
  const ComaPlan pl;
  const ComaMode m;
  const CDims cd;
  const Rep rp;    // the critic's batch: the whole one
  const Rep rpa;   // the actor's: this rank's episodes under a replicated critic
  const Dims d;    // the actor's dims (t < T)
  const Lay L;
  const Work w;
  const float epsilon;
  hipStream_t s;
  bool chained = false;      // the chain's launch was accepted: critic_steps() has nothing to launch
  bool actor_side = false;   // the actor's forward went out on the side stream
  int nnorm = 0;             // the agent's norm partials in norm_part

  int targets();
  int critic_chain();
  int critic_steps();
  int actor();
  int exchange();
  int apply_and_stats();
};

ComaStep make_coma_step(mc_handle* h, const mq_replay* batch, const ComaPlan& pl, const ComaMode& m, float epsilon,
                        hipStream_t s) {
  const mc_config& c = h->cfg;
  // replicated critic: the actor trains this rank's episodes only (the critic sees the whole batch)
  mq_replay av = m.replicated ? shard_replay(c, *batch, m.shard_lo, m.shard_hi) : *batch;
  av.t_len = pl.T;
  const Rep rp = make_rep(batch);
  Work w = h->ah->w;
  w.dHo = h->dHo;
  return ComaStep{h, pl, m, coma_dims(c, batch->batch_size, batch->t_len, batch->t_stride), rp,
                  m.replicated ? make_rep(&av) : rp, mq::make_dims(h->ah->cfg, av.batch_size, av.t_len, av.t_stride),
                  make_lay(h->ah), w, epsilon, s};
}

// Mask sums (summed over the ranks in exchange mode), the critic inputs X, the target critic over every stored step
// (coma_learner.py:102), TD(lambda) (rl_utils.py:4-14); then what the critic steps start from: q_vals zeroed (skipped
// steps keep 0) and, in exchange mode, the live steps on the host.
int ComaStep::targets() {
  const int T = pl.T, Tp = T + 1, R = pl.R;
  if (m.timing) MQ_HIP(hipEventRecord(h->ev[0], s));
  MQ_HIP(hipMemsetAsync(h->crec, 0, (size_t)T * 8 * sizeof(float), s));
  MQ_HIP(hipMemsetAsync(h->cstate, 0, 8 * sizeof(int), s));
  hipLaunchKernelGGL(coma_mask_kernel, dim3((T + 255) / 256), dim3(256), 0, s, cd, rp, h->msum);
  MQ_HIP(hipGetLastError());
  int rc;
  if (m.exchange) {   // global per-step mask sums: every rank normalises by them and skips the same steps
    if (h->dp_scratch_n < 8LL * T) return set_err(MQ_ERR_ARG, "data-parallel scratch smaller than 8 * t_len");
    if ((rc = mc_allreduce_ws(h, h->msum, T, s))) return rc;
  }
  hipLaunchKernelGGL(coma_xin_kernel, dim3(Tp * R), dim3(256), 0, s, cd, rp, h->X);
  MQ_HIP(hipGetLastError());
  if ((rc = critic_forward(h->tcritic, h->coff, cd, h->X, h->H1t, h->H2t, h->Qt, (int64_t)Tp * R, s))) return rc;
  hipLaunchKernelGGL(coma_td_kernel, dim3(cd.B), dim3(256), pl.lds_td, s, cd, rp, h->Qt, h->tgt);
  MQ_HIP(hipGetLastError());
  MQ_HIP(hipMemsetAsync(h->qvals, 0, (size_t)T * R * cd.A * sizeof(float), s));
  if (m.exchange) {   // the host needs the live steps to place the per-step exchanges (one synchronisation per train)
    h->dp_msum.resize(T);
    MQ_HIP(hipMemcpyAsync(h->dp_msum.data(), h->msum, (size_t)T * sizeof(float), hipMemcpyDeviceToHost, s));
    MQ_HIP(hipStreamSynchronize(s));
  }
  return MQ_OK;
}

// Every critic step (coma_learner.py:118-139) in one persistent launch where the plan says so, with the actor's agent
// unroll beside it: the unroll reads nothing the critic writes, so it runs on the side stream in the CUs the chain
// leaves idle. A refused launch clears chain_env and leaves the steps to critic_steps(), in this train() and after.
int ComaStep::critic_chain() {
  mq_handle* ah = h->ah;
  if (pl.overlap) {
    MQ_HIP(ensure_side(ah));
    MQ_HIP(hipEventRecord(ah->ev_fork, s));   // before the chain: the side stream does not wait for it
  }
  if (m.timing) MQ_HIP(hipEventRecord(h->ev[1], s));
  if (!pl.chain) return MQ_OK;
  int rc;
  if (env_item("MQ_DIAG", "coma_trace") &&
      (rc = h->chain_trace.alloc(16 * 8, "hipMalloc(&h->chain_trace, 16 * 8 * sizeof(unsigned long long))")))
    return rc;
  const CChain cc = chain_args(h, pl, cd, rp);
  MQ_HIP(hipMemsetAsync(h->cnorm, 0, 1024 * sizeof(float), s));   // norm granules and flags: no stale step tags
  MQ_LDS(coma_chain_kernel, pl.lds_chain);
  if (!h->chain_attr) {
    MQ_HIP(hipFuncSetAttribute((const void*)coma_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)pl.lds_chain));
    h->chain_attr = true;
  }
  // the chain updates the critic in place: keep the pre-train version, restored if a hand-off times out
  // (apply_and_stats: the critic is put back before the actor's apply, the apply is skipped through its halt word, so
  // the learner state is this train()'s starting state and COMALearner.train raises)
  MQ_HIP(hipMemcpyAsync(h->Pbak, h->critic, (size_t)h->Pc * sizeof(float), hipMemcpyDeviceToDevice, s));
  MQ_HIP(hipMemcpyAsync(h->Pbak + h->Pc, h->csq, (size_t)h->Pc * sizeof(float), hipMemcpyDeviceToDevice, s));
  // A plain launch: the grid (cc_ok: at most one 512-thread workgroup per CU, NG <= the CU count) is resident
  // by its size alone, which is all a cooperative launch would add a check for (MI355X_MICROARCH.md "Residency
  // and cooperative launch": plain and cooperative launches give the same residency). Nothing else on the device
  // waits on the chain, so a workgroup that starts late only delays it; every spin is bounded. The cooperative
  // launch also cost 15-19 us of host time per train and, under rocprofv3, its dedicated HIP queue crashed the
  // runtime's exit-time teardown (round 4: profiles/r04a_cfg5_rocprof_exit_crash.txt)
  hipLaunchKernelGGL(coma_chain_kernel, dim3(pl.NG), dim3(CC_THREADS), pl.lds_chain, s, cc);
  if (hipGetLastError() != hipSuccess) {   // the launch was refused: the three-launch path, from now on
    h->chain_env = false;
    return MQ_OK;
  }
  chained = true;
  if (h->chain_trace && (rc = print_chain_trace(h, s))) return rc;
  // Launched after the chain on a low-priority stream, so the chain's workgroups are normally dispatched first.
  // That order is a heuristic across hardware queues, not a guarantee: if actor workgroups take CUs first, the
  // chain's late workgroups start when they finish (the actor never waits on the chain), well inside the chain's
  // spin bound (CC_SPIN_LIMIT polls, orders of magnitude longer than the actor unroll); a timeout would still be
  // loud and leave the learner state unchanged (the restore)
  if (pl.overlap) {
    MQ_HIP(hipStreamWaitEvent(ah->side, ah->ev_fork, 0));
    if ((rc = actor_forward(h, pl.actor, d, rpa, L, w, pl.actor_rows, ah->side))) return rc;
    MQ_HIP(hipEventRecord(ah->ev_join, ah->side));
    actor_side = true;
  }
  return MQ_OK;
}

// The critic's T sequential steps as three launches each and the last update's apply, where no chain ran; then, in
// exchange mode, the per-step stat sums over the ranks.
int ComaStep::critic_steps() {
  const int T = pl.T;
  int rc;
  if (!chained) {
    const CritArgs ca = crit_args(h, pl, cd, rp);
    const dim3 l1_grid(pl.KS, CH / 16, (pl.R + kL1Rows - 1) / kL1Rows);
    int live = 0;
    for (int t = T - 1; t >= 0; --t) {
      // live steps before t: exact in exchange mode, else assumed none was skipped (the kernels correct it)
      const int Lexp = m.exchange ? live : T - 1 - t;
      hipLaunchKernelGGL(coma_l1_kernel, l1_grid, dim3(256), pl.lds_l1, s, ca, t, Lexp);
      hipLaunchKernelGGL(coma_head_kernel, dim3(pl.nhead), dim3(kHeadThreads), pl.lds_head, s, ca, t, Lexp);
      hipLaunchKernelGGL(coma_wgrad_kernel, dim3(pl.nwgrad), dim3(256), 0, s, ca, t);
      if (m.exchange && h->dp_msum[t] > 0.0f) {   // sum the step's unnormalised gradient, then its norm from the sum
        ++live;
        MQ_HIP(hipGetLastError());
        if ((rc = mc_allreduce(h, h->cgrad, h->Pc, s))) return rc;
        hipLaunchKernelGGL(sumsq_kernel, dim3(pl.nwgrad), dim3(256), 0, s, (const float*)h->cgrad, h->Pc, h->cnorm);
      }
    }
    MQ_HIP(hipGetLastError());
    hipLaunchKernelGGL(coma_capply_kernel, dim3((int)std::min<int64_t>((h->Pc + 255) / 256, 512)), dim3(256), 0, s,
                       ca);
  }
  MQ_HIP(hipGetLastError());
  if (m.exchange) {   // per-step critic stat sums; the replicated fields (mask sum, norm, live flag) come from rank 0
    if (h->dp_rank != 0) hipLaunchKernelGGL(coma_dp_crec_kernel, dim3((T + 255) / 256), dim3(256), 0, s, h->crec, T);
    MQ_HIP(hipGetLastError());
    if ((rc = mc_allreduce_ws(h, h->crec, 8LL * T, s))) return rc;
  }
  if (m.timing) MQ_HIP(hipEventRecord(h->ev[2], s));
  return MQ_OK;
}

// The agent unroll over t < T (coma_learner.py:52-57; joined here if it ran beside the chain), the policy, baseline,
// advantage, loss sums and dLogits (coma_learner.py:59-77, basic_controller.py:53-73), then the BPTT with the dense
// output gradient, the weight gradients and their reduction.
int ComaStep::actor() {
  int rc;
  if (actor_side) MQ_HIP(hipStreamWaitEvent(s, h->ah->ev_join, 0));
  else if ((rc = actor_forward(h, pl.actor, d, rpa, L, w, pl.actor_rows, s))) return rc;
  const float eps = epsilon, omeps = (float)(1.0 - (double)epsilon);
  hipLaunchKernelGGL(coma_policy_kernel, dim3(pl.npol), dim3(256), 0, s, d, rpa, (const float*)w.Q,
                     (const float*)h->qvals, pl.R, pl.qv_r0, eps, omeps, (int)(h->cfg.mask_before_softmax != 0), h->Ap,
                     h->dL, h->pi, h->ppart);
  MQ_HIP(hipGetLastError());
  return actor_backward(h, pl.actor, d, rpa, L, w, pl.actor_rows, pl.npol, s, &nnorm);
}

// Data parallel: the agent gradient + loss / mask sums over the ranks, then the norm partials of the summed gradient.
// Under a replicated critic the chain's error word rides in the agent sums' spare slot 7 (0 on success), so any rank's
// chain failure halts every rank: all roll back, skip the apply and raise.
int ComaStep::exchange() {
  if (!m.exchange && !m.replicated) return MQ_OK;
  const bool halt = m.replicated && chained;
  if (halt) {
    hipLaunchKernelGGL(coma_halt_to_sum_kernel, dim3(1), dim3(64), 0, s, (const int*)(h->cstate + 3),
                       h->agrad + h->Pa + 7);
    MQ_HIP(hipGetLastError());
  }
  const int rc = mc_allreduce(h, h->agrad, h->Pa + MQ_NSUMS, s);
  if (rc) return rc;
  if (halt) {
    hipLaunchKernelGGL(coma_sum_to_halt_kernel, dim3(1), dim3(64), 0, s, (const float*)(h->agrad + h->Pa + 7),
                       h->cstate + 3);
    MQ_HIP(hipGetLastError());
  }
  nnorm = 256;
  hipLaunchKernelGGL(sumsq_kernel, dim3(nnorm), dim3(256), 0, s, (const float*)h->agrad, h->Pa, h->norm_part);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

// A timed-out chain (on any rank, when replicated) puts the critic back to its pre-train version; the agent's RMSprop
// step (none after such a failure: its halt word); the stats.
int ComaStep::apply_and_stats() {
  const mc_config& c = h->cfg;
  if (chained) {
    hipLaunchKernelGGL(coma_chain_restore_kernel, dim3(64), dim3(256), 0, s, (const int*)h->cstate,
                       (const float*)h->Pbak, h->critic, h->csq, h->Pc);
    MQ_HIP(hipGetLastError());
  }
  const OptHP hp{c.lr, c.optim_alpha, c.optim_eps, c.grad_norm_clip, 1};
  const int blocks = (int)std::min<int64_t>((h->Pa + 255) / 256, 1024);
  hipLaunchKernelGGL(apply_kernel, dim3(blocks), dim3(256), 0, s, h->agent, h->agrad, h->asq, h->Pa,
                     (const float*)h->norm_part, nnorm, hp, h->stats + 8,
                     chained ? (const int*)(h->cstate + 3) : (const int*)nullptr);
  MQ_HIP(hipGetLastError());
  hipLaunchKernelGGL(coma_stats_kernel, dim3(1), dim3(64), 0, s, (const float*)h->crec, pl.T, (const int*)h->cstate,
                     h->stats);
  MQ_HIP(hipGetLastError());
  if (m.timing) MQ_HIP(hipEventRecord(h->ev[3], s));
  return MQ_OK;
}

}  // namespace

extern "C" {

int64_t mc_critic_forward_workspace(const mc_config* cfg, int32_t batch_size, int32_t t_count) {
  if (!cfg || batch_size < 1 || t_count < 1) return -1;
  const int64_t Kp = (coma_k(*cfg) + 3) & ~3;
  const int64_t M = (int64_t)t_count * batch_size * cfg->n_agents;
  return align_up(M * Kp) + 2 * align_up(M * CH) + align_up(M * cfg->n_actions);
}

int mc_critic_forward(const float* critic, const mc_config* cfg, const mq_replay* batch, int32_t t, float* q_out,
                      float* workspace, void* stream) {
  if (!critic || !cfg || !batch || !q_out || !workspace) return set_err(MQ_ERR_ARG, "mc_critic_forward: NULL pointer");
  if (!batch->obs || !batch->state || !batch->actions || !batch->filled)
    return set_err(MQ_ERR_ARG, "mc_critic_forward: batch needs obs, state, actions and filled");
  if (batch->batch_size < 1 || batch->t_len < 1 || batch->t_len > batch->t_stride)
    return set_err(MQ_ERR_ARG, "mc_critic_forward: bad batch dimensions");
  if (t >= batch->t_len) return set_err(MQ_ERR_ARG, "mc_critic_forward: t outside the batch");
  if (batch->ep_ids_host && batch->batch_size > MQ_INLINE_IDS && !batch->ep_ids)
    return set_err(MQ_ERR_ARG, "mc_critic_forward: more than MQ_INLINE_IDS episodes need device ids");
  hipStream_t s = (hipStream_t)stream;
  const int Tq = t < 0 ? batch->t_len : 1, t0 = t < 0 ? 0 : t;
  const CDims cd = coma_dims(*cfg, batch->batch_size, batch->t_len, batch->t_stride);
  const Rep rp = make_rep(batch);
  const int64_t M = (int64_t)Tq * cd.R;
  float* X = workspace;
  float* H1 = X + align_up(M * cd.Kp);
  float* H2 = H1 + align_up(M * CH);
  float* Q = H2 + align_up(M * CH);
  int64_t off[MC_P_COUNT + 1];
  mc_offsets(*cfg, off);
  hipLaunchKernelGGL(coma_xin_kernel, dim3((unsigned)M), dim3(256), 0, s, cd, rp, X, t0);
  MQ_HIP(hipGetLastError());
  const int rc = critic_forward(critic, off, cd, X, H1, H2, Q, M, s);
  if (rc) return rc;
  const int64_t tot = M * cd.A;
  hipLaunchKernelGGL(coma_q_layout_kernel, dim3((unsigned)std::min<int64_t>((tot + 255) / 256, 4096)), dim3(256), 0, s,
                     (const float*)Q, q_out, Tq, cd.B, cd.n, cd.A);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mc_create(const mc_config* cfg, mc_handle** out) {
  if (!cfg || !out) return set_err(MQ_ERR_ARG, "NULL argument");
  const mc_config& c = *cfg;
  if (c.n_actions < 1 || c.n_actions > 64) return set_err(MQ_ERR_ARG, "n_actions must be in [1, 64]");
  if (c.max_batch * c.n_agents > MQ_INLINE_IDS * 64) return set_err(MQ_ERR_ARG, "max_batch * n_agents too large");
  const mq_config ac = agent_config(c, c.gamma);
  mq_handle* ah = nullptr;
  int rc = mq_create(&ac, &ah);
  if (rc) return rc;
  std::unique_ptr<mc_handle> h(new mc_handle());   // owns ah from here: a failure below frees both
  h->cfg = c;
  h->ah = ah;
  h->I = ah->I;
  for (int i = 0; i <= MQ_P_COUNT; ++i) h->aoff[i] = ah->off[i];
  h->Pa = ah->P;
  const int n = c.n_agents, A = c.n_actions;
  h->Kc = coma_k(c);
  h->Kp = (h->Kc + 3) & ~3;
  h->Ap = (A + 3) & ~3;
  mc_offsets(c, h->coff);
  h->Pc = h->coff[MC_P_COUNT];

  const int64_t Tp = c.max_seq, R = (int64_t)c.max_batch * n, T = Tp - 1;
  const int64_t RTa = T * R;   // actor rows (T steps)
  const int64_t red_tmp = kRedZ * ((int64_t)mq::H * h->I + mq::H) + kRedZ * h->ah->len_rnn +
                          kRedZ * (A * mq::H + A) + kRedZ * 8;
  const WsTable ws = {
      {"X", Tp * R * h->Kp, &h->X},
      {"H1t", Tp * R * CH, &h->H1t}, {"H2t", Tp * R * CH, &h->H2t},
      {"Qt", Tp * R * A, &h->Qt},
      {"tgt", T * R, &h->tgt}, {"msum", T, &h->msum},
      // three-launch l1 or chain phase A
      {"H1p", coma_h1p_slices(h->Kc) * R * CH, &h->H1p},
      {"H1c", R * CH, &h->H1c}, {"H2c", R * CH, &h->H2c}, {"dH1c", R * CH, &h->dH1c}, {"dH2c", R * CH, &h->dH2c},
      {"dqc", R, &h->dqc}, {"actc", R, nullptr, &h->actc},
      {"qvals", T * R * A, &h->qvals},
      {"cpart", (int64_t)coma_heads((int)R) * 8, &h->cpart},
      // chain: 256 8-B granules + flags
      {"cnorm", std::max<int64_t>(coma_wgrad_blocks(h->Kc, A), 1024), &h->cnorm},
      {"crec", T * 8, &h->crec},
      // shadow params / square_avg (the chain's gradient exchange: Pshadow)
      {"Pshadow", h->Pc, &h->Pshadow}, {"SQshadow", h->Pc, &h->SQshadow},
      {"cstate", 8, nullptr, &h->cstate},   // + the critic chain's sync words
      {"dL", RTa * h->Ap, &h->dL}, {"dHo", RTa * mq::H, &h->dHo}, {"pi", RTa * A, &h->pi},
      {"ppart", ((RTa + 3) / 4) * 8, &h->ppart},
      {"slab_fc2", (int64_t)kNsplitMax * (A * mq::H + A), &h->slab_fc2},
      {"red_tmp", red_tmp, &h->red_tmp},
      {"norm_part", kNormPartMax, &h->norm_part},
      {"Pbak", 2 * h->Pc, &h->Pbak},
  };
  if ((rc = ws_carve(h->ws, ws, "COMA workspace hipMalloc"))) return rc;
  h->chain_env = plan_int("coma_chain", 1) != 0;   // MQ_PLAN coma_chain=0: three launches per critic step
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&h->num_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    h->num_cu = 0;
  *out = h.release();
  return MQ_OK;
}

int mc_destroy(mc_handle* h) {
  delete h;
  return MQ_OK;
}

int mc_param_offsets(const mc_handle* h, int64_t* agent_offsets, int64_t* critic_offsets) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  if (agent_offsets)
    for (int i = 0; i <= MQ_P_COUNT; ++i) agent_offsets[i] = h->aoff[i];
  if (critic_offsets)
    for (int i = 0; i <= MC_P_COUNT; ++i) critic_offsets[i] = h->coff[i];
  return MQ_OK;
}

int mc_bind(mc_handle* h, float* agent, float* agent_grad, float* agent_sq, float* critic, float* target_critic,
            float* critic_grad, float* critic_sq, float* stats) {
  if (!h || !agent || !agent_grad || !agent_sq || !critic || !target_critic || !critic_grad || !critic_sq || !stats)
    return set_err(MQ_ERR_ARG, "mc_bind: NULL pointer");
  h->agent = agent; h->agrad = agent_grad; h->asq = agent_sq; h->critic = critic; h->tcritic = target_critic;
  h->cgrad = critic_grad; h->csq = critic_sq; h->stats = stats;
  // the agent handle: online = target = the agent params (the actor has no target net); stats land at stats + 8
  return mq_bind(h->ah, agent, agent, agent_grad, agent_sq, stats + 8, nullptr);
}

int mc_train_step(mc_handle* h, const mq_replay* batch, float epsilon, void* stream) {
  if (!h || !h->agent) return set_err(MQ_ERR_STATE, "mc_train_step before mc_bind");
  int rc = check_batch(h->ah, batch);
  if (rc) return rc;
  const bool repl = h->shard_hi > h->shard_lo;
  if (repl && (h->shard_lo < 0 || h->shard_hi > batch->batch_size))
    return set_err(MQ_ERR_ARG, "actor shard [" + std::to_string(h->shard_lo) + ", " + std::to_string(h->shard_hi) +
                                   ") outside the batch of " + std::to_string(batch->batch_size) + " episodes");
  if (repl && !h->dp_fn)
    return set_err(MQ_ERR_STATE, "a replicated critic needs an all-reduce for the actor (mc_set_data_parallel / "
                                 "mc_comm_attach)");
  // exchange mode (an all-reduce and no shard): the critic steps are summed over the ranks. MQ_PLAN coma_overlap=0,
  // read per train(): the actor's agent unroll stays on the caller's stream
  const ComaMode mode{h->dp_fn != nullptr && !repl, repl, h->timing, h->chain_env, plan_int("coma_overlap", 1) != 0,
                      h->shard_lo, h->shard_hi};
  const ComaPlan pl = coma_plan(h->cfg, batch->batch_size, batch->t_len, h->num_cu, mode);
  if (pl.refused) return set_err(MQ_ERR_ARG, pl.refused);
  ComaStep st = make_coma_step(h, batch, pl, mode, epsilon, (hipStream_t)stream);
  if ((rc = st.targets()) || (rc = st.critic_chain()) || (rc = st.critic_steps()) || (rc = st.actor()) ||
      (rc = st.exchange()) || (rc = st.apply_and_stats()))
    return rc;
  h->last_path = st.chained ? 1 : 0;
  h->last_T = pl.T;
  h->last_R = pl.actor_R;   // the rows of pi (the actor's); qvals / targets keep the critic's R rows
  h->last_Rc = pl.R;
  return MQ_OK;
}

int mc_set_data_parallel(mc_handle* h, mc_allreduce_fn allreduce, void* ctx, int32_t rank, float* scratch,
                         int64_t scratch_count) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  if (allreduce && (!scratch || scratch_count < 8LL * h->cfg.max_seq))
    return set_err(MQ_ERR_ARG, "mc_set_data_parallel: scratch must hold 8 * max_seq floats");
  h->dp_fn = allreduce;
  h->dp_ctx = ctx;
  h->dp_rank = rank;
  h->dp_scratch = scratch;
  h->dp_scratch_n = scratch_count;
  return MQ_OK;
}

// mc_allreduce_fn over the handle's RCCL communicator (ctx = the mc_handle)
static int mc_rccl_allreduce(float* buf, int64_t count, void* stream, void* ctx) {
  mc_handle* h = (mc_handle*)ctx;
  return ncclAllReduce(buf, buf, (size_t)count, ncclFloat, ncclSum, h->comm, (hipStream_t)stream) == ncclSuccess ? 0 : 1;
}

int mc_set_actor_shard(mc_handle* h, int32_t lo, int32_t hi) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  if (hi > lo && (lo < 0 || hi > h->cfg.max_batch)) return set_err(MQ_ERR_ARG, "mc_set_actor_shard: bad episode range");
  h->shard_lo = hi > lo ? lo : 0;
  h->shard_hi = hi > lo ? hi : 0;
  return MQ_OK;
}

int mc_comm_attach(mc_handle* h, const uint8_t* id, int32_t rank, int32_t world) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  if (h->comm) return set_err(MQ_ERR_STATE, "a communicator is already attached");
  const int64_t n = 8LL * h->cfg.max_seq;
  // (the allocation's name is the text its failure message has always carried)
  int rc = h->comm_scratch.alloc(n, "hipMalloc(&h->comm_scratch, n * sizeof(float))");
  if (rc || (rc = comm_init(&h->comm, id, rank, world))) return rc;
  h->comm_owned = true;
  return mc_set_data_parallel(h, mc_rccl_allreduce, h, rank, h->comm_scratch, n);
}

int mc_comm_use(mc_handle* h, void* comm) {
  if (!h || !comm) return set_err(MQ_ERR_ARG, "NULL handle or communicator");
  if (h->comm) return set_err(MQ_ERR_STATE, "a communicator is already attached");
  int rank = 0;
  const ncclResult_t r = ncclCommUserRank((ncclComm_t)comm, &rank);
  if (r != ncclSuccess) return set_err(MQ_ERR_ARG, std::string("ncclCommUserRank: ") + ncclGetErrorString(r));
  const int64_t n = 8LL * h->cfg.max_seq;
  if (const int rc = h->comm_scratch.alloc(n, "hipMalloc(&h->comm_scratch, n * sizeof(float))")) return rc;
  h->comm = (ncclComm_t)comm;
  h->comm_owned = false;
  return mc_set_data_parallel(h, mc_rccl_allreduce, h, rank, h->comm_scratch, n);
}

int mc_comm_detach(mc_handle* h) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  if (h->comm && h->comm_owned) (void)ncclCommDestroy(h->comm);
  const bool was_rccl = h->dp_fn == mc_rccl_allreduce;
  h->comm = nullptr;
  h->comm_owned = false;
  return was_rccl ? mc_set_data_parallel(h, nullptr, nullptr, 0, nullptr, 0) : MQ_OK;
}

int mc_set_timing(mc_handle* h, int32_t on) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  for (auto& e : h->ev)
    if (!e) MQ_HIP(hipEventCreate(&e));
  h->timing = on != 0;
  return MQ_OK;
}

int mc_phase_times(mc_handle* h, float* ms) {
  if (!h || !ms) return set_err(MQ_ERR_ARG, "NULL argument");
  if (!h->ev[3]) return set_err(MQ_ERR_STATE, "timing was never enabled");
  MQ_HIP(hipEventSynchronize(h->ev[3]));
  for (int i = 0; i < 3; ++i) MQ_HIP(hipEventElapsedTime(&ms[i], h->ev[i], h->ev[i + 1]));
  return MQ_OK;
}

int32_t mc_last_critic_path(const mc_handle* h) { return h ? h->last_path : -1; }

int mc_update_targets(mc_handle* h, void* stream) {
  if (!h || !h->critic) return set_err(MQ_ERR_STATE, "mc_update_targets before mc_bind");
  MQ_HIP(hipMemcpyAsync(h->tcritic, h->critic, h->Pc * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MQ_OK;
}

int mc_policy(float* logits, const int32_t* avail, int32_t rows, int32_t n_actions, float epsilon,
              int32_t mask_before_softmax, int32_t test_mode, void* stream) {
  if (!logits || !avail || rows < 0 || n_actions < 1 || n_actions > 64) return set_err(MQ_ERR_ARG, "bad mc_policy args");
  if (rows == 0) return MQ_OK;
  hipLaunchKernelGGL(mc_policy_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, avail,
                     (int)rows, (int)n_actions, epsilon, (int)mask_before_softmax, (int)test_mode);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mc_copy_intermediate(mc_handle* h, int which, float* dst, int64_t* count, void* stream) {
  if (!h || h->last_T <= 0) return set_err(MQ_ERR_STATE, "no COMA train step has run");
  const int64_t TR = (int64_t)h->last_T * h->last_R, TRc = (int64_t)h->last_T * h->last_Rc;
  const float* src;
  int64_t cnt;
  switch (which) {
    case 0: src = h->qvals; cnt = TRc * h->cfg.n_actions; break;
    case 1: src = h->tgt; cnt = TRc; break;
    case 2: src = h->pi; cnt = TR * h->cfg.n_actions; break;
    default: return set_err(MQ_ERR_ARG, "unknown COMA intermediate id");
  }
  if (count) *count = cnt;
  if (dst) MQ_HIP(hipMemcpyAsync(dst, src, cnt * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MQ_OK;
}

}  // extern "C"
