// The launches of the policy-gradient actor the COMA, actor-critic and PPO learners share (actor_plan.hpp describes
// it): the agent handle a.ah lends the kernels and the workspace, a.y is the layout (the handle's own, but for the wide
// feed-forward actor, which also brings its own [RT][128] rows), a.agent are the parameters. Which kernels and how many
// slices is ActorPlan's answer; the policy kernel between forward and backward is its learner's.
#pragma once
#include "a2c_kernels.hpp"
#include "actor_plan.hpp"
#include "gru_fwd_fused.hpp"
#include "gru_kernels.hpp"
#include "learner_handle.hpp"
#include "optim_host.hpp"

namespace {

// The agent handle: online = target = the agent params (the actor has no target net); its stats land at stats + 8.
int actor_bind(Actor& a, float* agent, float* agent_grad, float* agent_sq, float* stats) {
  a.agent = agent; a.agrad = agent_grad; a.asq = agent_sq;
  return mq_bind(a.ah, agent, agent, agent_grad, agent_sq, stats + 8, nullptr);
}

// Before a step's first launch: the plan's slabs against actor_ws_rows' (`exceeds`: the learner's error text), the
// feed-forward kernels' LDS against the CU's. That LDS is past a launch's default: the attributes are raised once.
int actor_prepare(Actor& a, const ActorPlan& ap, const char* exceeds) {
  const bool grouped = ap.agent == MQ_AGENT_FFN_NS;   // its slabs are per agent (ns_bpa of them), not ffn_blocks
  if (ap.ns_w2 > kNsplitMax || (grouped ? ap.ns_bpa : ap.ffn_blocks) > a.ffn_slabs_max)
    return set_err(MQ_ERR_STATE, exceeds);
  if (ap.agent != MQ_AGENT_FFN && !grouped) return MQ_OK;
  if (ap.ffn_fwd_lds > kFfnActorLdsMax) return set_err(MQ_ERR_ARG, "the feed-forward actor's forward exceeds the LDS");
  const bool wide = ap.width == mq::HW;
  const void* fwd = grouped ? (const void*)ffn_actor_ns_fwd_kernel
                            : wide ? (const void*)ffn_actor_w_fwd_kernel : (const void*)ffn_actor_fwd_kernel;
  const void* bwd = grouped ? (const void*)ffn_actor_ns_bwd_kernel
                            : wide ? (const void*)ffn_actor_w_bwd_kernel : (const void*)ffn_actor_bwd_kernel;
  if (const int rc = lds_fits(fwd, ap.ffn_fwd_lds, grouped ? "ffn_actor_ns_fwd_kernel"
                                                            : wide ? "ffn_actor_w_fwd_kernel" : "ffn_actor_fwd_kernel"))
    return rc;
  if (const int rc = lds_fits(bwd, wide ? kFfnActorWBwdLds : kFfnActorBwdLds,
                              grouped ? "ffn_actor_ns_bwd_kernel" : wide ? "ffn_actor_w_bwd_kernel" : "ffn_actor_bwd_kernel"))
    return rc;
  if (!a.ffn_attr) {   // a handle has one agent kind: these are its two kernels
    MQ_HIP(hipFuncSetAttribute(fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFfnActorLdsMax));
    MQ_HIP(hipFuncSetAttribute(bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFfnActorLdsMax));
    a.ffn_attr = true;
  }
  return MQ_OK;
}

// The grouped forward's argument block over TB rows per agent whose t = 0 is stored step t0 (off: one agent's offsets).
FfnNsFwd ffn_ns_fwd_args(const Dims& d, const Rep& rp, const float* P, int64_t Pa1, const int64_t* off, float* X1,
                         float* Hh, float* Q, float* XIN, int TB, int t0) {
  return FfnNsFwd{d, rp, P, Pa1, off[MQ_P_FC1_W], off[MQ_P_FC1_B], off[MQ_P_FFN_W], off[MQ_P_FFN_B], off[MQ_P_FC2_W],
                  off[MQ_P_FC2_B], X1, Hh, Q, XIN, TB, (TB + FA_ROWS - 1) / FA_ROWS, t0,
                  ffn_actor_w1_resident(d.I) ? 1 : 0};
}

// One step's actor: its plan and the argument blocks its launches take.
struct ActorStep {
  ActorPlan ap;
  Dims d;       // the agent's dims over the T steps the actor unrolls (d.Tp = T)
  Rep rp;       // the actor's episodes
  Lay L;
  Work w;       // the agent handle's workspace, dHo the actor's
  int64_t RT;   // the actor's rows, T R
};

ActorStep make_actor_step(const Actor& a, const ActorPlan& ap, const Rep& rp, int B, int T, int t_stride) {
  const Dims d = mq::make_dims(a.ah->cfg, B, T, t_stride);
  ActorStep st{ap, d, rp, make_lay(a.ah), a.ah->w, (int64_t)T * d.R};
  st.w.dHo = a.dHo;
  if (ap.width == mq::HW) {   // the wide actor's rows are its own: the agent handle's are sized for width H
    st.w.X1 = a.X1w; st.w.Hs = a.Hw; st.w.dP1 = a.dP1w; st.w.slab_fc1 = a.slab_w1;
  }
  return st;
}

// The agent unroll over t < T, online net only: the logits land in w.Q. The feed-forward actor is one launch
// (ffn_actor_fwd_kernel: X1, Hh = w.Hs, the logits and XIN).
int actor_forward(const Actor& a, const ActorStep& st, hipStream_t s) {
  const auto& [ap, d, rp, L, w, RT] = st;
  const int64_t* off = a.y.off;
  const float* Pa = a.agent;
  if (ap.agent == MQ_AGENT_FFN_NS) {   // grid (workgroups per agent, agent): a workgroup loads one agent's weights
    const FfnNsFwd p = ffn_ns_fwd_args(d, rp, Pa, a.Pa1, off, w.X1, w.Hs, w.Q, w.XIN, (int)(RT / d.n), 0);
    hipLaunchKernelGGL(ffn_actor_ns_fwd_kernel, dim3(ap.ns_fpa, d.n), dim3(256), ap.ffn_fwd_lds, s, p);
    MQ_HIP(hipGetLastError());
    return MQ_OK;
  }
  if (ap.agent == MQ_AGENT_FFN && ap.width == mq::HW) {
    const FfnActorWFwd p{d, rp, Pa, off[MQ_P_FC1_W], off[MQ_P_FC1_B], off[MQ_P_FFN_W], off[MQ_P_FFN_B], off[MQ_P_FC2_W],
                         off[MQ_P_FC2_B], w.X1, w.Hs, w.Q, w.XIN, RT, ap.ffn_fwd_tiles, 0};
    hipLaunchKernelGGL(ffn_actor_w_fwd_kernel, dim3(ap.ffn_fwd_blocks), dim3(256), ap.ffn_fwd_lds, s, p);
  } else if (ap.agent == MQ_AGENT_FFN) {
    const FfnActorFwd p{d, rp, Pa, off[MQ_P_FC1_W], off[MQ_P_FC1_B], off[MQ_P_FFN_W], off[MQ_P_FFN_B], off[MQ_P_FC2_W],
                        off[MQ_P_FC2_B], w.X1, w.Hs, w.Q, w.XIN, RT, ap.ffn_tiles, ap.ffn_resident};
    hipLaunchKernelGGL(ffn_actor_fwd_kernel, dim3(ap.ffn_fwd_blocks), dim3(256), ap.ffn_fwd_lds, s, p);
  } else if (ap.fused_fwd) {
    launch_fwd_fused(dim3(d.R, 1), s, d, rp, Pa, Pa, L, w);
  } else {
    Fc1Prob p1{d, rp, Pa, Pa, off[MQ_P_FC1_W], off[MQ_P_FC1_B], w.X1, w.XIN, RT};
    MQ_HIP(launch_gemm(p1, (int)RT, 2 * mq::H, 1, s));
    GiProb p2{w.X1, Pa, Pa, off[MQ_P_RNN_W_IH], off[MQ_P_RNN_B_IH], w.GI, RT};
    MQ_HIP(launch_gemm(p2, (int)RT, mq::G3, 1, s));
    const dim3 grid((d.R + ap.rw_fwd - 1) / ap.rw_fwd, 1);
    const auto fwd = ap.rw_fwd == 1 ? gru_fwd_kernel<1, 0> : ap.rw_fwd == 2 ? gru_fwd_kernel<2, 0>
                     : ap.rw_fwd == 4 ? gru_fwd_kernel<4, 0> : gru_fwd_kernel<8, 0>;
    hipLaunchKernelGGL(fwd, grid, dim3(256), 0, s, d, Pa, Pa, L, w);
  }
  MQ_HIP(hipGetLastError());
  if (ap.agent == MQ_AGENT_FFN || ap.fused_fwd) return MQ_OK;   // the one launch wrote the logits too
  Fc2Prob p3{w.Hs, Pa, Pa, off[MQ_P_FC2_W], off[MQ_P_FC2_B], w.Q, RT, d.A};
  MQ_HIP(launch_gemm(p3, (int)RT, d.A, 1, s));
  return MQ_OK;
}

// From the policy kernel's a.dL [RT][Ap] (dense dLoss/dlogits) and its npol blocks of loss sums a.ppart: BPTT with
// the dense output gradient, the split-K weight gradients, and the two-pass reduction into a.agrad [Pa | MQ_NSUMS];
// *nnorm = the norm partials it left in a.norm_part. The feed-forward actor: ffn_actor_bwd_kernel (dP1 and one
// [dWr | dbr | dW2 | db2] slab per workgroup into a.slab_ffn), the split-K [dW1 | db1], the reduction.
int actor_backward(const Actor& a, const ActorStep& st, int npol, hipStream_t s, int* nnorm) {
  const auto& [ap, d, rp, L, w, RT] = st;
  const Layout* ah = &a.y;
  const float* Pa = a.agent;
  if (ap.agent == MQ_AGENT_FFN_NS) {
    // every (slab, agent) block is written whole: [dWr .. db2] by workgroup (j, g), [dW1 | db1] by slice (g, j)
    const int TB = (int)(RT / d.n);
    const FfnNsBwd p{a.dL, a.Ap, d.A, d.n, Pa, a.Pa1, ah->off[MQ_P_FFN_W], ah->off[MQ_P_FC2_W], w.Hs, w.X1, w.dP1,
                     a.slab_ffn, TB, ap.ns_tpa, ap.ffn_tpb};
    hipLaunchKernelGGL(ffn_actor_ns_bwd_kernel, dim3(ap.ns_bpa, d.n), dim3(256), kFfnActorBwdLds, s, p);
    MQ_HIP(hipGetLastError());
    const FfnNsDw1Prob p2{d.I, w.dP1, w.XIN, a.slab_ffn, a.Pa1, d.n, ap.ns_bpa, TB, ap.ffn_tpb * FA_ROWS};
    MQ_HIP(launch_gemm(p2, mq::H, d.I, d.n * ap.ns_bpa, s));
    return launch_reduce(actor_reduce_plan(ap, *ah, w, a, npol), a.norm_part, "agent", s, nnorm);
  }
  if (ap.agent == MQ_AGENT_FFN && ap.width == mq::HW) {
    const FfnActorWBwd p{a.dL, a.Ap, d.A, Pa + ah->off[MQ_P_FC2_W], Pa + ah->off[MQ_P_FFN_W], w.Hs, w.X1, w.dP1,
                         a.slab_ffn, ah->len_rnn, RT, ap.ffn_tiles, ap.ffn_tpb};
    hipLaunchKernelGGL(ffn_actor_w_bwd_kernel, dim3(ap.ffn_blocks), dim3(256), kFfnActorWBwdLds, s, p);
    MQ_HIP(hipGetLastError());
    // [dW1 | db1] [128][I]: the critic's weight-gradient policy, two row tiles, into Dw1Prob's slab scheme
    const A2cDwProb<128> p2{w.dP1, mq::HW, w.XIN, d.I, d.I, w.slab_fc1, RT, ap.ns_w1};
    MQ_HIP(launch_gemm(p2, mq::HW, d.I, ap.ns_w1, s));
    return launch_reduce(actor_reduce_plan(ap, *ah, w, a, npol), a.norm_part, "agent", s, nnorm);
  }
  if (ap.agent == MQ_AGENT_FFN) {
    const FfnActorBwd p{a.dL, a.Ap, d.A, Pa + ah->off[MQ_P_FC2_W], Pa + ah->off[MQ_P_FFN_W], w.Hs, w.X1, w.dP1,
                        a.slab_ffn, ah->len_rnn, RT, ap.ffn_tiles, ap.ffn_tpb};
    hipLaunchKernelGGL(ffn_actor_bwd_kernel, dim3(ap.ffn_blocks), dim3(256), kFfnActorBwdLds, s, p);
    MQ_HIP(hipGetLastError());
  } else {
    DhoProb p0{a.dL, a.Ap, d.A, Pa + ah->off[MQ_P_FC2_W], w.dHo, RT};
    MQ_HIP(launch_gemm(p0, (int)RT, mq::H, 1, s));
    const size_t dyn = ((size_t)2 * d.A * mq::H + d.A) * sizeof(float);
    const auto bwd = ap.rw_bwd == 1 ? gru_bwd_kernel<1, 0, true> : gru_bwd_kernel<2, 0, true>;
    hipLaunchKernelGGL(bwd, dim3(ap.nblk_bwd), dim3(512), dyn, s, d, rp, Pa, L, w, ah->len_rnn);
    MQ_HIP(hipGetLastError());
    Dx1Prob p1{w.dGI, Pa + ah->off[MQ_P_RNN_W_IH], w.X1, w.dP1, RT};
    MQ_HIP(launch_gemm(p1, (int)RT, mq::H, 1, s));
  }
  Dw1Prob p2{d.I, w.dP1, w.XIN, w.slab_fc1, RT, ap.ns_w1};
  MQ_HIP(launch_gemm(p2, mq::H, d.I, ap.ns_w1, s));
  if (ap.agent != MQ_AGENT_FFN) {
    Dw2Prob p3{a.dL, a.Ap, d.A, w.Hs, a.slab_fc2, RT, ap.ns_w2};
    MQ_HIP(launch_gemm(p3, d.A, mq::H, ap.ns_w2, s));
  }
  return launch_reduce(actor_reduce_plan(ap, *ah, w, a, npol), a.norm_part, "agent", s, nnorm);
}

}  // namespace
