// What the policy-gradient actor of the COMA, actor-critic and PPO learners launches (coma_host.hpp actor_forward /
// actor_backward), decided from the shape without a HIP call. coma_plan and a2c_plan both take their actor items from
// here, so what a plan reports is what the launches read.
#pragma once
#include "step_plan.hpp"

namespace mq {

struct ActorPlan {
  bool fused_fwd;   // gru_fwd_fused_kernel; else fc1 / gi GEMMs, gru_fwd<rw_fwd>, fc2 GEMM
  int rw_fwd;       // rows per workgroup of gru_fwd<RW>
  int rw_bwd;       // rows per workgroup of gru_bwd<RW> (RW >= 4 spills at 512 threads: capped at 2)
  int nblk_bwd;     // the BPTT's workgroups: slab_rnn slabs
  int ns_w1, ns_w2; // split-K slices of [dW1 | db1] (slab_fc1) and [dW2 | db2] (slab_fc2)
};

// I: the agent's input width; R = B n rows unrolled over T steps, RT = T R.
inline ActorPlan actor_plan(int I, int O, int A, int n, int R, int64_t RT) {
  ActorPlan p{};
  p.rw_fwd = pick_rw(R, 512);
  p.fused_fwd = p.rw_fwd == 1 && fused_fwd_ok(I, O, A, n, RT);
  p.rw_bwd = std::min(2, pick_rw(R, 256));
  p.nblk_bwd = (R + p.rw_bwd - 1) / p.rw_bwd;
  p.ns_w1 = split_k_slices(RT, (I + Dw1Prob::BN - 1) / Dw1Prob::BN);
  p.ns_w2 = split_k_slices(RT, 1);
  return p;
}

}  // namespace mq
