// What the policy-gradient actor of the COMA, actor-critic and PPO learners launches (coma_host.hpp actor_forward /
// actor_backward), decided from the shape without a HIP call. coma_plan and a2c_plan both take their actor items from
// here, so what a plan reports is what the launches read.
#pragma once
#include "ffn_actor_kernels.hpp"
#include "step_plan.hpp"

namespace mq {

struct ActorPlan {
  bool fused_fwd;   // gru_fwd_fused_kernel; else fc1 / gi GEMMs, gru_fwd<rw_fwd>, fc2 GEMM
  int rw_fwd;       // rows per workgroup of gru_fwd<RW>
  int rw_bwd;       // rows per workgroup of gru_bwd<RW> (RW >= 4 spills at 512 threads: capped at 2)
  int nblk_bwd;     // the BPTT's workgroups: slab_rnn slabs
  int ns_w1, ns_w2; // split-K slices of [dW1 | db1] (slab_fc1) and [dW2 | db2] (slab_fc2)
  // the feed-forward actor (ffn_actor_kernels.hpp): the items above but ns_w1 are then unused (0)
  int agent;            // MQ_AGENT_*
  int ffn_tiles;        // 64-row tiles of the RT rows
  int ffn_fwd_blocks;   // ffn_actor_fwd_kernel's grid
  int ffn_blocks;       // ffn_actor_bwd_kernel's workgroups = its slabs
  int ffn_tpb;          // tiles each of them walks (the last one the rest)
  int ffn_resident;     // 1: W1 stays in LDS, 0: streamed in K chunks
  size_t ffn_fwd_lds;   // the forward's dynamic LDS, bytes
};

// Most workgroups (slabs) ffn_actor_bwd_kernel runs over any step with at most RTmax rows: what ma_create allocates.
inline int ffn_actor_blocks_max(int64_t RTmax) {
  return (int)std::min<int64_t>(kFfnActorBlocks, std::max<int64_t>(1, (RTmax + FA_ROWS - 1) / FA_ROWS));
}

// I: the agent's input width; R = B n rows unrolled over T steps, RT = T R. ffn_cap: MQ_PLAN ffn_actor_blocks=<n>
// (0: the default cap), fewer workgroups walking longer runs of tiles: the same sums in another partition.
inline ActorPlan actor_plan(int I, int O, int A, int n, int R, int64_t RT, int agent = MQ_AGENT_GRU, int ffn_cap = 0) {
  ActorPlan p{};
  p.agent = agent;
  p.ns_w1 = split_k_slices(RT, (I + Dw1Prob::BN - 1) / Dw1Prob::BN);
  if (agent == MQ_AGENT_FFN) {
    p.ffn_tiles = (int)((RT + FA_ROWS - 1) / FA_ROWS);
    p.ffn_fwd_blocks = std::max(1, std::min(p.ffn_tiles, kFfnActorFwdBlocks));
    const int cap = ffn_cap > 0 ? std::min(ffn_cap, kFfnActorBlocks) : kFfnActorBlocks;
    p.ffn_tpb = std::max(1, (p.ffn_tiles + cap - 1) / cap);
    p.ffn_blocks = std::max(1, (p.ffn_tiles + p.ffn_tpb - 1) / p.ffn_tpb);
    p.ffn_resident = ffn_actor_w1_resident(I) ? 1 : 0;
    p.ffn_fwd_lds = ffn_actor_fwd_lds_bytes(I);
    return p;
  }
  p.rw_fwd = pick_rw(R, 512);
  p.fused_fwd = p.rw_fwd == 1 && fused_fwd_ok(I, O, A, n, RT);
  p.rw_bwd = std::min(2, pick_rw(R, 256));
  p.nblk_bwd = (R + p.rw_bwd - 1) / p.rw_bwd;
  p.ns_w2 = split_k_slices(RT, 1);
  return p;
}

}  // namespace mq
