// What one actor-critic train step launches (include/ma_a2c.h), decided from the config and the batch's shape without
// a HIP call: the critic's input width, the grids and the split-K slices. ma_train_step launches from it, ma_create
// sizes the workspace from its upper bounds, and tests/host/a2c_plan_probe.cpp prints it.
#pragma once
#include "../../include/ma_a2c.h"
#include "actor_plan.hpp"

namespace mq {

constexpr int A2C_DV_ROWS = 64;          // rows per workgroup of a2c_dv_kernel (one fc3-gradient slab each)
constexpr size_t kA2cNstepLdsMax = 64 * 1024;   // a2c_nstep_kernel's dynamic LDS without raising the kernel's attribute

// Critic input width: cv = state | n A last-action one-hots (obs_last_action) | agent id; ac = obs | agent id.
inline int a2c_k(const ma_config& c) {
  if (c.critic_type == MA_CRITIC_AC) return c.obs_dim + c.n_agents;
  return c.state_dim + (c.obs_last_action ? c.n_agents * c.n_actions : 0) + c.n_agents;
}

inline size_t a2c_nstep_lds_bytes(int Tp, int n) { return (size_t)Tp * (n + 2) * sizeof(float); }

// Upper bound of the split-K slices of any step with at most RTmax rows (ffn_wr_ns_max's bound: split_k_slices only
// ever rounds this number down).
inline int a2c_ns_max(int64_t RTmax) { return (int)std::min<int64_t>(kNsplitMax, std::max<int64_t>(1, RTmax / 256)); }

// `actor`, when given, receives the ActorPlan the actor's launches read: ns_aw1 / ns_aw2 / bwd_blocks report it.
inline ma_plan a2c_plan(const ma_config& c, int B, int t_len, bool reward_norm, bool adam, ActorPlan* actor = nullptr) {
  ma_plan p{};
  const int R = B * c.n_agents, T = t_len - 1;
  const int64_t RT = (int64_t)T * R;
  p.rows = (int32_t)RT;
  p.rows_target = (int32_t)((int64_t)t_len * R);
  p.k = a2c_k(c);
  p.kp = (p.k + 3) & ~3;
  p.hidden = c.critic_hidden;
  p.vec16 = p.k % 4 == 0 ? 1 : 0;   // X's pitch kp is always a multiple of 4; W1's rows are 16-byte aligned when k is
  p.fwd_tiles = (p.rows_target + GBM - 1) / GBM;
  p.vhead_blocks = (int32_t)(((int64_t)p.rows_target + RT + 3) / 4);
  p.nstep_lds = (int32_t)a2c_nstep_lds_bytes(t_len, c.n_agents);
  p.dv_blocks = (int32_t)((RT + A2C_DV_ROWS - 1) / A2C_DV_ROWS);
  p.ns_cw2 = split_k_slices(RT, (c.critic_hidden / 64) * (c.critic_hidden / 64));
  p.ns_cw1 = split_k_slices(RT, (c.critic_hidden / 64) * ((p.k + 127) / 128));
  p.policy_blocks = (int32_t)((RT + 3) / 4);
  p.policy_tail = (int32_t)(RT % 4);
  p.policy_lanes = c.n_actions;
  p.ap = (c.n_actions + 3) & ~3;
  const int I = c.obs_dim + (c.obs_last_action ? c.n_actions : 0) + (c.obs_agent_id ? c.n_agents : 0);
  const ActorPlan ap = actor_plan(I, c.obs_dim, c.n_actions, c.n_agents, R, RT);
  if (actor) *actor = ap;
  p.ns_aw1 = ap.ns_w1;
  p.ns_aw2 = ap.ns_w2;
  p.bwd_blocks = ap.nblk_bwd;
  p.reward_norm = reward_norm ? 1 : 0;
  p.adam = adam ? 1 : 0;
  return p;
}

}  // namespace mq
