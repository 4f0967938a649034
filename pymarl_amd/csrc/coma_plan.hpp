// What one COMA train step launches (include/mc_coma.h), decided from the config, the batch's shape, the CU count
// and the step's mode without a HIP call and without a getenv: the critic's widths and grids, whether the persistent
// chain and the actor's side stream run, the dynamic-LDS sizes, and the actor's shard and plan. mc_train_step launches
// from it (coma_host.hpp), mc_create sizes the workspace from the same functions, and tests/host/coma_plan_probe.cpp
// prints it.
#pragma once
#include "../../include/mc_coma.h"
#include "actor_plan.hpp"
#include "coma_chain.hpp"

namespace mq {

constexpr size_t kComaLdsMax = 160 * 1024;   // dynamic LDS a COMA kernel may ask for

// Critic input width (coma.py:61-70): state | obs | n A actions | n A last actions | agent id.
inline int coma_k(const mc_config& c) { return c.state_dim + c.obs_dim + 2 * c.n_agents * c.n_actions + c.n_agents; }

inline CDims coma_dims(const mc_config& c, int B, int t_len, int t_stride) {
  CDims d{};
  d.n = c.n_agents; d.A = c.n_actions; d.O = c.obs_dim; d.S = c.state_dim;
  d.Kc = coma_k(c); d.Kp = (d.Kc + 3) & ~3;
  d.R = B * c.n_agents; d.B = B; d.Tp = t_len; d.T = t_len - 1; d.t_stride = t_stride;
  d.lg = (float)((double)c.td_lambda * (double)c.gamma);
  d.og = (float)((1.0 - (double)c.td_lambda) * (double)c.gamma);
  d.dR = make_fastdiv((uint32_t)d.R);
  d.dN = make_fastdiv((uint32_t)d.n);
  return d;
}

// Offsets of fc1.weight .. fc3.bias (MC_P_* order); off[MC_P_COUNT] = the parameter count.
inline void mc_offsets(const mc_config& c, int64_t* off) {
  const int64_t A = c.n_actions;
  const int64_t sz[MC_P_COUNT] = {(int64_t)CH * coma_k(c), CH, (int64_t)CH * CH, CH, A * CH, A};
  int64_t o = 0;
  for (int i = 0; i < MC_P_COUNT; ++i) { off[i] = o; o += sz[i]; }
  off[MC_P_COUNT] = o;
}

// The grids the workspace is sized by: head blocks of R rows, wgrad blocks, and H1p's slices (the three-launch l1's K
// slices or the chain's phase-A owners, whichever is more).
inline int coma_heads(int R) { return (R + 15) / 16; }
inline int coma_wgrad_blocks(int Kc, int A) {
  CDims d{};
  d.Kc = Kc; d.A = A;
  return wgrad_blocks(d);
}
inline int coma_h1p_slices(int Kc) { return std::max(l1_slices((Kc + 3) & ~3), cc_nk(Kc)); }

// How the step runs, read by the caller where each switch is documented to be read (switches.hpp): exchange /
// replicated from the data-parallel setting and the actor shard, timing from mc_set_timing, chain_enabled from MQ_PLAN
// coma_chain at mc_create (cleared by a refused chain launch), overlap_enabled from MQ_PLAN coma_overlap per train().
struct ComaMode {
  bool exchange, replicated, timing, chain_enabled, overlap_enabled;
  int shard_lo, shard_hi;
};

struct ComaPlan {
  // critic: input width and its pitch, rows of a step, steps, l1's K slices, head / wgrad blocks, the chain's phase-A
  // owners and grid
  int Kc, Kp, R, T, KS, nhead, nwgrad, NK, NG;
  bool chain;     // every critic step in one persistent launch (cc_ok, and the mode allows it)
  bool overlap;   // the actor's forward on the side stream beside the chain
  size_t lds_td, lds_l1, lds_head, lds_chain;
  // actor: its episodes (the shard under a replicated critic), rows B n and T B n, its first row in the critic's
  // [T][R][A] Q values, the policy kernel's blocks
  int actor_B, actor_R, qv_r0, npol;
  int64_t actor_rows;
  ActorPlan actor;
  const char* refused;   // the limit a refused shape broke (the error's text), else nullptr
};

inline ComaPlan coma_plan(const mc_config& c, int B, int t_len, int num_cu, const ComaMode& m) {
  ComaPlan p{};
  const int n = c.n_agents, A = c.n_actions, A16 = (A + 15) / 16 * 16;
  p.Kc = coma_k(c);
  p.Kp = (p.Kc + 3) & ~3;
  p.R = B * n;
  p.T = t_len - 1;
  p.KS = l1_slices(p.Kp);
  p.nhead = coma_heads(p.R);
  p.nwgrad = coma_wgrad_blocks(p.Kc, A);
  p.NK = cc_nk(p.Kc);
  p.NG = 8 * p.NK;
  // exchange mode sums every critic step over the ranks: no chain. num_cu <= 0 (the device query failed): cc_ok says no
  p.chain = !m.exchange && m.chain_enabled && cc_ok(p.R, A, p.Kc, num_cu);
  p.overlap = p.chain && !m.timing && m.overlap_enabled;
  p.lds_td = (size_t)t_len * (n + 3) * sizeof(float);
  p.lds_l1 = (size_t)(16 + kL1Rows) * (KW + 1) * sizeof(float);
  p.lds_head = ((size_t)(CH + A16 + 48) * (CH + 1) + 16 * (A16 + 1) + CH + A16) * sizeof(float);
  p.lds_chain = cc_lds_bytes(A);
  if (p.lds_td > kComaLdsMax || n > 256) p.refused = "episode too long for the LDS TD(lambda) pass";
  else if (p.lds_l1 > kComaLdsMax || p.lds_head > kComaLdsMax)
    p.refused = "critic input width or n_actions too large for the LDS-staged critic step";
  p.actor_B = m.replicated ? m.shard_hi - m.shard_lo : B;
  p.actor_R = p.actor_B * n;
  p.actor_rows = (int64_t)p.T * p.actor_R;
  p.qv_r0 = m.replicated ? m.shard_lo * n : 0;
  p.npol = (int)((p.actor_rows + 3) / 4);
  const int I = c.obs_dim + (c.obs_last_action ? A : 0) + (c.obs_agent_id ? n : 0);
  p.actor = actor_plan(I, c.obs_dim, A, n, p.actor_R, p.actor_rows);
  return p;
}

}  // namespace mq
