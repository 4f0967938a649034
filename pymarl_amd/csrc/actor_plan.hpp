// The policy-gradient actor of the COMA, actor-critic and PPO learners without a HIP call: what a handle holds of it
// (Actor), its workspace rows (actor_ws_rows, probe: tests/host/actor_ws_probe.cpp), what a step launches (ActorPlan:
// coma_plan and a2c_plan report it, actor_host.hpp launches from it) and its backward's reduction (actor_reduce_plan).
#pragma once
#include "ffn_actor_ns_kernels.hpp"
#include "ffn_actor_w_kernels.hpp"
#include "reduce_plan.hpp"

namespace mq {

// A learner handle's actor. The agent's own buffers (X1 .. slab_fc1, slab_rnn) are the agent handle's workspace.
struct Actor {
  mq_handle* ah = nullptr;   // the agent's handle (no mixer): config, workspace, kernels; owned by the learner's handle
  // the actor's layout (actor_ws_rows sets it): the agent handle's own, except for the wide feed-forward actor
  // (y.Hd = 128), whose handle stays at width 64 (mq_create takes no other) and lends only Q, XIN and the batch checks
  Layout y;
  float *X1w = nullptr, *Hw = nullptr, *dP1w = nullptr, *slab_w1 = nullptr;   // the wide actor's [RT][128] rows, dW1 slabs
  float *agent = nullptr, *agrad = nullptr, *asq = nullptr;   // bound: parameters, gradient [Pa | MQ_NSUMS], square_avg
  int64_t Pa = 0;      // the agent's parameters
  int Ap = 0;          // dL's pitch: the actions rounded up to 4
  // workspace (actor_ws_rows); slab_ffn [ffn_slabs_max][len_rnn]: the feed-forward actor's slabs
  float *dL, *dHo, *pi, *ppart, *slab_fc2, *slab_ffn, *red_tmp, *norm_part;
  int ffn_slabs_max = 0, ffn_cap = 0;   // slabs slab_ffn holds; MQ_PLAN ffn_actor_blocks (0: the default cap)
  bool ffn_attr = false;   // the two ffn_actor kernels' dynamic-LDS attributes are raised
  // the non-shared actor (MQ_AGENT_FFN_NS): ns agents of Pa1 parameters each, Pa = ns Pa1, and slab_ffn holds
  // ffn_slabs_max whole-gradient slabs [ns][Pa1]. 0: one shared agent
  int ns = 0;
  int64_t Pa1 = 0;
};

struct ActorPlan {
  bool fused_fwd;   // gru_fwd_fused_kernel; else fc1 / gi GEMMs, gru_fwd<rw_fwd>, fc2 GEMM
  int rw_fwd;       // rows per workgroup of gru_fwd<RW>
  int rw_bwd;       // rows per workgroup of gru_bwd<RW> (RW >= 4 spills at 512 threads: capped at 2)
  int nblk_bwd;     // the BPTT's workgroups: slab_rnn slabs
  int ns_w1, ns_w2; // split-K slices of [dW1 | db1] (slab_fc1) and [dW2 | db2] (slab_fc2)
  // the feed-forward actor (ffn_actor_kernels.hpp): the items above but ns_w1 are then unused (0)
  int agent;            // MQ_AGENT_*
  int width;            // the agent's hidden width: H, or HW (ffn_actor_w_kernels.hpp; MQ_AGENT_FFN only)
  int ffn_tiles;        // the backward's tiles of the RT rows: 64-row, or at width HW 32-row (FWB_ROWS)
  int ffn_fwd_tiles;    // the forward's 64-row tiles
  int ffn_fwd_blocks;   // ffn_actor_fwd_kernel's grid
  int ffn_blocks;       // ffn_actor_bwd_kernel's workgroups = its slabs
  int ffn_tpb;          // tiles each of them walks (the last one the rest)
  int ffn_resident;     // 1: W1 stays in LDS, 0: streamed in K chunks
  size_t ffn_fwd_lds;   // the forward's dynamic LDS, bytes
  // the non-shared actor (ffn_actor_ns_kernels.hpp), per agent; then ffn_tiles = n ns_tpa, ffn_blocks = n ns_bpa,
  // ffn_fwd_blocks = n ns_fpa, ffn_tpb tiles per backward workgroup, and ns_w1 = ns_bpa
  int ns_tpa;   // 64-row tiles of an agent's T B rows
  int ns_bpa;   // the backward's workgroups per agent = gradient slabs = dW1 slices per agent
  int ns_fpa;   // the forward's workgroups per agent
};

// Most backward workgroups per agent (gradient slabs) of the non-shared actor over any step of at most TBmax = T B
// rows per agent: what slab_ffn holds. MQ_PLAN ffn_actor_blocks only lowers it.
inline int ffn_ns_bpa_max(int64_t TBmax, int n) {
  return (int)std::min<int64_t>(std::max(1, kFfnActorBlocks / n), std::max<int64_t>(1, (TBmax + FA_ROWS - 1) / FA_ROWS));
}

// Most workgroups (slabs) ffn_actor_bwd_kernel runs over any step with at most RTmax rows: what slab_ffn holds.
// rows: the backward's tile height (FWB_ROWS for the wide actor).
inline int ffn_actor_blocks_max(int64_t RTmax, int rows = FA_ROWS) {
  return (int)std::min<int64_t>(kFfnActorBlocks, std::max<int64_t>(1, (RTmax + rows - 1) / rows));
}

// I: the agent's input width; R = B n rows unrolled over T steps, RT = T R. ffn_cap: MQ_PLAN ffn_actor_blocks=<n>
// (0: the default cap), fewer workgroups walking longer runs of tiles: the same sums in another partition.
// width: the agent's hidden width (HW: MQ_AGENT_FFN's wide kernels; [dW1 | db1] then has two row tiles).
inline ActorPlan actor_plan(int I, int O, int A, int n, int R, int64_t RT, int agent = MQ_AGENT_GRU, int ffn_cap = 0,
                            int width = H) {
  ActorPlan p{};
  p.agent = agent;
  p.width = width;
  p.ns_w1 = split_k_slices(RT, (width / H) * ((I + Dw1Prob::BN - 1) / Dw1Prob::BN));
  if (agent == MQ_AGENT_FFN_NS) {   // grouped: every figure per agent, over its TB = RT / n rows
    const int64_t TB = RT / n;
    const int cap = ffn_cap > 0 ? std::min(ffn_cap, kFfnActorBlocks) : kFfnActorBlocks;
    p.ns_tpa = (int)std::max<int64_t>(1, (TB + FA_ROWS - 1) / FA_ROWS);
    p.ffn_tpb = (p.ns_tpa + std::max(1, cap / n) - 1) / std::max(1, cap / n);
    p.ns_bpa = (p.ns_tpa + p.ffn_tpb - 1) / p.ffn_tpb;   // every workgroup, and so every dW1 slice, has a tile
    p.ns_fpa = std::min(p.ns_tpa, std::max(1, kFfnActorFwdBlocks / n));
    p.ns_w1 = p.ns_bpa;
    p.ffn_tiles = n * p.ns_tpa;
    p.ffn_blocks = n * p.ns_bpa;
    p.ffn_fwd_blocks = n * p.ns_fpa;
    p.ffn_resident = ffn_actor_w1_resident(I) ? 1 : 0;
    p.ffn_fwd_lds = ffn_actor_fwd_lds_bytes(I);
    return p;
  }
  if (agent == MQ_AGENT_FFN) {
    const bool wide = width == HW;   // its W1 is always streamed, its LDS the same whatever I is
    const int rows = wide ? FWB_ROWS : FA_ROWS;
    p.ffn_tiles = (int)((RT + rows - 1) / rows);
    p.ffn_fwd_tiles = (int)((RT + FA_ROWS - 1) / FA_ROWS);
    p.ffn_fwd_blocks = std::max(1, std::min(p.ffn_fwd_tiles, kFfnActorFwdBlocks));
    const int cap = ffn_cap > 0 ? std::min(ffn_cap, kFfnActorBlocks) : kFfnActorBlocks;
    p.ffn_tpb = std::max(1, (p.ffn_tiles + cap - 1) / cap);
    p.ffn_blocks = std::max(1, (p.ffn_tiles + p.ffn_tpb - 1) / p.ffn_tpb);
    p.ffn_resident = !wide && ffn_actor_w1_resident(I) ? 1 : 0;
    p.ffn_fwd_lds = wide ? kFfnActorWFwdLds : ffn_actor_fwd_lds_bytes(I);
    return p;
  }
  p.rw_fwd = pick_rw(R, 512);
  p.fused_fwd = p.rw_fwd == 1 && fused_fwd_ok(I, O, A, n, RT);
  p.rw_bwd = std::min(2, pick_rw(R, 256));
  p.nblk_bwd = (R + p.rw_bwd - 1) / p.rw_bwd;
  p.ns_w2 = split_k_slices(RT, 1);
  return p;
}

// The internal agent handle's config (no mixer) from a COMA or an actor-critic config `c`; `agent`: MQ_AGENT_*.
template <class C>
mq_config agent_config(const C& c, float gamma, int agent = MQ_AGENT_GRU) {
  mq_config a{};
  a.n_agents = c.n_agents; a.n_actions = c.n_actions; a.obs_dim = c.obs_dim; a.state_dim = c.state_dim;
  a.rnn_hidden_dim = c.rnn_hidden_dim; a.mixer = MQ_MIXER_NONE;
  a.obs_last_action = c.obs_last_action; a.obs_agent_id = c.obs_agent_id; a.gamma = gamma; a.lr = c.lr;
  a.optim_alpha = c.optim_alpha; a.optim_eps = c.optim_eps; a.grad_norm_clip = c.grad_norm_clip;
  a.max_batch = c.max_batch; a.max_seq = c.max_seq;
  a.agent = agent == MQ_AGENT_FFN_NS ? MQ_AGENT_FFN : agent;   // the handle lends one agent's layout
  return a;
}

// The actor's rows of a learner's workspace table, for the agent layout y and steps of at most RTmax = T R rows; the
// capacities they give land in `a` with the pointers.
// ns > 0: the non-shared actor of ns agents (y is then one agent's layout): slab_ffn holds whole-gradient slabs and
// red_tmp the partials of the one region they make.
// y.Hd = HW (the wide feed-forward actor: y is then its own layout, not the agent handle's): the rows X1w, Hw, dP1w
// [RTmax][HW] and slab_w1, the [dW1 | db1] slabs, follow, since the agent handle's are sized for width H.
inline WsTable actor_ws_rows(Actor& a, int A, const Layout& y, int64_t RTmax, int ns = 0) {
  const int64_t Hd = y.Hd, l1 = Hd * y.I + Hd, l2 = (int64_t)A * Hd + A;
  const bool wide = Hd == HW;
  a.y = y;
  a.ns = ns;
  a.Pa1 = y.P;
  a.Pa = ns > 0 ? ns * y.P : y.P;
  a.Ap = (A + 3) & ~3;
  a.ffn_slabs_max = ns > 0 ? ffn_ns_bpa_max(RTmax / ns, ns)
                           : y.ffn ? ffn_actor_blocks_max(RTmax, wide ? FWB_ROWS : FA_ROWS) : 0;
  const int64_t slab_len = ns > 0 ? a.Pa : y.len_rnn;
  // pass 1's partials: at most kRedZ groups of each region's length (RedBuilder::add). GRU: [dW1 | db1], the BPTT
  // slabs' W_ih .. b_hh prefix (shorter than len_rnn), [dW2 | db2], the loss sums. Feed-forward: [dW1 | db1], the whole
  // len_rnn of a [dWr | dbr | dW2 | db2] slab, the loss sums, and no region of fc2's own: the one sum covers both
  const int64_t red_tmp = kRedZ * (ns > 0 ? a.Pa + MQ_NSUMS : l1 + y.len_rnn + l2 + MQ_NSUMS);
  WsTable rows = {
      {"dL", RTmax * a.Ap, &a.dL}, {"dHo", RTmax * H, &a.dHo}, {"pi", RTmax * A, &a.pi},
      {"ppart", ((RTmax + 3) / 4) * MQ_NSUMS, &a.ppart},
      {"slab_fc2", kNsplitMax * l2, &a.slab_fc2},
      {"slab_ffn", a.ffn_slabs_max * slab_len, &a.slab_ffn},
      {"red_tmp", red_tmp, &a.red_tmp},
      {"norm_part", kNormPartMax, &a.norm_part},
  };
  if (wide)
    rows.insert(rows.end(), {{"X1w", RTmax * Hd, &a.X1w}, {"Hw", RTmax * Hd, &a.Hw}, {"dP1w", RTmax * Hd, &a.dP1w},
                             {"slab_w1", kNsplitMax * l1, &a.slab_w1}});
  return rows;
}

// The regions of the actor's backward into a.agrad [Pa | MQ_NSUMS], from the policy kernel's npol blocks of loss sums
// and the slabs the plan's launches leave in `w` (the agent handle's workspace) and `a`. No launch, as plan_reduce.
inline RedBuilder actor_reduce_plan(const ActorPlan& p, const Layout& y, const Work& w, const Actor& a, int npol) {
  RedBuilder rb(a.red_tmp);
  if (p.agent == MQ_AGENT_FFN_NS) {   // one region: ns_bpa slabs, each the whole gradient [n][Pa1]
    rb.add(a.slab_ffn, p.ns_bpa, a.Pa, a.agrad, true);
    rb.add(a.ppart, npol, MQ_NSUMS, a.agrad + a.Pa, false);
    return rb;
  }
  // (the wide actor: `w` is its step's view, whose slab_fc1 is a.slab_w1)
  rb.add(w.slab_fc1, p.ns_w1, (int64_t)y.Hd * y.I + y.Hd, a.agrad + y.off[MQ_P_FC1_W], true);
  if (p.agent == MQ_AGENT_FFN) {   // one slab per workgroup of ffn_actor_bwd_kernel
    rb.add(a.slab_ffn, p.ffn_blocks, y.len_rnn, a.agrad + y.off[MQ_P_FFN_W], true);
  } else {
    // W_ih .. b_hh: the prefix of each BPTT slab; its fc2 part (unused in the dense-dy mode) is as long as fc2's slab
    const int64_t pre = y.off[MQ_P_FC2_W] - y.off[MQ_P_RNN_W_IH];
    rb.add(w.slab_rnn, p.nblk_bwd, pre, a.agrad + y.off[MQ_P_RNN_W_IH], true, y.len_rnn);
    rb.add(a.slab_fc2, p.ns_w2, y.len_rnn - pre, a.agrad + y.off[MQ_P_FC2_W], true);
  }
  rb.add(a.ppart, npol, MQ_NSUMS, a.agrad + a.Pa, false);
  return rb;
}

}  // namespace mq
