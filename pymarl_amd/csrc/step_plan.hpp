// Which kernels one QMIX / VDN / IQL train step runs: a pure function of the config, the batch shape, the MQ_PLAN
// overrides and the CU count (plan_step), decided before the step's first launch. No HIP call, no handle:
// tests/host/plan_probe.cpp answers "which plan does this shape get" on a machine without a GPU. The eligibility
// predicates stay in the kernel headers beside the constants they depend on.
#pragma once
#include <algorithm>

#include "learner_gemms.hpp"
#include "gru_fwd_fused.hpp"
#include "gru_fwd_pair.hpp"
#include "gru_bwd_fused.hpp"
#include "gru_tiles.hpp"
#include "mix_kernels.hpp"
#include "hyper_kernel.hpp"
#include "dwh_kernel.hpp"
#include "optim_kernels.hpp"
#include "ffn_kernels.hpp"
#include "switches.hpp"

namespace mq {

constexpr int kNsplitMax = 128;
// rows up to which the fused BPTT (one row per workgroup, one workgroup per CU) is used: past the CU count the rows
// run as a second wave of workgroups, which still beats gru_bwd<2> + dX1 + dW1 at configs[3]'s shard (R = 320;
// round 3)
constexpr int kFusedBwdRmax = 512;

// The MQ_PLAN items of this learner (switches.hpp; A/B runs and tests). -1: the default rule decides.
struct PlanOverrides {
  bool unfused_fwd = false;   // the unfused forward (GEMMs around gru_fwd<RW>)
  bool unfused_bwd = false;   // the unfused BPTT (gru_bwd<RW> + dX1 / dW1 GEMMs)
  // the row-tile MFMA forward / BPTT (gru_tiles.hpp) for batches past the one-row fused kernels (R > 512 rows);
  // row_tiles=1 forces it on any batch it can take (tests), =0 turns it off (A/B: the unfused GEMM path)
  int row_tiles = -1;
  // QMIX hypernet workgroups appended to the fused forward's grid (gru_fwd_fused.hpp hyper_fwd_body) when the
  // forward's 2R row-nets exceed two per CU: its second wave leaves CUs idle, and the hypernet fills them
  // (configs[3]'s shard, R = 320: 0.364 -> 0.346 ms a step). hyp_in_fwd=0 never appends (and launches hyper_ws_kernel
  // after the row-pair forward instead of running the hypernet inside it), =1 always (HYP bitwise the same either way)
  int hyp_in_fwd = -1;
  // dW_hyper's tiles appended to the fused BPTT's grid (gru_bwd_fused.hpp, DWH = 1) when its rows exceed the CUs
  // (a second wave of rows leaves CUs idle); dwh_in_bwd=0 never, =1 always (bitwise either way)
  int dwh_in_bwd = -1;
  // m-slices of the dW_hyper pass (A/B at cfg2, DESIGN §3: 4 / 8 / 16 / 32 -> 238.5 / 235.1 / 236.3 / 237.4 us)
  int dwh_split = 8;
  // the row-pair forward (gru_fwd_pair.hpp: both nets of a row in one workgroup, one per CU) when the rows fit one
  // wave of workgroups; fwd_pair=0 keeps the one-row-net kernel, =1 forces the pair
  int fwd_pair = -1;
  // the fused BPTT's lean per-step path (gru_bwd_fused.hpp LEAN) behind the row-pair forward; bwd_lean=0 keeps the
  // classic step (bitwise the same results)
  int bwd_lean = -1;
  bool pair_hyp_epi = false;   // the pair forward's hypernet as its epilogue, not on waves 4 / 5
  bool mix_generic = false;    // mix_kernel<false> where mix_kernel<true> (staged selection rows) would run
  // the TD(lambda) passes of the mixer tail (td_lambda_kernel.hpp) even at cfg.td_lambda = 0, where they compute the
  // one-step target through the scan
  bool lambda_path = false;
  // feed-forward agent: the most workgroups of ffn_dp2_kernel (ffn_dp2_blocks=<n>, 1 .. kFfnDp2Blocks; 0: the default
  // cap). Fewer workgroups walk longer runs of rows: the same sums in another slab partition (tests, A/B runs)
  int ffn_dp2_blocks = 0;
};

// The one read of MQ_PLAN per handle (mq_create).
inline PlanOverrides read_plan_overrides() {
  PlanOverrides o;
  o.unfused_fwd = plan_flag("unfused_fwd");
  o.unfused_bwd = plan_flag("unfused_bwd");
  o.row_tiles = plan_int("row_tiles", -1);
  o.hyp_in_fwd = plan_int("hyp_in_fwd", -1);
  o.dwh_in_bwd = plan_int("dwh_in_bwd", -1);
  o.dwh_split = plan_int("dwh_split", 8);
  o.fwd_pair = plan_int("fwd_pair", -1);
  o.bwd_lean = plan_int("bwd_lean", -1);
  o.pair_hyp_epi = plan_flag("pair_hyp_epi");
  o.mix_generic = plan_flag("mix_generic");
  o.lambda_path = plan_int("lambda_path", 0) != 0;
  o.ffn_dp2_blocks = plan_int("ffn_dp2_blocks", 0);
  return o;
}

// Shapes of a batch of B episodes unrolled over t_len steps under config c.
inline Dims make_dims(const mq_config& c, int B, int t_len, int t_stride) {
  Dims d;
  d.n = c.n_agents; d.A = c.n_actions; d.O = c.obs_dim; d.S = c.state_dim;
  d.E = c.mixer == MQ_MIXER_QMIX ? c.mixing_embed_dim : 0;
  d.I = c.obs_dim + (c.obs_last_action ? c.n_actions : 0) + (c.obs_agent_id ? c.n_agents : 0);
  d.NH = d.E * (c.n_agents + 3);
  d.B = B; d.Tp = t_len; d.T = t_len - 1; d.R = d.B * d.n; d.M = d.T * d.B;
  d.t_stride = t_stride;
  d.last_action = c.obs_last_action; d.agent_id = c.obs_agent_id; d.mixer = c.mixer; d.double_q = c.double_q;
  d.gamma = c.gamma;
  d.huber = c.huber_delta;
  d.dR = make_fastdiv((uint32_t)d.R);
  d.dN = make_fastdiv((uint32_t)d.n);
  d.dB = make_fastdiv((uint32_t)d.B);
  d.dO = make_fastdiv((uint32_t)d.O);
  d.dI = make_fastdiv((uint32_t)d.I);
  d.dS = make_fastdiv((uint32_t)std::max(d.S, 1));
  return d;
}

inline int pick_rw(int R, int max_blocks) {
  const int rws[4] = {1, 2, 4, 8};
  for (int i = 0; i < 4; ++i)
    if ((R + rws[i] - 1) / rws[i] <= max_blocks) return rws[i];
  return 8;
}

enum FwdKind {
  FWD_UNFUSED,   // fc1 / gi GEMMs, gru_fwd<rw_fwd>, fc2 GEMM
  FWD_ONE_ROW,   // gru_fwd_fused_kernel: one row-net per workgroup
  FWD_PAIR,      // gru_fwd_pair_kernel: both nets of a row per workgroup, one per CU
  FWD_TILES,     // gru_fwd_tile_kernel<kq1>: 32-row tiles (with gru_bwd_split_kernel<kq1> as the BPTT)
};
enum HypPlace {
  HYP_ABSENT,       // no QMIX mixer
  HYP_OWN_LAUNCH,   // after the forward: hyper_ws_kernel / hyper_kernel / the GEMM, as StepPlan::hyper says
  HYP_FWD_GRID,     // workgroups appended to the one-row forward's grid
  HYP_PAIR_WAVES,   // inside the pair kernel on waves 4 / 5
  HYP_PAIR_EPI,     // the pair kernel's epilogue
};

// Everything a step decides before its first launch.
struct StepPlan {
  int fwd = FWD_UNFUSED;   // FwdKind
  int rw_fwd = 1;          // rows per workgroup of gru_fwd<RW> (FWD_UNFUSED)
  int kq1 = 0;             // the tile kernels' K-quads of the obs block (FWD_TILES)
  bool fused_bwd = false;  // gru_bwd_fused_kernel; else the split-tile BPTT (FWD_TILES) or gru_bwd<rw_bwd> + dX1 + dW1
  int rw_bwd = 1;
  bool lean = false;       // the fused BPTT's lean per-step path
  int rec_coef = 0;        // Work::rec_coef: the pair forward writes the coefficient record the lean path reads
  int hyp_place = HYP_ABSENT;   // HypPlace
  int hyper = MQ_HYP_NONE;      // MQ_HYP_*: the hypernet kernel
  int mix = MQ_MIX_GENERIC;     // MQ_MIX_*: the mixer tail's kernel
  bool lambda = false;          // the tail runs as the TD(lambda) passes
  bool per = false;             // prioritized replay: the loss-bearing pass in its PER form, then per_priority_kernel
  // dW_hyper (QMIX): tiles appended to the fused BPTT's grid, or fused with pass 1 of the reduction; tj x ts output
  // tiles in ns m-slices, ndwh tiles in all
  bool dwh_in_bwd = false, dwh_in_red1 = false;
  int tj = 0, ts = 0, ns = 0, ndwh = 0;
  // QMIX with the two-layer hypernet (hyper2_kernels.hpp): layer 1 and layer 2 forward as launches of their own
  // before the mixer tail, layer 2 backward and the weight gradients (ns m-slices into slab_mix) after it
  bool hyper2 = false;
  int hyper_layers = 0;   // what mq_last_hyper_layers returns: 2 (hyper2), 1 (the one-layer hypernet), 0 (no QMIX mixer)
  int dw1_ns = 1;     // split-K slices of the dW1 GEMM (unfused BPTT)
  int nblk_mix = 1;   // the mixer tail's workgroups: slab_v2 / loss_part slabs
  int nblk_bwd = 1;   // the BPTT's workgroups: slab_rnn slabs
  int nsplit_fc1 = 1, nsplit_mix = 1;   // slab_fc1 / slab_mix slabs
  // the feed-forward agent (mq_config.agent = MQ_AGENT_FFN, ffn_kernels.hpp): the forward and the backward are the
  // GEMM chain; fwd / fused_bwd / rw_* / lean above are then unused. ffn_wr_ns: split-K slices of [dWr | dbr];
  // ffn_nblk2 workgroups of ffn_dp2_kernel own ffn_rpb rows each (the fc2-gradient slabs)
  bool ffn = false;
  int ffn_wr_ns = 1, ffn_nblk2 = 1, ffn_rpb = FFN_DP2_STEP;
  int agent_report = 0;   // what mq_last_agent returns
  mq_plan report{};   // what mq_last_plan returns
};

// Split-K slices of a weight-gradient GEMM with `ntile` output tiles over RT rows: enough workgroups to fill the
// device, every slice non-empty under krange_split's GBK rounding.
inline int split_k_slices(int64_t RT, int ntile) {
  int ns = (int)std::min<int64_t>(kNsplitMax, std::max<int64_t>(1, RT / 256));
  ns = std::max(1, std::min(ns, (512 + ntile - 1) / ntile));
  const int64_t chunk = ((RT + ns - 1) / ns + GBK - 1) / GBK * GBK;
  return (int)((RT + chunk - 1) / chunk);
}

// most workgroups (fc2-gradient slabs) of ffn_dp2_kernel: a workgroup walks its rows four at a time, each round a
// dependent chain of loads (episode id -> action, dchosen, Hh), so the launch is as long as the longest walk. At the
// cfg2 shape (30,976 rows) 1024 leave 8 rounds each (24 us; a cap of 256, 31 rounds, measured 40 us), and the slabs
// of A * 65 floats are summed by reduction pass 1 in the launch it shares with dW_hyper
constexpr int kFfnDp2Blocks = 1024;
// Upper bounds of a handle's feed-forward slabs from its largest batch (mq_create's workspace): the [dWr | dbr]
// split-K slices and ffn_dp2_kernel's workgroups of any step with at most RTmax rows.
inline int ffn_wr_ns_max(int64_t RTmax) { return (int)std::min<int64_t>(kNsplitMax, std::max<int64_t>(1, RTmax / 256)); }
inline int ffn_nblk2_max(int64_t RTmax) {
  return (int)std::min<int64_t>(kFfnDp2Blocks, (RTmax + FFN_DP2_STEP - 1) / FFN_DP2_STEP);
}

// The mixer tail's kernel (MQ_MIX_*): the same for either agent kind.
inline int pick_mix(const Dims& d, const PlanOverrides& o) {
  const bool fast = d.n <= 16 && d.E <= 64;   // mix_kernel serves the rest (n > 16 or A > 32)
  const bool stream = mix_stream_ok(d.n, d.A) && !o.mix_generic;
  return fast && d.A <= 16 ? MQ_MIX_FAST16 : fast && d.A <= 32 ? MQ_MIX_FAST32 : stream ? MQ_MIX_STREAM : MQ_MIX_GENERIC;
}

inline StepPlan plan_step(const mq_config& c, const PlanOverrides& o, const Dims& d, bool inline_ids,
                          bool have_lambda_ws, int num_cu, bool per = false, int hyper_layers = 1,
                          int agent = MQ_AGENT_GRU) {
  StepPlan p;
  const int64_t RT = (int64_t)d.Tp * d.R;
  const bool qmix = c.mixer == MQ_MIXER_QMIX;
  if (agent == MQ_AGENT_FFN) {
    // No chain over t, so none of the recurrence's choices exists. The hypernet is a launch of its own, dW_hyper rides
    // with reduction pass 1, and the mixer tail is chosen as for the GRU: it meets the agent through Q and dQ/dchosen.
    const bool hyper2 = qmix && hyper_layers == 2;
    p.ffn = true;
    p.agent_report = 1;
    if (qmix) {
      p.hyp_place = HYP_OWN_LAUNCH;
      p.hyper2 = hyper2;
      p.hyper = hyper2 ? MQ_HYP_GEMM : hyper_ws_ok(d.S, d.E, d.NH, d.M) ? MQ_HYP_WS
                : hyper_ok(d.S, d.NH) ? MQ_HYP_LDS : MQ_HYP_GEMM;
      p.ns = p.nsplit_mix = std::max(1, std::min({o.dwh_split, kRedZ, (d.M + 1) / 2}));
      if (!hyper2) {
        p.dwh_in_red1 = true;
        p.tj = (d.NH + DWH_T - 1) / DWH_T;
        p.ts = (d.S + 1 + DWH_T - 1) / DWH_T;
        p.ndwh = p.tj * p.ts * p.ns;
      }
    }
    p.mix = pick_mix(d, o);
    p.lambda = have_lambda_ws;
    p.per = per;
    p.nblk_mix = (d.M + 3) / 4;
    p.dw1_ns = p.nsplit_fc1 = split_k_slices(RT, (d.I + Dw1Prob::BN - 1) / Dw1Prob::BN);
    p.ffn_wr_ns = split_k_slices(RT, 1);
    const int cap = o.ffn_dp2_blocks > 0 ? std::min(o.ffn_dp2_blocks, kFfnDp2Blocks) : kFfnDp2Blocks;
    const int64_t per_blk = (RT + cap - 1) / cap;
    p.ffn_rpb = (int)((per_blk + FFN_DP2_STEP - 1) / FFN_DP2_STEP * FFN_DP2_STEP);
    p.ffn_nblk2 = (int)((RT + p.ffn_rpb - 1) / p.ffn_rpb);
    mq_plan& r = p.report;   // fused_fwd, rw_fwd, fused_bwd, rw_bwd, tiles, bwd_lean and dwh stay 0
    r.rows = d.R;
    r.inline_ids = inline_ids ? 1 : 0;
    r.hyper = p.hyper;
    r.mix = p.mix;
    r.td_lambda = p.lambda ? 1 : 0;
    r.per = p.per ? 1 : 0;
    p.hyper_layers = hyper2 ? 2 : qmix ? 1 : 0;
    return p;
  }
  // the two-layer hypernet never rides in a forward or in the BPTT's grid: the forward and BPTT choices below are then
  // those of a step without a hypernet (the same shape's VDN plan)
  const bool hyper2 = qmix && hyper_layers == 2;
  // num_cu <= 0: the device query failed, so no pair forward and no second-wave appends
  const bool two_waves = num_cu > 0 && d.R > num_cu;   // 2R row-nets at two per CU; a second wave of BPTT rows

  // forward and BPTT kind
  p.kq1 = tile_kq1(d.O);
  p.rw_fwd = pick_rw(d.R, 512);
  p.rw_bwd = std::min(2, pick_rw(d.R, 256));   // RW >= 4 spills the role registers at 512 threads: capped at 2
  const bool tiles = tiles_ok(d.I, d.O, d.A, d.n, d.Tp, RT) && !o.unfused_fwd && !o.unfused_bwd &&
                     (o.row_tiles == 1 || (o.row_tiles < 0 && d.R > 512));
  p.fused_bwd = !tiles && d.R <= kFusedBwdRmax && fused_bwd_ok(d.I, d.O, d.A, d.n, RT) && !o.unfused_bwd;
  const bool hyf = qmix && !hyper2 && hyper_ws_ok(d.S, d.E, d.NH, d.M) && hyf_ok(d.S, d.E, d.NH, d.M);   // may ride in a forward
  if (tiles) {
    p.fwd = FWD_TILES;
  } else if (p.rw_fwd == 1 && fused_fwd_ok(d.I, d.O, d.A, d.n, RT) && !o.unfused_fwd) {
    // the row-pair forward when the rows fit one wave of workgroups (fwd_pair=1 forces it, =0 keeps the one-row-net
    // kernel); hyp_in_fwd=1 asks for the one-row-net kernel with the hypernet appended to its grid
    const bool pair = o.hyp_in_fwd != 1 && pair_fwd_ok(d.I, d.O, d.A, d.n, RT) &&
                      (o.fwd_pair == 1 || (o.fwd_pair < 0 && !two_waves && num_cu > 0));
    p.fwd = FWD_ONE_ROW;
    if (!pair && (o.hyp_in_fwd == 1 || (o.hyp_in_fwd < 0 && two_waves)) && hyf) {
      p.hyp_place = HYP_FWD_GRID;
    } else if (pair) {
      p.fwd = FWD_PAIR;
      // the hypernet inside the pair kernel (hyp_in_fwd=0 keeps hyper_ws_kernel after it): on waves 4 / 5 when every
      // hypernet block has a workgroup, else as its epilogue (pair_hyp_epi forces the epilogue)
      if (o.hyp_in_fwd != 0 && hyf)
        p.hyp_place = 2 * ((d.M + 31) / 32) <= d.R && !o.pair_hyp_epi ? HYP_PAIR_WAVES : HYP_PAIR_EPI;
    }
  }
  // One expression for both ends of the lean path. The forward used to set rec_coef from `fused_bwd && bwd_lean != 0`
  // inside its pair branch and the BPTT `lean` from `pair forward && bwd_lean != 0` inside its fused branch: each is
  // this conjunction in every case.
  p.lean = p.fused_bwd && p.fwd == FWD_PAIR && o.bwd_lean != 0;
  p.rec_coef = p.lean && (kBwdLean & LEAN_COEF) != 0 ? 1 : 0;

  // hypernet kernel
  if (qmix) {
    if (p.hyp_place == HYP_ABSENT) p.hyp_place = HYP_OWN_LAUNCH;
    p.hyper2 = hyper2;
    p.hyper = hyper2 ? MQ_HYP_GEMM   // layer 1 is the state-fed GEMM at every shape
              : p.hyp_place != HYP_OWN_LAUNCH || hyper_ws_ok(d.S, d.E, d.NH, d.M) ? MQ_HYP_WS   // weight streaming
              : hyper_ok(d.S, d.NH) ? MQ_HYP_LDS : MQ_HYP_GEMM;
  }

  // mixer tail
  p.mix = pick_mix(d, o);
  p.lambda = have_lambda_ws;   // cfg.td_lambda > 0 or MQ_PLAN lambda_path=1 (mq_create)
  p.per = per;   // armed for this step (mq_set_per): changes no other choice
  p.nblk_mix = (d.M + 3) / 4;

  // BPTT slabs, dW1 split
  if (tiles) {
    p.nblk_bwd = p.nsplit_fc1 = (d.R + TR_B - 1) / TR_B;
  } else if (p.fused_bwd) {
    p.nblk_bwd = p.nsplit_fc1 = d.R;
  } else {
    p.nblk_bwd = (d.R + p.rw_bwd - 1) / p.rw_bwd;
    p.dw1_ns = p.nsplit_fc1 = split_k_slices(RT, (d.I + Dw1Prob::BN - 1) / Dw1Prob::BN);
  }

  // dW_hyper: appended to the fused BPTT's grid when its rows exceed the CUs (the second wave of rows leaves CUs
  // idle), else fused with pass 1 of the reduction (dwh_red1_kernel); dwh_in_bwd=0|1 forces one. (Round 6: its tiles
  // on the BPTT's chain waves in the kernel's tail, idle while the producers reduce the last chunk, made the BPTT 14 us
  // longer against the 8.6 us they took out of the reduction's launch: four waves per CU leave each tile's load round
  // trips exposed. Removed.)
  if (hyper2) {
    // the weight gradients are a launch of their own: m-slices into slab_mix, summed by both reduction passes
    p.ns = p.nsplit_mix = std::max(1, std::min({o.dwh_split, kRedZ, (d.M + 1) / 2}));
  } else if (qmix) {
    p.dwh_in_bwd = p.fused_bwd && (o.dwh_in_bwd >= 0 ? o.dwh_in_bwd != 0 : two_waves);
    p.dwh_in_red1 = !p.dwh_in_bwd;
    p.tj = (d.NH + DWH_T - 1) / DWH_T;
    p.ts = (d.S + 1 + DWH_T - 1) / DWH_T;
    // pass 1 shares its launch with dW_hyper, so dW_hyper's slabs must go straight to pass 2: at most kRedZ
    p.ns = p.nsplit_mix = std::max(1, std::min({o.dwh_split, kRedZ, (d.M + 1) / 2}));
    p.ndwh = p.tj * p.ts * p.ns;
  }

  mq_plan& r = p.report;
  r.rows = d.R;
  r.inline_ids = inline_ids ? 1 : 0;
  r.tiles = tiles ? 1 : 0;
  r.fused_fwd = p.fwd == FWD_PAIR ? 2 : p.fwd == FWD_ONE_ROW ? 1 : 0;
  r.rw_fwd = p.fwd == FWD_UNFUSED ? p.rw_fwd : 0;
  r.fused_bwd = p.fused_bwd ? 1 : 0;
  r.rw_bwd = p.fused_bwd || tiles ? 0 : p.rw_bwd;
  r.hyper = p.hyper;
  r.mix = p.mix;
  r.dwh = p.dwh_in_bwd ? 1 : 0;
  r.td_lambda = p.lambda ? 1 : 0;
  r.bwd_lean = p.lean ? 1 : 0;
  r.per = p.per ? 1 : 0;
  p.hyper_layers = hyper2 ? 2 : qmix ? 1 : 0;
  return p;
}

}  // namespace mq
