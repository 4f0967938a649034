// Does an actor-critic handle sized for max_B episodes of max_t_len stored steps cover what the feed-forward actor at
// width 128 asks of it at EVERY batch of 1 .. max_B episodes of t_len steps? actor_ws_rows at the wide
// layout (as ma_create calls it) against a2c_plan's ActorPlan and actor_reduce_plan: no HIP call, no GPU.
//   actor_w128_probe n A O S last_action max_B max_t_len t_len
// MQ_PLAN is read as ma_create reads it. Prints one JSON line: the kernels' LDS bytes, over the batches the largest need
// of each buffer beside its size, the largest norm partial count and plan items, whether every region of every
// reduction plan lies inside the buffer it starts in, and whether every dW1 slice was non-empty.
// Build: hipcc --offload-arch=gfx950 -std=c++17 -O1 tests/host/actor_w128_probe.cpp -o actor_w128_probe
#include <cstdio>
#include <cstdlib>

#include "../../pymarl_amd/csrc/a2c_plan.hpp"

int main(int argc, char** argv) {
  if (argc != 9) return 2;
  int v[8];
  for (int i = 0; i < 8; ++i) v[i] = std::atoi(argv[i + 1]);
  ma_config c{};
  c.n_agents = v[0]; c.n_actions = v[1]; c.obs_dim = v[2]; c.state_dim = v[3]; c.obs_last_action = v[4];
  c.obs_agent_id = 1; c.agent = MQ_AGENT_FFN; c.rnn_hidden_dim = mq::HW; c.critic_type = MA_CRITIC_CV;
  c.critic_hidden = 128; c.max_batch = v[5]; c.max_seq = v[6];
  const int t_len = v[7];
  if (t_len < 2 || t_len > c.max_seq) return 2;

  mq_config ac = mq::agent_config(c, 0.99f, c.agent);
  ac.rnn_hidden_dim = mq::H;   // as ma_create: the agent handle stays at width 64 and lends Q and XIN
  mq::Work w{};
  mq::Actor a{};
  a.ffn_cap = mq::plan_int("ffn_actor_blocks", 0);
  WsTable ws = mq::mq_ws_table(ac, mq::make_layout(ac), w);
  const mq::Layout y = mq::make_layout(ac, mq::HW);
  const int64_t RTmax = (int64_t)(c.max_seq - 1) * c.max_batch * c.n_agents;
  const WsTable rows = mq::actor_ws_rows(a, c.n_actions, y, RTmax);
  ws.insert(ws.end(), rows.begin(), rows.end());
  float* const base = (float*)(uintptr_t)(1 << 20);   // a made-up, 64-float-aligned base: never dereferenced
  a.agrad = base + ws_assign(ws, base);
  mq::Work wv = w;   // make_actor_step's view
  wv.X1 = a.X1w; wv.Hs = a.Hw; wv.dP1 = a.dP1w; wv.slab_fc1 = a.slab_w1;
  auto size_of = [&](const float* p) {
    for (const WsRow& r : ws)
      if (r.f && *r.f == p) return (long long)r.count;
    return -1LL;
  };
  auto inside = [&](const float* lo, int64_t floats) {
    for (const WsRow& r : ws) {
      const float* b0 = r.f ? *r.f : (const float*)*r.i;
      if (lo >= b0 && lo < b0 + align_up(std::max<int64_t>(r.count, 1))) return lo + floats <= b0 + r.count;
    }
    return false;
  };

  const int64_t l1 = (int64_t)mq::HW * y.I + mq::HW;
  long long need_w1 = 0, need_ffn = 0, need_rows = 0, need_xin = 0, need_red = 0;
  int norm = 0, blocks = 0, tpb = 0, ns_w1 = 0;
  bool ok = true, slices = true;
  for (int B = 1; B <= c.max_batch; ++B) {
    const int64_t RT = (int64_t)(t_len - 1) * B * c.n_agents;
    mq::ActorPlan p;
    const int npol = mq::a2c_plan(c, B, t_len, false, false, &p, a.ffn_cap).policy_blocks;
    const mq::RedBuilder rb = mq::actor_reduce_plan(p, y, wv, a, npol);
    ok = ok && rb.ok && p.width == mq::HW && p.ffn_blocks <= a.ffn_slabs_max &&
         (int64_t)p.ffn_blocks * p.ffn_tpb >= p.ffn_tiles && (int64_t)(p.ffn_blocks - 1) * p.ffn_tpb < p.ffn_tiles;
    for (int k = 0; k < rb.pl.nr; ++k) {
      const mq::RedRegion& r = rb.pl.r[k];
      ok = ok && inside(r.src, (r.nslab - 1) * r.pitch + r.len) && inside(r.tmp, (r.ng - 1) * r.tpitch + r.len);
    }
    // krange_split's chunk: the last slice starts inside the rows
    const int64_t chunk = ((RT + p.ns_w1 - 1) / p.ns_w1 + mq::GBK - 1) / mq::GBK * mq::GBK;
    slices = slices && (int64_t)(p.ns_w1 - 1) * chunk < RT;
    need_w1 = std::max<long long>(need_w1, p.ns_w1 * l1);
    need_ffn = std::max<long long>(need_ffn, p.ffn_blocks * y.len_rnn);
    need_rows = std::max<long long>(need_rows, RT * mq::HW);
    need_xin = std::max<long long>(need_xin, RT * y.I);
    need_red = std::max<long long>(need_red, rb.tmp - a.red_tmp);
    norm = std::max(norm, rb.b2);
    blocks = std::max(blocks, p.ffn_blocks);
    tpb = std::max(tpb, p.ffn_tpb);
    ns_w1 = std::max(ns_w1, p.ns_w1);
  }
  std::printf("{\"fwd_lds\": %zu, \"bwd_lds\": %zu, \"lds_max\": %zu, \"need\": {\"slab_w1\": %lld, \"slab_ffn\": %lld, "
              "\"X1w\": %lld, \"Hw\": %lld, \"dP1w\": %lld, \"XIN\": %lld, \"red_tmp\": %lld}, "
              "\"size\": {\"slab_w1\": %lld, \"slab_ffn\": %lld, \"X1w\": %lld, \"Hw\": %lld, \"dP1w\": %lld, "
              "\"XIN\": %lld, \"red_tmp\": %lld}, \"norm_part\": %d, \"norm_part_max\": %d, \"ffn_blocks\": %d, "
              "\"ffn_tpb\": %d, \"ns_w1\": %d, \"len_rnn\": %lld, \"P\": %lld, \"regions_inside\": %s, "
              "\"slices_non_empty\": %s}\n",
              mq::kFfnActorWFwdLds, mq::kFfnActorWBwdLds, mq::kFfnActorLdsMax, need_w1, need_ffn, need_rows, need_rows,
              need_rows, need_xin, need_red, size_of(a.slab_w1), size_of(a.slab_ffn), size_of(a.X1w), size_of(a.Hw),
              size_of(a.dP1w), size_of(w.XIN), size_of(a.red_tmp), norm, mq::kNormPartMax, blocks, tpb, ns_w1,
              (long long)y.len_rnn, (long long)y.P, ok ? "true" : "false", slices ? "true" : "false");
  return 0;
}
