// The grouped plan of the non-shared actor (actor_plan.hpp, MQ_AGENT_FFN_NS) against what ma_create allocates, in the
// style of actor_ws_probe.cpp: no HIP call, no GPU.
//   actor_ns_probe n A O S last_action B t_len max_B max_t_len
// The handle is sized for max_B episodes of max_t_len stored steps. MQ_PLAN is read as ma_create reads it. Prints one
// JSON line: the plan of the step (B, t_len), the floats it needs of slab_ffn / red_tmp and its norm partials beside
// their sizes, and over EVERY batch (b, t) with b <= max_B, t <= max_t_len: whether the slabs fit slab_ffn and the
// reduction's regions lie inside their buffers ("fits"), and whether every dW1 slice is non-empty, stays inside its
// agent's rows and the slices of an agent tile them exactly ("slices_ok").
// Build: hipcc --offload-arch=gfx950 -std=c++17 -O1 tests/host/actor_ns_probe.cpp -o actor_ns_probe
#include <cstdio>
#include <cstdlib>

#include "../../pymarl_amd/csrc/a2c_plan.hpp"

int main(int argc, char** argv) {
  if (argc < 10) {
    std::fprintf(stderr, "usage: %s n A O S last_action B t_len max_B max_t_len\n", argv[0]);
    return 2;
  }
  int v[9];
  for (int i = 0; i < 9; ++i) v[i] = std::atoi(argv[i + 1]);
  ma_config c{};
  c.n_agents = v[0]; c.n_actions = v[1]; c.obs_dim = v[2]; c.state_dim = v[3]; c.obs_last_action = v[4];
  c.obs_agent_id = 1; c.agent = MQ_AGENT_FFN_NS; c.rnn_hidden_dim = mq::H; c.critic_type = MA_CRITIC_CV;
  c.critic_hidden = 64;
  const int B = v[5], t_len = v[6], n = c.n_agents;
  c.max_batch = v[7]; c.max_seq = v[8];
  if (B < 1 || B > c.max_batch || t_len < 2 || t_len > c.max_seq) {
    std::fprintf(stderr, "the step must fit the handle\n");
    return 2;
  }
  const mq_config ac = mq::agent_config(c, 0.99f, c.agent);
  const mq::Layout y = mq::make_layout(ac);
  mq::Work w{};
  mq::Actor a{};
  a.ffn_cap = mq::plan_int("ffn_actor_blocks", 0);
  WsTable ws = mq::mq_ws_table(ac, y, w);
  const WsTable rows = mq::actor_ws_rows(a, c.n_actions, y, (int64_t)(c.max_seq - 1) * c.max_batch * n, n);
  ws.insert(ws.end(), rows.begin(), rows.end());
  int64_t slab_size = 0, red_size = 0;
  for (const WsRow& r : rows) {
    if (r.f == &a.slab_ffn) slab_size = r.count;
    if (r.f == &a.red_tmp) red_size = r.count;
  }
  float* const base = (float*)(uintptr_t)(1 << 20);   // a made-up, 64-float-aligned base: never dereferenced
  a.agrad = base + ws_assign(ws, base);

  auto inside = [&](const float* lo, int64_t floats) {
    for (const WsRow& r : ws) {
      const float* b0 = r.f ? *r.f : (const float*)*r.i;
      if (lo >= b0 && lo < b0 + align_up(std::max<int64_t>(r.count, 1))) return lo + floats <= b0 + r.count;
    }
    return false;
  };
  bool fits = true, slices_ok = true;
  mq::ActorPlan step{};
  int64_t need_slab = 0, need_red = 0;
  int need_norm = 0, regions = 0;
  for (int b = 1; b <= c.max_batch; ++b)
    for (int t = 2; t <= c.max_seq; ++t) {
      mq::ActorPlan p;
      const int npol = mq::a2c_plan(c, b, t, false, false, &p, a.ffn_cap).policy_blocks;
      const mq::RedBuilder rb = mq::actor_reduce_plan(p, y, w, a, npol);
      bool ok = rb.ok && p.ns_bpa <= a.ffn_slabs_max && rb.b2 <= mq::kNormPartMax && p.ns_w1 == p.ns_bpa;
      for (int k = 0; k < rb.pl.nr; ++k) {
        const mq::RedRegion& r = rb.pl.r[k];
        ok = ok && inside(r.src, (r.nslab - 1) * r.pitch + r.len) && inside(r.tmp, (r.ng - 1) * r.tpitch + r.len);
      }
      fits = fits && ok;
      const int TB = (t - 1) * b;
      for (int g = 0; g < n; ++g) {
        int next = g * TB;   // an agent's slices in order: each starts where the one before ended
        for (int s = 0; s < p.ns_w1; ++s) {
          int kb, ke;
          mq::ffn_ns_slice(TB, p.ffn_tpb * mq::FA_ROWS, g, s, kb, ke);
          slices_ok = slices_ok && kb == next && ke > kb && ke <= (g + 1) * TB;
          next = ke;
        }
        slices_ok = slices_ok && next == (g + 1) * TB;
      }
      if (b == B && t == t_len) {
        step = p;
        need_slab = (int64_t)p.ns_bpa * a.Pa;
        need_red = rb.tmp - a.red_tmp;
        need_norm = rb.b2;
        regions = rb.pl.nr;
      }
    }
  std::printf("{\"plan\": {\"tpa\": %d, \"bpa\": %d, \"tpb\": %d, \"fpa\": %d, \"slices\": %d, \"ffn_tiles\": %d, "
              "\"ffn_blocks\": %d, \"resident\": %d, \"fwd_lds\": %d}, ",
              step.ns_tpa, step.ns_bpa, step.ffn_tpb, step.ns_fpa, step.ns_w1, step.ffn_tiles, step.ffn_blocks,
              step.ffn_resident, (int)step.ffn_fwd_lds);
  std::printf("\"Pa\": %lld, \"Pa1\": %lld, \"need\": {\"slab_ffn\": %lld, \"red_tmp\": %lld, \"norm_part\": %d}, "
              "\"size\": {\"slab_ffn\": %lld, \"red_tmp\": %lld, \"norm_part\": %d}, \"regions\": %d, "
              "\"slabs_max\": %d, \"fits\": %s, \"slices_ok\": %s}\n",
              (long long)a.Pa, (long long)a.Pa1, (long long)need_slab, (long long)need_red, need_norm,
              (long long)slab_size, (long long)red_size, mq::kNormPartMax, regions, a.ffn_slabs_max,
              fits ? "true" : "false", slices_ok ? "true" : "false");
  return 0;
}
