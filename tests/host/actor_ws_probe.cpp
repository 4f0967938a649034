// Do a learner handle's buffers cover what the policy-gradient actor's step asks of them? The agent handle's
// mq_ws_table (learner_layout.hpp) and the actor's rows (actor_plan.hpp actor_ws_rows) against a2c_plan's ActorPlan and
// actor_reduce_plan on the command line: no HIP call, no GPU.
//   actor_ws_probe n A O S last_action agent_id agent B t_len max_B max_t_len [buffer=floats ..]
// The handle is sized for max_B episodes of max_t_len stored steps, the step is a batch of B episodes of t_len. MQ_PLAN
// is read as ma_create reads it. `buffer=floats` is the probe's own test hook: it replaces one row's count ("agent."
// in front of the agent handle's rows), so that a test can see a short buffer reported.
// Prints one JSON line: every buffer's floats, the floats the step needs of the slab buffers, the policy kernel's
// arrays, red_tmp and norm_part, the plan's items, and whether every region of the reduction plan (its slabs and its
// partials) lies inside the buffer that holds its first float.
// Build: hipcc --offload-arch=gfx950 -std=c++17 -O1 tests/host/actor_ws_probe.cpp -o actor_ws_probe
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../pymarl_amd/csrc/a2c_plan.hpp"

int main(int argc, char** argv) {
  if (argc < 12) {
    std::fprintf(stderr, "usage: %s n A O S last_action agent_id agent B t_len max_B max_t_len [buffer=floats ..]\n",
                 argv[0]);
    return 2;
  }
  int v[11];
  for (int i = 0; i < 11; ++i) v[i] = std::atoi(argv[i + 1]);
  ma_config c{};
  c.n_agents = v[0]; c.n_actions = v[1]; c.obs_dim = v[2]; c.state_dim = v[3]; c.obs_last_action = v[4];
  c.obs_agent_id = v[5]; c.agent = v[6]; c.rnn_hidden_dim = mq::H; c.critic_type = MA_CRITIC_CV; c.critic_hidden = 64;
  const int B = v[7], t_len = v[8];
  c.max_batch = v[9]; c.max_seq = v[10];
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
  const size_t n_agent_rows = ws.size();
  const WsTable rows = mq::actor_ws_rows(a, c.n_actions, y, (int64_t)(c.max_seq - 1) * c.max_batch * c.n_agents);
  ws.insert(ws.end(), rows.begin(), rows.end());
  auto name_of = [&](size_t i) { return std::string(i < n_agent_rows ? "agent." : "") + ws[i].name; };
  for (int k = 12; k < argc; ++k) {
    const char* eq = std::strchr(argv[k], '=');
    bool found = false;
    for (size_t i = 0; eq && i < ws.size(); ++i)
      if (name_of(i) == std::string(argv[k], (size_t)(eq - argv[k]))) {
        ws[i].count = std::atoll(eq + 1);
        found = true;
      }
    if (!found) {
      std::fprintf(stderr, "no buffer named in %s\n", argv[k]);
      return 2;
    }
  }
  float* const base = (float*)(uintptr_t)(1 << 20);   // a made-up, 64-float-aligned base: never dereferenced
  const int64_t total = ws_assign(ws, base);
  a.agrad = base + total;   // behind the workspace: the regions' destinations are not checked

  const int R = B * c.n_agents;
  const int64_t RT = (int64_t)(t_len - 1) * R;
  mq::ActorPlan p;   // as ma_step_plan gets it; coma_plan makes the same actor_plan call and npol = policy_blocks
  const int npol = mq::a2c_plan(c, B, t_len, false, false, &p, a.ffn_cap).policy_blocks;
  const mq::RedBuilder rb = mq::actor_reduce_plan(p, y, w, a, npol);

  std::printf("{\"total_floats\": %lld, \"size\": {", (long long)total);
  for (size_t i = 0; i < ws.size(); ++i)
    std::printf("%s\"%s\": %lld", i ? ", " : "", name_of(i).c_str(), (long long)ws[i].count);
  const bool ffn = c.agent == MQ_AGENT_FFN;
  const int64_t l1 = (int64_t)mq::H * y.I + mq::H, l2 = (int64_t)c.n_actions * mq::H + c.n_actions;
  std::printf("}, \"need\": {\"agent.slab_fc1\": %lld, \"agent.slab_rnn\": %lld, \"slab_fc2\": %lld, "
              "\"slab_ffn\": %lld, \"ppart\": %lld, \"dL\": %lld, \"dHo\": %lld, \"pi\": %lld, \"red_tmp\": %lld, "
              "\"norm_part\": %d}",
              (long long)(p.ns_w1 * l1), (long long)(ffn ? 0 : p.nblk_bwd * y.len_rnn), (long long)(p.ns_w2 * l2),
              (long long)(p.ffn_blocks * y.len_rnn), (long long)((int64_t)npol * MQ_NSUMS), (long long)(RT * a.Ap),
              (long long)(ffn ? 0 : RT * mq::H), (long long)(RT * c.n_actions), (long long)(rb.tmp - a.red_tmp), rb.b2);
  std::printf(", \"plan\": {\"rows\": %lld, \"ns_w1\": %d, \"ns_w2\": %d, \"nblk_bwd\": %d, \"ffn_tiles\": %d, "
              "\"ffn_blocks\": %d, \"ffn_tpb\": %d}",
              (long long)RT, p.ns_w1, p.ns_w2, p.nblk_bwd, p.ffn_tiles, p.ffn_blocks, p.ffn_tpb);

  // every region's slabs [src, src + (nslab - 1) pitch + len) and partials [tmp, tmp + (ng - 1) tpitch + len) inside
  // the buffer that holds their first float
  auto inside = [&](const float* lo, int64_t floats) {
    for (const WsRow& r : ws) {
      const float* b0 = r.f ? *r.f : (const float*)*r.i;
      if (lo >= b0 && lo < b0 + align_up(std::max<int64_t>(r.count, 1))) return lo + floats <= b0 + r.count;
    }
    return false;
  };
  bool ok = rb.ok;
  for (int k = 0; k < rb.pl.nr; ++k) {
    const mq::RedRegion& r = rb.pl.r[k];
    ok = ok && inside(r.src, (r.nslab - 1) * r.pitch + r.len) && inside(r.tmp, (r.ng - 1) * r.tpitch + r.len);
  }
  std::printf(", \"regions\": %d, \"norm_part_max\": %d, \"regions_inside\": %s}\n", rb.pl.nr, mq::kNormPartMax,
              ok ? "true" : "false");
  return 0;
}
