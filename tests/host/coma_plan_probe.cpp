// What does a COMA train step launch at a shape? coma_plan (pymarl_amd/csrc/coma_plan.hpp) on the command line: no HIP
// call, no GPU.
//   coma_plan_probe num_cu n A O S last_action agent_id B t_len
//                   [exchange replicated timing chain_enabled overlap_enabled shard_lo shard_hi]
// The mode defaults to a plain step: 0 0 0 1 1 0 0. Prints the ComaPlan as one JSON object, followed by the workspace
// bounds mc_create takes from the same header at (B, t_len): ws_nhead, ws_cnorm, ws_h1p_slices.
//   coma_plan_probe red
// adds kRedMaxRegions + 1 regions to a RedBuilder (reduce_plan.hpp) and prints its `ok` flag and region count.
// Build: hipcc --offload-arch=gfx950 -std=c++17 -O1 tests/host/coma_plan_probe.cpp -o coma_plan_probe
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../pymarl_amd/csrc/coma_plan.hpp"
#include "../../pymarl_amd/csrc/reduce_plan.hpp"

static int red_overflow() {
  static float slab[64], dst[64], tmp[64 * (mq::kRedMaxRegions + 1)];
  mq::RedBuilder rb(tmp);
  for (int i = 0; i < mq::kRedMaxRegions + 1; ++i) rb.add(slab, 1, 4, dst, true);
  std::printf("{\"ok\": %d, \"nr\": %d, \"max_regions\": %d}\n", rb.ok ? 1 : 0, rb.pl.nr, mq::kRedMaxRegions);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "red")) return red_overflow();
  if (argc < 10) {
    std::fprintf(stderr, "usage: %s num_cu n A O S last_action agent_id B t_len [exchange replicated timing "
                         "chain_enabled overlap_enabled shard_lo shard_hi] | red\n", argv[0]);
    return 2;
  }
  int a[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, /* mode */ 0, 0, 0, 1, 1, 0, 0};
  for (int i = 1; i < argc && i < 17; ++i) a[i - 1] = std::atoi(argv[i]);
  mc_config c{};
  const int num_cu = a[0];
  c.n_agents = a[1]; c.n_actions = a[2]; c.obs_dim = a[3]; c.state_dim = a[4]; c.obs_last_action = a[5];
  c.obs_agent_id = a[6];
  c.rnn_hidden_dim = 64;
  const int B = a[7], t_len = a[8];
  const mq::ComaMode m{a[9] != 0, a[10] != 0, a[11] != 0, a[12] != 0, a[13] != 0, a[14], a[15]};
  const mq::ComaPlan p = mq::coma_plan(c, B, t_len, num_cu, m);
  int64_t off[MC_P_COUNT + 1];
  mq::mc_offsets(c, off);
  std::printf("{\"Kc\": %d, \"Kp\": %d, \"R\": %d, \"T\": %d, \"KS\": %d, \"nhead\": %d, \"nwgrad\": %d, \"NK\": %d, "
              "\"NG\": %d, \"chain\": %d, \"overlap\": %d, \"lds_td\": %zu, \"lds_l1\": %zu, \"lds_head\": %zu, "
              "\"lds_chain\": %zu, \"actor_B\": %d, \"actor_R\": %d, \"actor_rows\": %lld, \"qv_r0\": %d, \"npol\": %d, "
              "\"fused_fwd\": %d, \"rw_fwd\": %d, \"rw_bwd\": %d, \"nblk_bwd\": %d, \"ns_w1\": %d, \"ns_w2\": %d, "
              "\"refused\": \"%s\", \"Pc\": %lld, \"ws_nhead\": %d, \"ws_cnorm\": %d, \"ws_h1p_slices\": %d}\n",
              p.Kc, p.Kp, p.R, p.T, p.KS, p.nhead, p.nwgrad, p.NK, p.NG, p.chain ? 1 : 0, p.overlap ? 1 : 0, p.lds_td,
              p.lds_l1, p.lds_head, p.lds_chain, p.actor_B, p.actor_R, (long long)p.actor_rows, p.qv_r0, p.npol,
              p.actor.fused_fwd ? 1 : 0, p.actor.rw_fwd, p.actor.rw_bwd, p.actor.nblk_bwd, p.actor.ns_w1, p.actor.ns_w2,
              p.refused ? p.refused : "", (long long)off[MC_P_COUNT], mq::coma_heads(p.R),
              std::max(mq::coma_wgrad_blocks(p.Kc, c.n_actions), 1024), mq::coma_h1p_slices(p.Kc));
  return 0;
}
