// What does an actor-critic train step launch at a shape? a2c_plan (pymarl_amd/csrc/a2c_plan.hpp) on the command
// line: no HIP call, no GPU.
//   a2c_plan_probe critic_type hidden n A O S last_action agent_id B t_len [max_B max_t_len]
// critic_type: 0 cv_critic / 1 ac_critic. Prints the ma_plan as one JSON object, followed by the workspace's slab
// bounds at (max_B, max_t_len) (default: the batch's own): ns_max, ndv_max.
// Build: hipcc --offload-arch=gfx950 -std=c++17 -O1 tests/host/a2c_plan_probe.cpp -o a2c_plan_probe
#include <cstdio>
#include <cstdlib>

#include "../../pymarl_amd/csrc/a2c_plan.hpp"

int main(int argc, char** argv) {
  if (argc < 11) {
    std::fprintf(stderr, "usage: %s critic_type hidden n A O S last_action agent_id B t_len [max_B max_t_len]\n",
                 argv[0]);
    return 2;
  }
  int a[12] = {};
  for (int i = 1; i < argc && i < 13; ++i) a[i - 1] = std::atoi(argv[i]);
  ma_config c{};
  c.critic_type = a[0]; c.critic_hidden = a[1]; c.n_agents = a[2]; c.n_actions = a[3]; c.obs_dim = a[4];
  c.state_dim = a[5]; c.obs_last_action = a[6]; c.obs_agent_id = a[7];
  const int B = a[8], t_len = a[9], maxB = argc > 11 ? a[10] : B, maxT = argc > 12 ? a[11] : t_len;
  const ma_plan p = mq::a2c_plan(c, B, t_len, false, false);
  const int64_t RTmax = (int64_t)(maxT - 1) * maxB * c.n_agents;
  std::printf("{\"rows\": %d, \"rows_target\": %d, \"k\": %d, \"kp\": %d, \"hidden\": %d, \"vec16\": %d, "
              "\"fwd_tiles\": %d, \"vhead_blocks\": %d, \"nstep_lds\": %d, \"dv_blocks\": %d, \"ns_cw2\": %d, "
              "\"ns_cw1\": %d, \"policy_blocks\": %d, \"policy_tail\": %d, \"policy_lanes\": %d, \"ap\": %d, "
              "\"ns_aw1\": %d, \"ns_aw2\": %d, "
              "\"bwd_blocks\": %d, \"ns_max\": %d, \"ndv_max\": %d}\n",
              p.rows, p.rows_target, p.k, p.kp, p.hidden, p.vec16, p.fwd_tiles, p.vhead_blocks, p.nstep_lds,
              p.dv_blocks, p.ns_cw2, p.ns_cw1, p.policy_blocks, p.policy_tail, p.policy_lanes, p.ap, p.ns_aw1, p.ns_aw2,
              p.bwd_blocks,
              mq::a2c_ns_max(RTmax), (int)((RTmax + mq::A2C_DV_ROWS - 1) / mq::A2C_DV_ROWS));
  return 0;
}
