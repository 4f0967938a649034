// Which plan does a shape get under either agent kind? plan_step (pymarl_amd/csrc/step_plan.hpp) on the command
// line: no HIP call, no GPU.
//   ffn_plan_probe num_cu mixer n A O S E last_action agent_id double_q B t_len agent [hyper_layers]
// agent: 0 the GRU (MQ_AGENT_GRU) / 1 the feed-forward agent (MQ_AGENT_FFN). MQ_PLAN is read as mq_create reads it.
// For the GRU kind the output is plan_probe.cpp's line, byte for byte (the trailing agent argument must not change a
// GRU plan). For the feed-forward kind the same items are followed by the plan's own: where the hypernet and dW_hyper
// run, the split-K slices and ffn_dp2_kernel's grid.
// Build: hipcc --offload-arch=gfx950 -std=c++17 -O1 tests/host/ffn_plan_probe.cpp -o ffn_plan_probe
#include <cstdio>
#include <cstdlib>

#include "../../pymarl_amd/csrc/step_plan.hpp"

int main(int argc, char** argv) {
  if (argc < 14) {
    std::fprintf(stderr,
                 "usage: %s num_cu mixer n A O S E last_action agent_id double_q B t_len agent [hyper_layers]\n",
                 argv[0]);
    return 2;
  }
  int a[14] = {};
  for (int i = 1; i < argc && i < 15; ++i) a[i - 1] = std::atoi(argv[i]);
  mq_config c{};
  c.mixer = a[1]; c.n_agents = a[2]; c.n_actions = a[3]; c.obs_dim = a[4]; c.state_dim = a[5];
  c.mixing_embed_dim = a[6]; c.obs_last_action = a[7]; c.obs_agent_id = a[8]; c.double_q = a[9];
  c.rnn_hidden_dim = mq::H; c.gamma = 0.99f;
  const int B = a[10], t_len = a[11], agent = a[12], layers = argc > 14 ? a[13] : 1;
  c.max_batch = B; c.max_seq = t_len; c.agent = agent;
  const mq::PlanOverrides ov = mq::read_plan_overrides();
  const mq::Dims d = mq::make_dims(c, B, t_len, t_len);
  const mq::StepPlan p = mq::plan_step(c, ov, d, B <= MQ_INLINE_IDS, ov.lambda_path, a[0], false, layers, agent);
  const mq_plan& r = p.report;
  std::printf("{\"rows\": %d, \"fused_fwd\": %d, \"rw_fwd\": %d, \"fused_bwd\": %d, \"rw_bwd\": %d, \"inline_ids\": %d, "
              "\"hyper\": %d, \"mix\": %d, \"tiles\": %d, \"dwh\": %d, \"td_lambda\": %d, \"bwd_lean\": %d",
              r.rows, r.fused_fwd, r.rw_fwd, r.fused_bwd, r.rw_bwd, r.inline_ids, r.hyper, r.mix, r.tiles, r.dwh,
              r.td_lambda, r.bwd_lean);
  if (agent == MQ_AGENT_FFN)
    std::printf(", \"agent\": %d, \"ffn\": %d, \"hyp_own_launch\": %d, \"dwh_in_red1\": %d, \"dwh_in_bwd\": %d, "
                "\"hyper_layers\": %d, \"dw1_ns\": %d, \"ffn_wr_ns\": %d, \"ffn_nblk2\": %d, \"ffn_rpb\": %d, "
                "\"nsplit_mix\": %d",
                p.agent_report, p.ffn ? 1 : 0, p.hyp_place == mq::HYP_OWN_LAUNCH ? 1 : 0, p.dwh_in_red1 ? 1 : 0,
                p.dwh_in_bwd ? 1 : 0, p.hyper_layers, p.dw1_ns, p.ffn_wr_ns, p.ffn_nblk2, p.ffn_rpb, p.nsplit_mix);
  std::printf("}\n");
  return 0;
}
