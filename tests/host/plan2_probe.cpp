// plan_probe.cpp's sibling for the two-layer QMIX hypernet: plan_step with its hyper_layers input, no HIP call, no GPU.
//   plan2_probe num_cu mixer n A O S E last_action agent_id double_q B t_len hyper_layers hypernet_embed
// Prints mq_plan as one JSON line, with StepPlan::hyper_layers (what mq_last_hyper_layers reports) beside it.
// Build: hipcc --offload-arch=gfx950 -std=c++17 -O1 tests/host/plan2_probe.cpp -o plan2_probe
#include <cstdio>
#include <cstdlib>

#include "../../pymarl_amd/csrc/step_plan.hpp"

int main(int argc, char** argv) {
  if (argc != 15) {
    std::fprintf(stderr, "usage: %s num_cu mixer n A O S E last_action agent_id double_q B t_len hyper_layers "
                         "hypernet_embed\n", argv[0]);
    return 2;
  }
  int a[14] = {};
  for (int i = 1; i < argc; ++i) a[i - 1] = std::atoi(argv[i]);
  mq_config c{};
  c.mixer = a[1]; c.n_agents = a[2]; c.n_actions = a[3]; c.obs_dim = a[4]; c.state_dim = a[5];
  c.mixing_embed_dim = a[6]; c.obs_last_action = a[7]; c.obs_agent_id = a[8]; c.double_q = a[9];
  c.rnn_hidden_dim = mq::H; c.gamma = 0.99f;
  const int B = a[10], t_len = a[11];
  c.max_batch = B; c.max_seq = t_len;
  c.hypernet_layers = a[12]; c.hypernet_embed = a[13];
  const mq::PlanOverrides ov = mq::read_plan_overrides();
  const mq::Dims d = mq::make_dims(c, B, t_len, t_len);
  const mq::StepPlan sp = mq::plan_step(c, ov, d, B <= MQ_INLINE_IDS, ov.lambda_path, a[0], false,
                                        c.mixer == MQ_MIXER_QMIX && c.hypernet_layers == 2 ? 2 : 1);
  const mq_plan& r = sp.report;
  std::printf("{\"rows\": %d, \"fused_fwd\": %d, \"rw_fwd\": %d, \"fused_bwd\": %d, \"rw_bwd\": %d, \"inline_ids\": %d, "
              "\"hyper\": %d, \"mix\": %d, \"tiles\": %d, \"dwh\": %d, \"td_lambda\": %d, \"bwd_lean\": %d, "
              "\"hyper_layers\": %d}\n",
              r.rows, r.fused_fwd, r.rw_fwd, r.fused_bwd, r.rw_bwd, r.inline_ids, r.hyper, r.mix, r.tiles, r.dwh,
              r.td_lambda, r.bwd_lean, sp.hyper_layers);
  return 0;
}
