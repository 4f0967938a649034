// Which plan does a shape get? plan_step (pymarl_amd/csrc/step_plan.hpp) on the command line: no HIP call, no GPU.
//   plan_probe num_cu mixer n A O S E last_action agent_id double_q B t_len [have_lambda_ws]
// mixer: 0 none / 1 vdn / 2 qmix (MQ_MIXER_*). MQ_PLAN is read as mq_create reads it; have_lambda_ws defaults to
// what mq_create would allocate (MQ_PLAN lambda_path; a td_lambda > 0 config passes 1). Prints mq_plan as one JSON
// line. Build: hipcc --offload-arch=gfx950 -std=c++17 -O1 tests/host/plan_probe.cpp -o plan_probe
#include <cstdio>
#include <cstdlib>

#include "../../pymarl_amd/csrc/step_plan.hpp"

int main(int argc, char** argv) {
  if (argc < 13) {
    std::fprintf(stderr, "usage: %s num_cu mixer n A O S E last_action agent_id double_q B t_len [have_lambda_ws]\n",
                 argv[0]);
    return 2;
  }
  int a[13] = {};
  for (int i = 1; i < argc && i < 14; ++i) a[i - 1] = std::atoi(argv[i]);
  mq_config c{};
  c.mixer = a[1]; c.n_agents = a[2]; c.n_actions = a[3]; c.obs_dim = a[4]; c.state_dim = a[5];
  c.mixing_embed_dim = a[6]; c.obs_last_action = a[7]; c.obs_agent_id = a[8]; c.double_q = a[9];
  c.rnn_hidden_dim = mq::H; c.gamma = 0.99f;
  const int B = a[10], t_len = a[11];
  c.max_batch = B; c.max_seq = t_len;
  const mq::PlanOverrides ov = mq::read_plan_overrides();
  const bool have_lambda_ws = argc > 13 ? a[12] != 0 : ov.lambda_path;
  const mq::Dims d = mq::make_dims(c, B, t_len, t_len);
  const mq_plan r = mq::plan_step(c, ov, d, B <= MQ_INLINE_IDS, have_lambda_ws, a[0]).report;
  std::printf("{\"rows\": %d, \"fused_fwd\": %d, \"rw_fwd\": %d, \"fused_bwd\": %d, \"rw_bwd\": %d, \"inline_ids\": %d, "
              "\"hyper\": %d, \"mix\": %d, \"tiles\": %d, \"dwh\": %d, \"td_lambda\": %d, \"bwd_lean\": %d}\n",
              r.rows, r.fused_fwd, r.rw_fwd, r.fused_bwd, r.rw_bwd, r.inline_ids, r.hyper, r.mix, r.tiles, r.dwh,
              r.td_lambda, r.bwd_lean);
  return 0;
}
