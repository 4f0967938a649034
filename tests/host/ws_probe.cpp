// Does a handle's workspace cover what a step asks of it? make_layout / mq_ws_table (learner_layout.hpp) against
// plan_step and plan_reduce (step_plan.hpp, reduce_plan.hpp) on the command line: no HIP call, no GPU.
//   ws_probe num_cu mixer n A O S E last_action agent_id double_q B t_len agent hyper_layers hypernet_embed
// The handle is sized for max_batch = B, max_seq = t_len and the step is a batch of exactly that shape. MQ_PLAN is
// read as mq_create reads it. Prints one JSON line: the parameter offsets (MQ_P_* order, then the total), every
// workspace buffer's floats, the floats the step's plan needs of the slab buffers, red_tmp and norm_part, and whether
// every region of the reduction plan (its slabs and its partials) lies inside the buffer it starts in.
// Build: hipcc --offload-arch=gfx950 -std=c++17 -O1 tests/host/ws_probe.cpp -o ws_probe
#include <cstdio>
#include <cstdlib>

#include "../../pymarl_amd/csrc/reduce_plan.hpp"

int main(int argc, char** argv) {
  if (argc < 16) {
    std::fprintf(stderr, "usage: %s num_cu mixer n A O S E last_action agent_id double_q B t_len agent hyper_layers "
                         "hypernet_embed\n", argv[0]);
    return 2;
  }
  int a[15] = {};
  for (int i = 1; i < 16; ++i) a[i - 1] = std::atoi(argv[i]);
  mq_config c{};
  c.mixer = a[1]; c.n_agents = a[2]; c.n_actions = a[3]; c.obs_dim = a[4]; c.state_dim = a[5];
  c.mixing_embed_dim = a[6]; c.obs_last_action = a[7]; c.obs_agent_id = a[8]; c.double_q = a[9];
  c.rnn_hidden_dim = mq::H; c.gamma = 0.99f;
  const int B = a[10], t_len = a[11];
  c.max_batch = B; c.max_seq = t_len; c.agent = a[12]; c.hypernet_layers = a[13]; c.hypernet_embed = a[14];

  const mq::Layout y = mq::make_layout(c);
  mq::Work w{};
  const WsTable ws = mq::mq_ws_table(c, y, w);
  float* const base = (float*)(uintptr_t)(1 << 20);   // a made-up, 64-float-aligned base: never dereferenced
  const int64_t total = ws_assign(ws, base);
  const mq::PlanOverrides ov = mq::read_plan_overrides();
  const mq::Dims d = mq::make_dims(c, B, t_len, t_len);
  const mq::StepPlan p =
      mq::plan_step(c, ov, d, B <= MQ_INLINE_IDS, ov.lambda_path, a[0], false, y.hyper2 ? 2 : 1, c.agent);
  float* const grad = base + total;   // behind the workspace: the regions' destinations are not checked
  const mq::RedBuilder rb = mq::plan_reduce(p, d, y, w, grad);

  std::printf("{\"offsets\": [");
  for (int i = 0; i <= MQ_P_COUNT; ++i) std::printf("%s%lld", i ? ", " : "", (long long)y.off[i]);
  std::printf("], \"total_floats\": %lld, \"size\": {", (long long)total);
  for (size_t i = 0; i < ws.size(); ++i)
    std::printf("%s\"%s\": %lld", i ? ", " : "", ws[i].name, (long long)ws[i].count);

  const int64_t l1 = (int64_t)mq::H * d.I + mq::H, l2 = (int64_t)d.A * mq::H + d.A;
  const int64_t need_rnn = p.ffn ? mq::ffn_w2_slabs(p) + p.ffn_nblk2 * l2
                                 : (int64_t)p.nblk_bwd * (p.fused_bwd ? y.pitch_rnn : y.len_rnn);
  const bool qmix = c.mixer == MQ_MIXER_QMIX;
  std::printf("}, \"need\": {\"slab_fc1\": %lld, \"slab_rnn\": %lld, \"slab_mix\": %lld, \"slab_v2\": %lld, "
              "\"loss_part\": %lld, \"red_tmp\": %lld, \"norm_part\": %d}",
              (long long)(p.nsplit_fc1 * l1), (long long)need_rnn, (long long)(qmix ? p.nsplit_mix * y.len_mix : 0),
              (long long)(qmix ? (int64_t)p.nblk_mix * (d.E + 1) : 0), (long long)((int64_t)p.nblk_mix * MQ_NSUMS),
              (long long)(rb.tmp - w.red_tmp), rb.b2);

  // every region's slabs [src, src + (nslab - 1) pitch + len) and partials [tmp, tmp + (ng - 1) tpitch + len) inside
  // the workspace buffer that holds their first float
  auto inside = [&](const float* lo, int64_t floats) {
    for (const WsRow& r : ws) {
      const float* b0 = r.f ? *r.f : (const float*)*r.i;
      if (lo >= b0 && lo < b0 + std::max<int64_t>(r.count, 1)) return lo + floats <= b0 + r.count;
    }
    return false;
  };
  bool ok = true;
  for (int k = 0; k < rb.pl.nr; ++k) {
    const mq::RedRegion& R = rb.pl.r[k];
    ok = ok && inside(R.src, (R.nslab - 1) * R.pitch + R.len) && inside(R.tmp, (R.ng - 1) * R.tpitch + R.len);
  }
  std::printf(", \"regions\": %d, \"regions_inside\": %s}\n", rb.pl.nr, ok ? "true" : "false");
  return 0;
}
