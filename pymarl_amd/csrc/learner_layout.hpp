// Where a learner's floats live, as pure functions of its mq_config: the flat parameter buffer's layout (make_layout)
// and the workspace's buffers with their sizes at max_batch x max_seq (mq_ws_table). No HIP call, no handle:
// tests/host/ws_probe.cpp prints both, and checks the sizes against what a step's plan asks of them.
#pragma once
#include "host_util.hpp"
#include "hyper2_kernels.hpp"
#include "step_plan.hpp"

namespace mq {

struct Layout {
  int I = 0, E = 0, NH = 0;   // as every step's Dims derives them
  bool hyper2 = false;        // QMIX with cfg.hypernet_layers = 2
  bool ffn = false;           // cfg.agent = MQ_AGENT_FFN: the feed-forward agent
  int64_t off[MQ_P_COUNT + 1] = {};
  int64_t P = 0;
  int64_t len_rnn = 0, len_mix = 0;
  int64_t pitch_rnn = 0;   // the fused BPTT's slab pitch: len_rnn rounded up to 4 floats (16-byte slab rows)
  Hyp2Lay y2{};            // hyper2: the two-layer hypernet's own offsets
};

inline Layout make_layout(const mq_config& c) {
  Layout y;
  const Dims dmax = make_dims(c, c.max_batch, c.max_seq, c.max_seq);
  y.E = dmax.E; y.I = dmax.I; y.NH = dmax.NH;
  y.hyper2 = c.mixer == MQ_MIXER_QMIX && c.hypernet_layers == 2;
  y.ffn = c.agent == MQ_AGENT_FFN;
  const int Hd = H, n = c.n_agents, A = c.n_actions, S = c.state_dim, E = y.E, I = y.I;
  const bool ffn = y.ffn;
  int64_t sz[MQ_P_COUNT] = {};
  sz[MQ_P_FC1_W] = (int64_t)Hd * I; sz[MQ_P_FC1_B] = Hd;
  sz[MQ_P_RNN_W_IH] = 3LL * Hd * Hd; sz[MQ_P_RNN_W_HH] = 3LL * Hd * Hd;
  sz[MQ_P_RNN_B_IH] = 3 * Hd; sz[MQ_P_RNN_B_HH] = 3 * Hd;
  sz[MQ_P_FC2_W] = (int64_t)A * Hd; sz[MQ_P_FC2_B] = A;
  if (ffn) {   // rnn is Linear(64, 64): the GRU's four tensors are empty
    sz[MQ_P_RNN_W_IH] = sz[MQ_P_RNN_W_HH] = sz[MQ_P_RNN_B_IH] = sz[MQ_P_RNN_B_HH] = 0;
    sz[MQ_P_FFN_W] = (int64_t)Hd * Hd; sz[MQ_P_FFN_B] = Hd;
  }
  // the buffer's order: the enum's, with the two-layer hypernet's second layers behind their first layers
  // (parameters() order of upstream's QMixer) and the feed-forward agent's rnn.weight / rnn.bias in the GRU tensors'
  // place; the entries a configuration lacks are empty and come last
  int order[MQ_P_COUNT];
  int no = 0;
  for (int i = 0; i <= MQ_P_V2_B; ++i) {
    if (ffn && i >= MQ_P_RNN_W_IH && i <= MQ_P_RNN_B_HH) continue;
    order[no++] = i;
    if (ffn && i == MQ_P_FC1_B) { order[no++] = MQ_P_FFN_W; order[no++] = MQ_P_FFN_B; }
    if (y.hyper2 && i == MQ_P_HW1_B) { order[no++] = MQ_P_HW1_W2; order[no++] = MQ_P_HW1_B2; }
    if (y.hyper2 && i == MQ_P_HWF_B) { order[no++] = MQ_P_HWF_W2; order[no++] = MQ_P_HWF_B2; }
  }
  if (!y.hyper2)
    for (int i = MQ_P_HW1_W2; i <= MQ_P_HWF_B2; ++i) order[no++] = i;
  if (ffn)
    for (int i = MQ_P_RNN_W_IH; i <= MQ_P_RNN_B_HH; ++i) order[no++] = i;
  else { order[no++] = MQ_P_FFN_W; order[no++] = MQ_P_FFN_B; }
  if (c.mixer == MQ_MIXER_QMIX) {
    sz[MQ_P_HW1_W] = (int64_t)E * n * S; sz[MQ_P_HW1_B] = (int64_t)E * n;
    sz[MQ_P_HWF_W] = (int64_t)E * S; sz[MQ_P_HWF_B] = E;
    if (y.hyper2) {
      const int64_t He = c.hypernet_embed;
      sz[MQ_P_HW1_W] = He * S; sz[MQ_P_HW1_B] = He;
      sz[MQ_P_HWF_W] = He * S; sz[MQ_P_HWF_B] = He;
      sz[MQ_P_HW1_W2] = (int64_t)E * n * He; sz[MQ_P_HW1_B2] = (int64_t)E * n;
      sz[MQ_P_HWF_W2] = (int64_t)E * He; sz[MQ_P_HWF_B2] = E;
    }
    sz[MQ_P_HB1_W] = (int64_t)E * S; sz[MQ_P_HB1_B] = E;
    sz[MQ_P_V0_W] = (int64_t)E * S; sz[MQ_P_V0_B] = E;
    sz[MQ_P_V2_W] = E; sz[MQ_P_V2_B] = 1;
  }
  int64_t o = 0;
  for (int i = 0; i < MQ_P_COUNT; ++i) { y.off[order[i]] = o; o += sz[order[i]]; }
  y.off[MQ_P_COUNT] = o;
  y.P = o;
  if (y.hyper2) {
    Hyp2Lay& h = y.y2;
    h.w1a = y.off[MQ_P_HW1_W]; h.b1a = y.off[MQ_P_HW1_B]; h.w12 = y.off[MQ_P_HW1_W2]; h.b12 = y.off[MQ_P_HW1_B2];
    h.wfa = y.off[MQ_P_HWF_W]; h.bfa = y.off[MQ_P_HWF_B]; h.wf2 = y.off[MQ_P_HWF_W2]; h.bf2 = y.off[MQ_P_HWF_B2];
    h.hbw = y.off[MQ_P_HB1_W]; h.hbb = y.off[MQ_P_HB1_B]; h.v0w = y.off[MQ_P_V0_W]; h.v0b = y.off[MQ_P_V0_B];
    h.He = c.hypernet_embed; h.E = E; h.nE = n * E; h.N1 = 2 * h.He + 2 * E;
  }
  // the BPTT's slab: [w_ih | w_hh | b_ih | b_hh | fc2.w | fc2.b]; feed-forward agent: [rnn.w | rnn.b | fc2.w | fc2.b]
  y.len_rnn = y.off[MQ_P_FC2_B] + A - y.off[ffn ? MQ_P_FFN_W : MQ_P_RNN_W_IH];
  y.pitch_rnn = (y.len_rnn + 3) & ~int64_t(3);
  y.len_mix = y.off[MQ_P_V2_W] - y.off[MQ_P_HW1_W];
  return y;
}

// The step workspace: every buffer once, in allocation order, with its floats for the largest batch (max_batch
// episodes of max_seq steps) and the pointer it lands in. The slab, red_tmp and norm_part sizes must cover whatever
// plan_step and plan_reduce ask for at any batch up to that one: tests/test_workspace_host.py checks that they do.
inline WsTable mq_ws_table(const mq_config& c, const Layout& y, Work& w) {
  const int64_t n = c.n_agents, A = c.n_actions, Hd = H, NH = y.NH;
  const int64_t RT = (int64_t)c.max_seq * c.max_batch * n;
  const int64_t Mm = (int64_t)(c.max_seq - 1) * c.max_batch;
  const int64_t Rm = (int64_t)c.max_batch * n;
  const int64_t nmix = (Mm + 3) / 4;
  const int64_t l1 = Hd * y.I + Hd, l2 = A * Hd + A;
  auto ng = [](int64_t ns) { return std::min<int64_t>(ns, kRedZ); };
  const int64_t nfc1 = std::max<int64_t>(kNsplitMax, Rm);   // fc1 slabs: split-K GEMM, or one per fused-BPTT row
  // the feed-forward agent's slab_rnn, from the largest batch: its [dWr | dbr] slabs, then its [dW2 | db2] slabs
  const int64_t ffn_ns = ffn_wr_ns_max(RT), ffn_nb = ffn_nblk2_max(RT);
  const int64_t ffn_slabs = y.ffn ? ffn_ns * FfnDwrProb::LEN + ffn_nb * l2 : 0;
  const int64_t red_tmp = (y.ffn ? ng(ffn_ns) * FfnDwrProb::LEN + ng(ffn_nb) * l2 : 0) + ng(Rm) * y.len_rnn +
                          ng(nfc1) * l1 + ng(kNsplitMax) * y.len_mix + ng(nmix) * (y.E + 1) + ng(nmix) * 8;
  const int64_t norm_parts = (l1 + 255) / 256 + (y.len_rnn + 255) / 256 + (y.len_mix + 255) / 256 +
                             (y.E + 1 + 255) / 256 + 1 + 8;
  return {
      {"X1", 2 * RT * Hd, &w.X1},
      {"GI", 2 * RT * 3 * Hd, &w.GI},
      {"Hs", 2 * RT * Hd, &w.Hs},           // both nets
      {"Gates", RT * 5 * Hd, &w.Gates},     // four gate planes, or five coefficient planes
      {"Q", 2 * RT * A, &w.Q},
      {"HYP", 2 * Mm * NH, &w.HYP},
      {"dHYP", Mm * NH, &w.dHYP},
      {"dch", Mm * n, &w.dch},
      {"dGI", RT * 3 * Hd, &w.dGI},
      {"dP1", RT * Hd, &w.dP1},
      {"slab_fc1", nfc1 * l1, &w.slab_fc1},
      {"slab_rnn", std::max(Rm * y.pitch_rnn, ffn_slabs), &w.slab_rnn},   // RW = 1 worst case
      {"slab_mix", (int64_t)kNsplitMax * y.len_mix, &w.slab_mix},
      {"slab_v2", nmix * (y.E + 1), &w.slab_v2},
      {"loss_part", nmix * 8, &w.loss_part},
      {"norm_part", std::max<int64_t>(norm_parts, 256), &w.norm_part},
      {"curmax", Mm * n, nullptr, &w.curmax},   // int32
      {"red_tmp", red_tmp, &w.red_tmp},         // two-pass reduction partials
      {"XIN", RT * y.I, &w.XIN},                // dense agent inputs
      {"S0", Mm * c.state_dim, &w.S0},          // gathered state[:, :-1] rows
  };
}

}  // namespace mq
