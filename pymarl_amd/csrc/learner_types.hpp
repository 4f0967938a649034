// Shapes, replay view and workspace of one learner train step (shared by every kernel of the step).
#pragma once
#include "common.hpp"
#include "../../include/mq_learner.h"

namespace mq {

constexpr int H = 64;        // rnn_hidden_dim (reference default, rnn_agent.py:19-21)
constexpr int G3 = 3 * H;    // GRU gate width (r, z, n)

struct Dims {
  int n, A, O, S, E, I, NH;  // agents, actions, obs, state, mixer embed, agent input width, hypernet outputs
  int B, Tp, T, R, M;        // episodes, unrolled steps (max_t_filled), transitions, rows B*n, mixer rows T*B
  int t_stride;              // storage max_seq_length
  int last_action, agent_id, mixer, double_q;
  float gamma;
  float huber;                      // TD loss: 0 = masked L2 (the reference), > 0 = Huber delta (opt-in)
  FastDiv dR, dN, dB, dO, dI, dS;   // fast division by R, n, B, obs / agent-input / state widths
  MQ_DEV int64_t RT() const { return (int64_t)Tp * R; }
};

// The masked TD loss term of one transition and its derivative d/dQ_tot (before the 1 / mask_sum scale).
// delta == 0: L2, (td m)^2 (q_learner.py:96-97, the reference's loss and the default). delta > 0: Huber, an opt-in
// the reference lacks (north_star names it): 0.5 x^2 for |x| <= delta, delta (|x| - delta / 2) beyond, x = td m.
MQ_DEV float td_loss(float mtd, float delta) {
  if (delta > 0.0f) {
    const float ax = fabsf(mtd);
    return ax <= delta ? 0.5f * mtd * mtd : delta * (ax - 0.5f * delta);
  }
  return mtd * mtd;
}
MQ_DEV float td_dy(float mtd, float mask, float delta) {
  return delta > 0.0f ? fminf(fmaxf(mtd, -delta), delta) * mask : (2.0f * mtd) * mask;
}

// Borrowed replay storage (reference scheme dtypes), episode-major, plus the sampled episode ids.
struct Rep {
  const float* obs;
  const float* state;
  const int64_t* actions;
  const int32_t* avail;
  const float* reward;
  const uint8_t* term;
  const int64_t* filled;
  const int64_t* ep_ids;
  const uint64_t* avail_bits = nullptr;   // optional bitmask view of avail (mq_replay.avail_bits); NULL: avail
  int32_t nids;                    // > 0: the ids live in `ids` (kernel arguments), ep_ids unused
  int32_t ids[MQ_INLINE_IDS];
  MQ_DEV int64_t ep(int b) const { return nids ? (int64_t)ids[b] : (ep_ids ? ep_ids[b] : (int64_t)b); }
};

// The offsets every kernel of the step carries: the tensors up to V.2.bias, then the buffer's total. The two-layer
// hypernet's second-layer tensors (MQ_P_HW1_W2 ..) are not in it: only the hyper2_kernels.hpp launches read them, from
// their own Hyp2Lay, and the kernels of the one-layer step keep their argument blocks.
constexpr int LAY_N = MQ_P_V2_B + 1;
struct Lay {
  int64_t o[LAY_N + 1];
};

// Activation workspace, time-major: row index tr = t*R + r with r = b*n + agent.
struct Work {
  float* X1;      // [2][RT][H]   relu(fc1) per net
  float* GI;      // [2][RT][3H]  W_ih x1 + b_ih per net
  float* Hs;      // [2][RT][H]   hidden after step t per net
  float* Gates;   // [RT][4H]     online r, z, n, W_hn h + b_hn; rec_coef: [RT][5H] a_r, a_z, a_n, a_n r, z (gru_coef)
  float* Q;       // [2][RT][A]   mac_out / target_mac_out
  float* HYP;     // [2][M][NH]   QMIX hypernet outputs per net (state t for online, t+1 for target)
  float* dHYP;    // [M][NH]
  float* dch;     // [T*R]        dLoss_num/dchosen
  float* dGI;     // [RT][3H]
  float* dP1;     // [RT][H]
  float* slab_fc1;   // [nsplit][H*I + H]
  float* slab_rnn;   // [blocks][len_rnn]   w_ih, w_hh, b_ih, b_hh, fc2.w, fc2.b
  float* slab_mix;   // [nsplit][len_mix]   hyper_w_1 .. V.0 (weights+biases)
  float* slab_v2;    // [mix blocks][E+1]   V.2 weight, bias
  float* loss_part;  // [mix blocks][8]
  float* norm_part;  // [norm blocks]
  int32_t* curmax;   // [T*R]
  float* red_tmp;    // two-pass slab reduction partials
  float* XIN;        // [RT][I]  dense agent inputs (written by the fc1 pass, read by dW1)
  float* S0;         // [M][S]   gathered state[:, :-1] rows (written by the hypernet pass, read by dW_hyper)
  float* dHo;        // [RT][H]  COMA actor only: dLogits W2 per (t, row), read by gru_bwd_kernel<.., DY = true>
  // dW_hyper tiles appended to the fused BPTT's grid (gru_bwd_fused.hpp, DWH = 1): slab length, m-slices, j-tiles,
  // tile count
  int64_t dwh_len = 0;
  int dwh_ns = 0, dwh_tj = 0, dwh_n = 0;
  // 1: the row-pair forward writes the BPTT's coefficient record instead of the gate record (the fused BPTT's lean
  // path reads it; every other forward and BPTT keeps the gate record)
  int rec_coef = 0;
};

// The linearised BPTT step's coefficients of one unit (gru_bwd_fused.hpp) from the forward's gate record (r, z, n,
// ghn = W_hn h + b_hn) and h_{t-1}: d(a_r) = dh a_r, d(a_z) = dh a_z, d(a_n) = dh a_n, dgh_n = dh (a_n r).
// Contraction is pinned, so the forward's producers and the BPTT's in-chain form yield the same bits. 1 - n^2 has two
// forms, one fma (fuse_n2) or a rounded product and a subtraction: the in-chain form used to leave the choice to the
// compiler, which fused it in every step copy of the chain but the third of each 4-step round, and results stay
// bit-identical to those builds. coef_fused says which form step t of Tp takes (the rounds start at t = Tp - 1, so
// the third steps' coefficients are those of t = Tp - 4, Tp - 8, ..).
MQ_DEV bool coef_fused(int t, int Tp) { return t > Tp - 4 || ((Tp - t) & 3) != 0; }
struct GruCoef { float ar, az, an, anr; };
MQ_DEV GruCoef gru_coef(float gr, float gz, float gn, float ghn, float hp, bool fuse_n2) {
#pragma clang fp contract(off)
  GruCoef c;
  const float n2 = gn * gn;
  c.an = (1.0f - gz) * (fuse_n2 ? fmaf(-gn, gn, 1.0f) : 1.0f - n2);
  c.ar = (c.an * ghn) * (gr * (1.0f - gr));
  c.az = (hp - gn) * (gz * (1.0f - gz));
  c.anr = c.an * gr;
  return c;
}

MQ_DEV void split_tr(const Dims& d, uint32_t tr, int& t, int& r, int& b, int& ag) {
  t = (int)fdiv(tr, d.dR);
  r = (int)tr - t * d.R;
  b = (int)fdiv((uint32_t)r, d.dN);
  ag = r - b * d.n;
}

}  // namespace mq
