// The QPLEX mixer (pymarl2's mixer: dmaq, DMAQer with adv_hypernet_layers = 1 and is_stop_gradient), fp32, gfx950.
//
// Per live mixer row m = (t, b), state s [S], per-agent chosen q_i, per-agent max m_i and joint action u:
//   w = |W2w relu(W1w s + b1w) + b2w| + 1e-10          v = W2v relu(W1v s + b1v) + b2v                 (both [n])
//   q'_i = w_i q_i + v_i, m'_i = w_i m_i + v_i         (weighted_head; else q' = q, m' = m)
//   key_k = |Wk_k s + bk_k| + 1e-10, ag_k = sigmoid(Wa_k s + ba_k), ac_k = sigmoid(Wu_k [s; onehot(u)] + bu_k)
//   lambda_i = sum_k key_k ag_k,i ac_k,i
//   Q_tot = sum_i q'_i + sum_i stopgrad(q'_i - m'_i) (lambda_i - is_minus_one)
//
// How the work is split (launches around the tail, as the two-layer hypernet's are):
//   DmaqL1Prob      every state-fed product of both nets as ONE GEMM on the MFMA core (gemm_f32.hpp): the columns are
//                   the concatenation [W1w | W1v | Wk_0.. | Wa_0.. | Wu_0..'s state part], NC = 2 He + K (1 + 2 n), so a
//                   state row is gathered once per column tile for all five families; Z[z][m][NC] holds the
//                   pre-activations (bias added). z = 0 writes the gathered states S0 for the weight gradients.
//   dmaq_mix_kernel the tail, one wave per row, four rows per workgroup. Lanes play agents for the selection (chosen q,
//                   masked max of the online Q at t, the double-Q argmax at t + 1, the target's value there and its own
//                   masked max) and for the mix; lanes play hidden units for layer 2's backward. The action part of Wu
//                   is never a product with a one-hot: lane i adds the n gathered weights Wu_k[i][S + j A + u_j] to its
//                   Z column and stores the finished pre-activation back (the backward re-reads it). Layer 2 of w / v
//                   (He <= 64 inputs, n outputs) runs out of LDS in the same wave. The tail writes dQ/dchosen where
//                   mix_kernel writes it, the five loss sums where mix_kernel writes them, and D[m][ND], ND = NC + 2 n:
//                   the gradients of Z's NC pre-activations, then of w's and v's n layer-2 pre-activations.
//   DmaqDwProb      every weight and bias gradient as ONE split-over-rows GEMM, D^T [S0 | onehot(u)]: row tiles of D's
//                   NC columns against the state block and, for the Wu rows only, the one-hot block formed from the
//                   action indices U the tail stored; two more row tiles contract w's / v's layer-2 gradients with
//                   relu(Z). Biases are the row sums. Slice z writes slab z of slab_mix in the parameter layout; the
//                   step's two-pass reduction sums the slabs in a fixed order, so two runs give the same bits.
//
// Bounds, read from the code: rows are guarded with m < M (an idle wave reads row M - 1's inputs, skips the mix and
// stores nothing), columns
// with their family's width, K with the range's end; scalar loads need no alignment, so S % 4 != 0 and He % 4 != 0 are
// ordinary cases. n <= DMAQ_N_MAX, K <= DMAQ_K_MAX and He <= MQ_HYPERNET_EMBED_MAX are checked on the host.
#pragma once
#include "learner_gemms.hpp"
#include "mix_kernels.hpp"

namespace mq {

constexpr int DMAQ_N_MAX = MQ_DMAQ_AGENTS_MAX, DMAQ_K_MAX = MQ_DMAQ_KERNEL_MAX;

// Where DMAQer's tensors lie, relative to `base` (hyper_w_final.0.weight, itself at 0), in parameters() order:
// hyper_w_final.{0,2}, V.{0,2}, si_weight.key_extractors.k, .agents_extractors.k, .action_extractors.k.
struct DmaqLay {
  int64_t base;
  int64_t b1w, w2w, b2w, w1v, b1v, w2v, b2v, key0, ag0, ac0, len;
  int S, n, A, He, K, SA, NC, ND;   // SA = S + n A; NC layer-1 columns; ND = NC + 2 n
  int wh, mo;                       // weighted_head, is_minus_one
};

inline DmaqLay make_dmaq_lay(int64_t base, int S, int n, int A, const mq_dmaq& q) {
  DmaqLay Y{};
  const int64_t He = q.hypernet_embed, K = q.num_kernel;
  Y.base = base;
  Y.S = S; Y.n = n; Y.A = A; Y.He = (int)He; Y.K = (int)K; Y.SA = S + n * A;
  Y.NC = (int)(2 * He + K * (1 + 2 * n)); Y.ND = Y.NC + 2 * n;
  Y.wh = q.weighted_head != 0; Y.mo = q.is_minus_one != 0;
  Y.b1w = He * S; Y.w2w = Y.b1w + He; Y.b2w = Y.w2w + n * He;
  Y.w1v = Y.b2w + n; Y.b1v = Y.w1v + He * S; Y.w2v = Y.b1v + He; Y.b2v = Y.w2v + n * He;
  Y.key0 = Y.b2v + n;
  Y.ag0 = Y.key0 + K * (S + 1);
  Y.ac0 = Y.ag0 + K * ((int64_t)n * S + n);
  Y.len = Y.ac0 + K * ((int64_t)n * Y.SA + n);
  return Y;
}

// Layer-1 column c: its weight row and bias (relative to base) and the row's length F (S, or S + n A for Wu).
struct DmaqCol {
  int64_t w, b;
  int F;
};
MQ_DEV DmaqCol dmaq_col(const DmaqLay& Y, int c) {
  DmaqCol s;
  s.F = Y.S;
  const int h2 = 2 * Y.He, kn = Y.K * Y.n;
  if (c < Y.He) { s.w = (int64_t)c * Y.S; s.b = Y.b1w + c; }
  else if (c < h2) { s.w = Y.w1v + (int64_t)(c - Y.He) * Y.S; s.b = Y.b1v + c - Y.He; }
  else if (c < h2 + Y.K) { s.w = Y.key0 + (int64_t)(c - h2) * (Y.S + 1); s.b = s.w + Y.S; }
  else if (c < h2 + Y.K + kn) {
    const int j = c - h2 - Y.K, k = j / Y.n, i = j - k * Y.n;
    const int64_t o = Y.ag0 + (int64_t)k * (Y.n * Y.S + Y.n);
    s.w = o + (int64_t)i * Y.S; s.b = o + (int64_t)Y.n * Y.S + i;
  } else {
    const int j = c - h2 - Y.K - kn, k = j / Y.n, i = j - k * Y.n;
    const int64_t o = Y.ac0 + (int64_t)k * (Y.n * Y.SA + Y.n);
    s.w = o + (int64_t)i * Y.SA; s.b = o + (int64_t)Y.n * Y.SA + i; s.F = Y.SA;
  }
  return s;
}

// The step's DMAQ buffers (handle-owned).
struct DmaqBuf {
  float* Z;     // [2][M][NC] layer-1 pre-activations per net; the tail finishes the online net's Wu columns in place
  float* D;     // [M][ND]    gradients of Z's columns, then of w's and v's layer-2 pre-activations
  int32_t* U;   // [M][n]     the taken actions
};

// ---------------------------------------------------------------------------------------------- layer 1, both nets
// grid = (ceil(M / 64), ceil(NC / 64), 2 nets): Z[z] = state_{t+z} W^T + b over the state part of every family.
struct DmaqL1Prob {
  static constexpr int BN = 64;
  Dims d;
  Rep rp;
  DmaqLay Y;
  const float* P0;
  const float* P1;
  float* Z;
  float* S0;   // [M][S] gathered state[:, :-1] rows, written by the z == 0 pass
  using APat = KPat;
  using BPat = KPat;
  static constexpr bool kRowSum = false;
  struct Ctx {
    const float* arow;
    const float* brow;
    int m;
  };
  MQ_DEV Ctx make_ctx(int m0, int n0, int z, int tid) const {
    Ctx c;
    c.m = m0 + KPat::row(tid);
    c.arow = nullptr;
    if (c.m < d.M) {
      const int t = (int)fdiv((uint32_t)c.m, d.dB), b = c.m - t * d.B;
      c.arow = rp.state + (rp.ep(b) * d.t_stride + t + z) * (int64_t)d.S;
    }
    const int nn = n0 + KPat::row(tid);
    c.brow = nn < Y.NC ? (z ? P1 : P0) + Y.base + dmaq_col(Y, nn).w : nullptr;
    return c;
  }
  MQ_DEV void krange(int, int& kb, int& ke) const { kb = 0; ke = d.S; }
  MQ_DEV void load_a(const Ctx& c, int k0, int ke, float (&r)[4]) const {
    const int k = k0 + KPat::kq(threadIdx.x);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (c.arow && k + i < ke) ? c.arow[k + i] : 0.0f;
    if (c.arow && blockIdx.z == 0 && blockIdx.y == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (k + i < ke) S0[(int64_t)c.m * d.S + k + i] = r[i];
    }
  }
  MQ_DEV void load_b(const Ctx& c, int, int k0, int ke, float (&r)[4]) const {
    const int k = k0 + KPat::kq(threadIdx.x);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (c.brow && k + i < ke) ? c.brow[k + i] : 0.0f;
  }
  MQ_DEV void epilogue(const Ctx&, const f32x16& acc, int mrow0, int ncol0, int z, int lane) const {
    const int j = ncol0 + (lane & 31);
    if (j >= Y.NC) return;
    const float bj = (z ? P1 : P0)[Y.base + dmaq_col(Y, j).b];
    float* out = Z + (int64_t)z * d.M * Y.NC;
    for_tile(acc, mrow0, ncol0, lane, [&](int m, int jj, float v) {
      if (m < d.M) out[(int64_t)m * Y.NC + jj] = v + bj;
    });
  }
  MQ_DEV void rowsum_out(int, int, float) const {}
};

// ---------------------------------------------------------------------------------------------- the mix of one row
struct DmaqSide {
  float w, wraw, adv;   // lane i: w_i, its pre-abs value, q'_i - m'_i
};

// V_tot + A_tot of one net for the wave's row (the same on every lane). W: the net's DMAQer block; z: the row's NC
// layer-1 pre-activations; hw / hv: relu of their first 2 He, in LDS; u: the joint action, in LDS; q / mx: lane i's
// value and max. KEEP: store the finished Wu pre-activations back into z.
template <bool KEEP>
MQ_DEV float dmaq_side(const DmaqLay& Y, const float* __restrict__ W, float* z, const float* hw, const float* hv,
                       const int* u, float q, float mx, bool on, int lane, DmaqSide& keep) {
  const int n = Y.n, He = Y.He, li = min(lane, n - 1);
  float w = 1.0f, wraw = 0.0f, v = 0.0f;
  if (Y.wh) {
    const float* rw = W + Y.w2w + (int64_t)li * He;
    const float* rv = W + Y.w2v + (int64_t)li * He;
    float aw = W[Y.b2w + li], av = W[Y.b2v + li];
    for (int h = 0; h < He; ++h) {
      aw = fmaf(rw[h], hw[h], aw);
      av = fmaf(rv[h], hv[h], av);
    }
    wraw = aw; w = fabsf(aw) + 1e-10f; v = av;
  }
  const float qp = Y.wh ? fmaf(w, q, v) : q;
  // q' - m' = w (q - m): the same value without the cancellation of two rounded sums (v drops out exactly)
  const float adv = Y.wh ? w * (q - mx) : q - mx;
  const int h2 = 2 * He, c_ag = h2 + Y.K, c_ac = c_ag + Y.K * n;
  float lam = 0.0f;
  for (int k = 0; k < Y.K; ++k) {
    const float key = fabsf(z[h2 + k]) + 1e-10f;
    const float ag = sigmoidf_(z[c_ag + k * n + li]);
    const float* wu = W + Y.ac0 + (int64_t)k * (n * Y.SA + n) + (int64_t)li * Y.SA + Y.S;
    float pre = z[c_ac + k * n + li];
    for (int j = 0; j < n; ++j) pre += wu[j * Y.A + u[j]];
    if (KEEP && on) z[c_ac + k * n + li] = pre;
    lam = fmaf(key * ag, sigmoidf_(pre), lam);
  }
  keep.w = w; keep.wraw = wraw; keep.adv = adv;
  const float vt = wave_sum(on ? qp : 0.0f);
  const float at = wave_sum(on ? adv * (lam - (float)Y.mo) : 0.0f);
  return vt + at;
}

// ---------------------------------------------------------------------------------------------- the tail
// grid = ceil(M / 4) workgroups of 256: wave wv owns row m = 4 blockIdx.x + wv.
__global__ __launch_bounds__(256) void dmaq_mix_kernel(Dims d, Rep rp, const float* __restrict__ P0,
                                                       const float* __restrict__ P1, DmaqLay Y, Work w, DmaqBuf B,
                                                       int32_t* curmax_out) {
  __shared__ float s_h[4][4][64];   // relu of the hidden layers: online w, online v, target w, target v
  __shared__ int s_u[4][2][64];     // the taken actions, the target side's actions
  __shared__ float s_g[4][2][64];   // gradients of w's and v's layer-2 pre-activations
  __shared__ float red[4][8];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + wv, n = d.n, A = d.A, R = d.R, He = Y.He;
  const bool valid = m < d.M;
  const int mc = min(m, d.M - 1);   // an idle wave reads the last row and stores nothing
  const int t = (int)fdiv((uint32_t)mc, d.dB), b = mc - t * d.B;
  const int64_t slot = rp.ep(b) * d.t_stride + t;
  const bool on = valid && lane < n;
  const int li = min(lane, n - 1), r = b * n + li;
  // ---- selection: chosen q and the online max at t; at t + 1 the argmax (first index on ties), the target's value
  // there and the target's own max, every max over available actions with the rest at -9999999
  const float* Qon = w.Q;
  const float* Qtg = w.Q + d.RT() * A;
  const int at = (int)rp.actions[slot * n + li];
  const float* q0 = Qon + ((int64_t)t * R + r) * A;
  const float* q1 = Qon + ((int64_t)(t + 1) * R + r) * A;
  const float* qt = Qtg + ((int64_t)(t + 1) * R + r) * A;
  const int32_t* av0 = rp.avail + (slot * n + li) * (int64_t)A;
  const int32_t* av1 = rp.avail + ((slot + 1) * n + li) * (int64_t)A;
  const float chosen = q0[at];
  const float* qsel = d.double_q ? q1 : qt;
  float mon = 0.0f, best = 0.0f, mtg = 0.0f;
  int cur = 0;
  for (int a = 0; a < A; ++a) {
    const float v0 = av0[a] ? q0[a] : kNegMask;
    const float vs = av1[a] ? qsel[a] : kNegMask;
    const float vt = av1[a] ? qt[a] : kNegMask;
    if (a == 0 || v0 > mon) mon = v0;
    if (a == 0 || vs > best) { best = vs; cur = a; }
    if (a == 0 || vt > mtg) mtg = vt;
  }
  const float tq = d.double_q ? (av1[cur] ? qt[cur] : kNegMask) : best;
  if (on) {
    if (curmax_out) curmax_out[(int64_t)t * R + r] = cur;
    B.U[(int64_t)m * n + lane] = at;
  }
  s_u[wv][0][lane] = at;
  s_u[wv][1][lane] = cur;
  float* zon = B.Z + (int64_t)mc * Y.NC;
  float* ztg = B.Z + ((int64_t)d.M + mc) * Y.NC;
  {
    const int hl = min(lane, He - 1);
    s_h[wv][0][lane] = fmaxf(zon[hl], 0.0f);
    s_h[wv][1][lane] = fmaxf(zon[He + hl], 0.0f);
    s_h[wv][2][lane] = fmaxf(ztg[hl], 0.0f);
    s_h[wv][3][lane] = fmaxf(ztg[He + hl], 0.0f);
  }
  float mask = 0.0f, rew = 0.0f, term = 0.0f;
  if (valid) {
    mask = (float)rp.filled[slot];
    if (t > 0) mask *= 1.0f - (float)rp.term[slot - 1];
    rew = rp.reward[slot];
    term = (float)rp.term[slot];
  }
  __syncthreads();
  // ---- both nets' mix, the TD error and the loss sums (mix_kernel's definitions)
  // An idle wave (wave-uniform) skips the mix and the backward's head loop: row M - 1's Wu columns, which its owner
  // rewrites in place, are then read by their owner alone. The sums inside are wave-local; the barriers are outside.
  DmaqSide so{1.0f, 0.0f, 0.0f}, st;
  float y = 0.0f, yt = 0.0f;
  if (valid) {
    y = dmaq_side<true>(Y, P0 + Y.base, zon, s_h[wv][0], s_h[wv][1], s_u[wv][0], chosen, mon, on, lane, so);
    yt = dmaq_side<false>(Y, P1 + Y.base, ztg, s_h[wv][2], s_h[wv][3], s_u[wv][1], tq, mtg, on, lane, st);
  }
  const float target = rew + d.gamma * (1.0f - term) * yt;
  const float td = y - target, mtd = td * mask;
  const float dy = valid ? td_dy(mtd, mask, d.huber) : 0.0f;
  if (lane == 0) {
    red[wv][0] = valid ? td_loss(mtd, d.huber) : 0.0f;
    red[wv][1] = valid ? mask : 0.0f;
    red[wv][2] = valid ? fabsf(mtd) : 0.0f;
    red[wv][3] = valid ? y * mask : 0.0f;
    red[wv][4] = valid ? target * mask : 0.0f;
  }
  // ---- backward: dQ/dchosen for the BPTT, and D. q' - m' is detached as a whole, so w and v receive V_tot's part only
  float* dr = B.D + (int64_t)mc * Y.ND;
  const float dlam = dy * so.adv;
  const float dwpre = Y.wh ? dy * chosen * sgnf(so.wraw) : 0.0f, dvpre = Y.wh ? dy : 0.0f;
  if (on) {
    w.dch[(int64_t)t * R + r] = Y.wh ? dy * so.w : dy;
    dr[Y.NC + lane] = dwpre;
    dr[Y.NC + n + lane] = dvpre;
  }
  s_g[wv][0][lane] = on ? dwpre : 0.0f;
  s_g[wv][1][lane] = on ? dvpre : 0.0f;
  const int h2 = 2 * He, c_ag = h2 + Y.K, c_ac = c_ag + Y.K * n;
  for (int k = 0; valid && k < Y.K; ++k) {
    const float zk = zon[h2 + k], key = fabsf(zk) + 1e-10f;
    const float ag = sigmoidf_(zon[c_ag + k * n + li]), ac = sigmoidf_(zon[c_ac + k * n + li]);
    const float dk = wave_sum(on ? dlam * ag * ac : 0.0f) * sgnf(zk);
    if (on) {
      dr[c_ag + k * n + lane] = (dlam * key * ac) * (ag * (1.0f - ag));
      dr[c_ac + k * n + lane] = (dlam * key * ag) * (ac * (1.0f - ac));
    }
    if (lane == 0) dr[h2 + k] = dk;
  }
  __syncthreads();
  if (valid && lane < He) {   // layer 2 -> layer 1 of w and v: lanes play hidden units
    const float* W2w = P0 + Y.base + Y.w2w;
    const float* W2v = P0 + Y.base + Y.w2v;
    float aw = 0.0f, av = 0.0f;
    for (int i = 0; i < n; ++i) {
      aw = fmaf(s_g[wv][0][i], W2w[i * He + lane], aw);
      av = fmaf(s_g[wv][1][i], W2v[i * He + lane], av);
    }
    dr[lane] = zon[lane] > 0.0f ? aw : 0.0f;
    dr[He + lane] = zon[He + lane] > 0.0f ? av : 0.0f;
  }
  if (threadIdx.x < 8) {
    const int c = threadIdx.x;
    w.loss_part[(int64_t)blockIdx.x * 8 + c] = c < 5 ? ((red[0][c] + red[1][c]) + (red[2][c] + red[3][c])) : 0.0f;
  }
}

// ---------------------------------------------------------------------------------------------- weight gradients
// Output rows are D's columns, 64 per tile: t1 = ceil(NC / 64) tiles of layer-1 rows against [S0 | onehot(U)] (a row
// keeps its first F columns: S, or S + n A for Wu), then one tile of w's n layer-2 rows against relu(Z[:, 0:He]) and one
// of v's against relu(Z[:, He:2He]). grid = (t1 + 2, ceil(max(S + n A, He) / 64), ns m-slices); a tile whose rows all
// end before its first column walks no K at all.
struct DmaqDwProb {
  static constexpr int BN = 64;
  DmaqLay Y;
  const float* Z;     // [M][NC] online
  const float* D;     // [M][ND]
  const float* S0;    // [M][S]
  const int32_t* U;   // [M][n]
  float* slab;        // [ns][len]
  int64_t len;
  int M, ns, t1;
  using APat = MPat;
  using BPat = MPat;
  static constexpr bool kRowSum = true;
  struct Ctx {
    int seg, j0, jend, m0, f;   // seg 0: layer 1, 1: w's layer 2, 2: v's; D columns [j0, jend) from tile row 0
  };
  MQ_DEV Ctx tile_of(int m0) const {
    Ctx c{};
    const int tile = m0 / GBM;
    c.m0 = m0;
    if (tile < t1) { c.seg = 0; c.j0 = m0; c.jend = Y.NC; }
    else if (tile == t1) { c.seg = 1; c.j0 = Y.NC; c.jend = Y.NC + Y.n; }
    else { c.seg = 2; c.j0 = Y.NC + Y.n; c.jend = Y.ND; }
    return c;
  }
  MQ_DEV Ctx make_ctx(int m0, int n0, int, int tid) const {
    Ctx c = tile_of(m0);
    c.f = n0 + MPat::row(tid);
    return c;
  }
  MQ_DEV void krange(int z, int& kb, int& ke) const {
    krange_split(M, ns, z, kb, ke);
    const Ctx c = tile_of(blockIdx.x * GBM);
    const int last = min(c.j0 + GBM, c.jend) - 1;   // the tile's last row: Wu's rows are the last of layer 1
    const int fmax = c.seg ? Y.He : dmaq_col(Y, last).F;
    if ((int)(blockIdx.y * BN) >= fmax) ke = kb;
  }
  MQ_DEV void load_a(const Ctx& c, int k0, int ke, float (&r)[4]) const {
    const int j = c.j0 + MPat::row(threadIdx.x), k = k0 + MPat::kq(threadIdx.x);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (j < c.jend && k + i < ke) ? D[(int64_t)(k + i) * Y.ND + j] : 0.0f;
  }
  MQ_DEV void load_b(const Ctx& c, int, int k0, int ke, float (&r)[4]) const {
    const int k = k0 + MPat::kq(threadIdx.x), f = c.f;
    int ja = 0, a = 0;
    if (c.seg == 0 && f >= Y.S) { ja = (f - Y.S) / Y.A; a = f - Y.S - ja * Y.A; }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t mm = k + i;
      float v = 0.0f;
      if (mm < ke) {
        if (c.seg == 0) {
          if (f < Y.S) v = S0[mm * Y.S + f];
          else if (f < Y.SA) v = U[mm * Y.n + ja] == a ? 1.0f : 0.0f;
        } else if (f < Y.He) {
          v = fmaxf(Z[mm * Y.NC + (c.seg == 2 ? Y.He : 0) + f], 0.0f);
        }
      }
      r[i] = v;
    }
  }
  // where row j of the tile's segment keeps its weights (row start) and bias, relative to base, and the row's length
  MQ_DEV void out_of(const Ctx& c, int j, int64_t& ow, int64_t& ob, int& F) const {
    if (c.seg == 0) { const DmaqCol g = dmaq_col(Y, j); ow = g.w; ob = g.b; F = g.F; }
    else if (c.seg == 1) { const int i = j - Y.NC; ow = Y.w2w + (int64_t)i * Y.He; ob = Y.b2w + i; F = Y.He; }
    else { const int i = j - Y.NC - Y.n; ow = Y.w2v + (int64_t)i * Y.He; ob = Y.b2v + i; F = Y.He; }
  }
  MQ_DEV void epilogue(const Ctx& c, const f32x16& acc, int mrow0, int ncol0, int z, int lane) const {
    float* out = slab + (int64_t)z * len;
    for_tile(acc, mrow0, ncol0, lane, [&](int m, int ff, float v) {
      const int j = c.j0 + (m - c.m0);
      if (j < c.jend) {
        int64_t ow, ob;
        int F;
        out_of(c, j, ow, ob, F);
        if (ff < F) out[ow + ff] = v;
      }
    });
  }
  MQ_DEV void rowsum_out(int row, int z, float v) const {
    const Ctx c = tile_of(row / GBM * GBM);
    const int j = c.j0 + row % GBM;
    if (j < c.jend) {
      int64_t ow, ob;
      int F;
      out_of(c, j, ow, ob, F);
      slab[(int64_t)z * len + ob] = v;
    }
  }
};

// ---------------------------------------------------------------------------------------------- standalone forward
// DMAQer.forward outside train() (mq_dmaq_forward): V_tot (is_v) or A_tot of `rows` rows. W: the module's parameters
// in parameters() order (Y.base = 0); act: the joint action as the module takes it, [rows][n A] floats (not required
// to be one-hot: Wu's action part is a dot product here). One wave per row, its [s | act] staged in LDS.
constexpr int DMF_ROWS = 4;
constexpr size_t DMF_STATIC_LDS = DMF_ROWS * 2 * 64 * sizeof(float);   // the kernel's s_h, beside the dynamic staging
inline size_t dmaq_forward_lds(int S, int n, int A) { return (size_t)DMF_ROWS * (S + n * A) * sizeof(float); }

MQ_DEV float dmaq_dot(const float* __restrict__ wrow, const float* x, int len, float acc) {
  for (int k = 0; k < len; ++k) acc = fmaf(wrow[k], x[k], acc);
  return acc;
}

__global__ __launch_bounds__(256) void dmaq_forward_kernel(const float* __restrict__ W, DmaqLay Y,
                                                           const float* __restrict__ qs, const float* __restrict__ st,
                                                           const float* __restrict__ act, const float* __restrict__ mx,
                                                           int is_v, float* __restrict__ out, int rows) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ float s_h[DMF_ROWS][2][64];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, m = blockIdx.x * DMF_ROWS + wv;
  const int n = Y.n, S = Y.S, He = Y.He, nA = Y.SA - Y.S;
  const bool valid = m < rows, on = valid && lane < n;
  const int64_t mc = min(m, rows - 1);
  const int li = min(lane, n - 1);
  float* x = lds + wv * Y.SA;   // [s | act]
  for (int e = lane; e < S; e += 64) x[e] = st[mc * S + e];
  if (!is_v)
    for (int e = lane; e < nA; e += 64) x[S + e] = act[mc * nA + e];
  __syncthreads();
  {
    const int hl = min(lane, He - 1);
    s_h[wv][0][lane] = fmaxf(dmaq_dot(W + (int64_t)hl * S, x, S, W[Y.b1w + hl]), 0.0f);
    s_h[wv][1][lane] = fmaxf(dmaq_dot(W + Y.w1v + (int64_t)hl * S, x, S, W[Y.b1v + hl]), 0.0f);
  }
  __syncthreads();
  const float q = qs[mc * n + li], mq_ = is_v ? q : mx[mc * n + li];
  float qp = q, adv = q - mq_;   // q' - m' as w (q - m), the train tail's form: v drops out exactly
  if (Y.wh) {
    const float wi = fabsf(dmaq_dot(W + Y.w2w + (int64_t)li * He, s_h[wv][0], He, W[Y.b2w + li])) + 1e-10f;
    const float vi = dmaq_dot(W + Y.w2v + (int64_t)li * He, s_h[wv][1], He, W[Y.b2v + li]);
    qp = fmaf(wi, q, vi);
    adv = wi * (q - mq_);
  }
  float res;
  if (is_v) {
    res = wave_sum(on ? qp : 0.0f);
  } else {
    float lam = 0.0f;
    for (int k = 0; k < Y.K; ++k) {
      const float* wk = W + Y.key0 + (int64_t)k * (S + 1);
      const int64_t oa = Y.ag0 + (int64_t)k * (n * S + n), ou = Y.ac0 + (int64_t)k * (n * Y.SA + n);
      const float key = fabsf(dmaq_dot(wk, x, S, wk[S])) + 1e-10f;
      const float ag = sigmoidf_(dmaq_dot(W + oa + (int64_t)li * S, x, S, W[oa + (int64_t)n * S + li]));
      const float ac = sigmoidf_(dmaq_dot(W + ou + (int64_t)li * Y.SA, x, Y.SA, W[ou + (int64_t)n * Y.SA + li]));
      lam = fmaf(key * ag, ac, lam);
    }
    res = wave_sum(on ? adv * (lam - (float)Y.mo) : 0.0f);
  }
  if (valid && lane == 0) out[m] = res;
}

}  // namespace mq
