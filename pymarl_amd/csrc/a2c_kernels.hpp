// Actor-critic learner kernels (include/ma_a2c.h): epymarl's actor_critic_learner on gfx950, fp32
// throughout. The critic is a V network trained in one optimiser step over every t, so nothing here is a chain: every
// kernel is row-parallel over the (t, row) index tr = t R + r, r = b n + agent.
//
//   a2c_xin_kernel     dense critic inputs X [Tp R][Kp] (cv: state | last joint actions | id; ac: obs | id)
//   A2cLin2            fc1 / fc2 of the target net (Tp R rows) and the online net (its first T R rows) in one launch each
//                      (grid.z = net), two CLinProbT through gemm_f32_kernel
//   a2c_vhead_kernel   fc3 (one output column): a wave per row, V' and V
//   a2c_nstep_kernel   the n-step return, a workgroup per episode out of LDS
//   a2c_dv_kernel      td, the loss sums, dV, dH2 and the fc3 gradient slabs
//   A2cDh1Prob         dH1 = (dH2 W2) [H1 > 0]
//   A2cDwProb          split-K [dW | db] = dY^T Xin for fc2 and fc1 (db = the GEMM's row sum)
//   a2c_policy_kernel  softmax policy, entropy, policy-gradient loss sums and dLoss/dlogits, a wave per row
//   a2c_gate_kernel    the halt word of both applies: set when the batch's mask is empty (and both gradient buffers
//                      put back)
// Gradients are written unnormalised (dV = -2 td, not -2 td / M): the apply kernels divide by the mask elements M they
// read from the sums tail, as every learner of the library does, so no pass over the mask precedes the backward.
//
// Bounds, from the code: every row-indexed kernel tests its row against the launch's row count before the first
// access (xin: tr < rows; vhead: row < Mt + Mo; dv: tr < TR; policy: tr < RT; nstep: e < T n). The taken action is
// clamped to [0, A) before it selects a lane (policy). Slab z of a split-K GEMM is blockIdx.z < nsplit <=
// a2c_ns_max(max rows), slab b of a2c_dv_kernel is blockIdx.x < ceil(T R / 64): both are what ma_create allocated for.
#pragma once
#include "a2c_plan.hpp"
#include "coma_kernels.hpp"
#include "epymarl_kernels.hpp"

namespace mq {

struct ADims {
  int n, A, O, S, K, Kp, Hc, R, B, Tp, T, t_stride;
  int kind, last_action;   // MA_CRITIC_*; cv: the last joint actions are part of the input
  FastDiv dR, dN;
};

// ------------------------------------------------------------------------------------------- critic inputs
// A wave per row tr of `rows` = Tq R rows, first stored step t0 (the standalone forward(batch, t) builds one step).
__global__ __launch_bounds__(256) void a2c_xin_kernel(ADims d, Rep rp, float* __restrict__ X, int t0, int64_t rows) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t tr = (int64_t)blockIdx.x * 4 + wv;
  if (tr >= rows) return;
  const int tl = (int)fdiv((uint32_t)tr, d.dR), r = (int)(tr - (int64_t)tl * d.R), t = t0 + tl;
  const int b = (int)fdiv((uint32_t)r, d.dN), ag = r - b * d.n;
  const int64_t slot = rp.ep(b) * d.t_stride + t;
  float* out = X + tr * d.Kp;
  if (d.kind == MA_CRITIC_CV) {
    const float* st = rp.state + slot * d.S;
    const int k2 = d.S + (d.last_action ? d.n * d.A : 0);
    const bool fill_p = t > 0 && rp.filled[slot - 1] != 0;
    for (int k = lane; k < d.Kp; k += 64) {
      float v = 0.0f;
      if (k < d.S) {
        v = st[k];
      } else if (k < k2) {
        const int j = (k - d.S) / d.A, a = (k - d.S) - j * d.A;
        v = (fill_p && rp.actions[(slot - 1) * d.n + j] == a) ? 1.0f : 0.0f;
      } else if (k < d.K) {
        v = (k - k2) == ag ? 1.0f : 0.0f;
      }
      out[k] = v;
    }
  } else {
    const float* ob = rp.obs + (slot * d.n + ag) * d.O;
    for (int k = lane; k < d.Kp; k += 64) {
      float v = 0.0f;
      if (k < d.O) v = ob[k];
      else if (k < d.K) v = (k - d.O) == ag ? 1.0f : 0.0f;
      out[k] = v;
    }
  }
}

// Two dense linear layers in one launch: net[blockIdx.z] is a CLinProbT of its own (weights, rows, output). The online
// net's rows are a prefix of the target's (t < T of the same X), so its surplus row tiles load nothing and store
// nothing (CLinProbT's m < M tests).
template <int BN_>
struct A2cLin2 {
  static constexpr int BN = BN_;
  CLinProbT<BN_> net[2];
  using APat = KPat;
  using BPat = KPat;
  static constexpr bool kRowSum = false;
  struct Ctx {
    typename CLinProbT<BN_>::Ctx c;
    int z;
  };
  MQ_DEV Ctx make_ctx(int m0, int n0, int z, int tid) const { return Ctx{net[z].make_ctx(m0, n0, z, tid), z}; }
  MQ_DEV void krange(int z, int& kb, int& ke) const { net[z].krange(z, kb, ke); }
  MQ_DEV void load_a(const Ctx& c, int k0, int ke, float (&r)[4]) const { net[c.z].load_a(c.c, k0, ke, r); }
  MQ_DEV void load_b(const Ctx& c, int pass, int k0, int ke, float (&r)[4]) const {
    net[c.z].load_b(c.c, pass, k0, ke, r);
  }
  MQ_DEV void epilogue(const Ctx& c, const f32x16& acc, int mrow0, int ncol0, int z, int lane) const {
    net[z].epilogue(c.c, acc, mrow0, ncol0, z, lane);
  }
  MQ_DEV void rowsum_out(int, int, float) const {}
};

// fc3 has one output column: a wave per row, lane l takes units l (and l + 64 at Hc = 128), a butterfly sums the
// lanes. Rows [0, Mt) are the target net's (-> Vt), [Mt, Mt + Mo) the online net's (-> Vo). bt_Tq > 0: the standalone
// forward, whose row tr = t R + b n + ag goes to out[(b Tq + t) n + ag].
__global__ __launch_bounds__(256) void a2c_vhead_kernel(const float* __restrict__ H2t, const float* __restrict__ H2o,
                                                        const float* __restrict__ Pt, const float* __restrict__ Po,
                                                        int64_t o_w3, int64_t o_b3, int Hc, int64_t Mt, int64_t Mo,
                                                        float* __restrict__ Vt, float* __restrict__ Vo, int R, int n,
                                                        int bt_Tq) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + wv;
  if (row >= Mt + Mo) return;
  const bool tg = row < Mt;
  const int64_t m = tg ? row : row - Mt;
  const float* h = (tg ? H2t : H2o) + m * Hc;
  const float* P = tg ? Pt : Po;
  float s = 0.0f;
  for (int k = lane; k < Hc; k += 64) s = fmaf(h[k], P[o_w3 + k], s);
  s = wave_sum(s);
  if (lane != 0) return;
  const float v = s + P[o_b3];
  if (bt_Tq > 0) {
    const int t = (int)(m / R), r = (int)(m - (int64_t)t * R), b = r / n, ag = r - b * n;
    Vt[((int64_t)b * bt_Tq + t) * n + ag] = v;
  } else {
    (tg ? Vt : Vo)[m] = v;
  }
}

// ------------------------------------------------------------------------------------------- n-step return
// One workgroup per episode. V' (every t, agent), the rewards and the mask of the episode are staged in LDS by all
// threads, then thread e = t0 n + agent accumulates, with N = q_nstep and g[k] = float32(gamma ** k),
//   for s in 0..N, t = t0 + s, stop at t >= T:
//     s == N:                          acc += (g[s] V'[t]) m[t]
//     t == T - 1 and add_last:         acc += (g[s] r[t]) m[t];  acc += g[s + 1] V'[t + 1]
//     else:                            acc += (g[s] r[t]) m[t]
// in that order, every product and sum rounded to fp32 (no contraction). RS != NULL: the standardised rewards
// ([t][b], reward_norm_kernel's output) in the storage's place. LDS: Tp (n + 2) floats. g holds N + 2 floats.
__global__ __launch_bounds__(256) void a2c_nstep_kernel(ADims d, Rep rp, const float* __restrict__ Vt,
                                                        const float* __restrict__ RS, const float* __restrict__ g,
                                                        int N, int add_last, float* __restrict__ ret) {
  // plain operators with contraction off: every product and sum below is rounded on its own. (__fmul_rn / __fadd_rn
  // do not pin that: they are inline functions of plain operators compiled under the default contraction mode, and
  // once inlined here the backend fused their product and sum into one v_fma_f32.)
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float a2c_sm[];
  const int b = blockIdx.x, n = d.n, Tp = d.Tp, T = d.T;
  float* vt = a2c_sm;           // [Tp][n]
  float* rw = vt + Tp * n;      // [Tp]
  float* mk = rw + Tp;          // [Tp]
  const int64_t e0 = rp.ep(b) * d.t_stride;
  for (int e = threadIdx.x; e < Tp * n; e += 256) {
    const int t = e / n, ag = e - t * n;
    vt[e] = Vt[(int64_t)t * d.R + b * n + ag];
  }
  for (int t = threadIdx.x; t < Tp; t += 256) {
    rw[t] = t < T ? (RS ? RS[t * d.B + b] : rp.reward[e0 + t]) : 0.0f;
    mk[t] = coma_mask(rp, e0 + t, t);
  }
  __syncthreads();
  for (int e = threadIdx.x; e < T * n; e += 256) {
    const int t0 = e / n, ag = e - t0 * n;
    float acc = 0.0f;
    for (int s = 0; s <= N; ++s) {
      const int t = t0 + s;
      if (t >= T) break;
      if (s == N) {
        acc = acc + (g[s] * vt[t * n + ag]) * mk[t];
      } else {
        acc = acc + (g[s] * rw[t]) * mk[t];
        if (t == T - 1 && add_last) acc = acc + g[s + 1] * vt[(t + 1) * n + ag];
      }
    }
    ret[(int64_t)t0 * d.R + b * n + ag] = acc;
  }
}

// ------------------------------------------------------------------------------------------- critic loss
// Workgroup b owns rows [64 b, 64 b + 64) of the T R rows. Wave 0 takes one row per lane: td = (ret - V) m, dV = -2 td
// (d sum td^2 / dV; the apply divides by M), and the wave's sums go to part[b][0..4] = sum td^2, sum m, sum |td|,
// sum V m, sum ret m and to the slab's last word (db3 = sum dV). Then every thread (unit k = tid % Hc, group
// q = tid / Hc) walks the rows q, q + 256 / Hc, .. in order: dH2 = dV w3 [H2 > 0] out, dV H2 into its own accumulator;
// the groups' accumulators are summed in group order: slab[b] = [dW3 (Hc) | db3]. No atomics, a fixed order.
__global__ __launch_bounds__(256) void a2c_dv_kernel(ADims d, Rep rp, const float* __restrict__ ret,
                                                     const float* __restrict__ V, const float* __restrict__ H2,
                                                     const float* __restrict__ w3, float* __restrict__ td_out,
                                                     float* __restrict__ dH2, float* __restrict__ slab,
                                                     float* __restrict__ part) {
  __shared__ float dvs[A2C_DV_ROWS];
  __shared__ float accs[4][128];
  const int tid = threadIdx.x, Hc = d.Hc;
  const int64_t TR = (int64_t)d.T * d.R, r0 = (int64_t)blockIdx.x * A2C_DV_ROWS;
  float* out = slab + (int64_t)blockIdx.x * (Hc + 1);
  if (tid < 64) {
    const int64_t tr = r0 + tid;
    float s[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (tr < TR) {
      const int t = (int)fdiv((uint32_t)tr, d.dR), r = (int)(tr - (int64_t)t * d.R);
      const int b = (int)fdiv((uint32_t)r, d.dN);
      const float m = coma_mask(rp, rp.ep(b) * d.t_stride + t, t);
      const float v = V[tr], y = ret[tr];
      const float td = (y - v) * m;
      s[0] = td * td; s[1] = m; s[2] = fabsf(td); s[3] = v * m; s[4] = y * m; s[5] = -2.0f * td;
      td_out[tr] = td;
    }
    dvs[tid] = s[5];
#pragma unroll
    for (int k = 0; k < 6; ++k) s[k] = wave_sum(s[k]);
    if (tid < 8) part[(int64_t)blockIdx.x * 8 + tid] = tid == 0 ? s[0] : tid == 1 ? s[1] : tid == 2 ? s[2]
                                                       : tid == 3 ? s[3] : tid == 4 ? s[4] : 0.0f;
    if (tid == 0) out[Hc] = s[5];
  }
  __syncthreads();
  const int nq = 256 / Hc, k = tid & (Hc - 1), q = tid / Hc;   // Hc = 64 or 128
  const float wk = w3[k];
  float acc = 0.0f;
  for (int i = q; i < A2C_DV_ROWS; i += nq) {
    const int64_t tr = r0 + i;
    if (tr >= TR) break;
    const float h = H2[tr * Hc + k], dv = dvs[i];
    dH2[tr * Hc + k] = h > 0.0f ? dv * wk : 0.0f;
    acc += dv * h;
  }
  accs[q][k] = acc;
  __syncthreads();
  if (tid < Hc) {
    float s = accs[0][tid];
    for (int j = 1; j < nq; ++j) s += accs[j][tid];
    out[tid] = s;
  }
}

// dH1 = (dH2 W2) * [H1 > 0]: FfnDx1Prob with the critic's runtime width.
struct A2cDh1Prob {
  static constexpr int BN = 64;
  const float* dH2;   // [M][Hc]
  const float* W2;    // online fc2.weight [Hc][Hc]
  const float* H1;    // online relu(fc1) [M][Hc]
  float* dH1;         // [M][Hc]
  int64_t M;
  int Hc;
  using APat = KPat;
  using BPat = MPat;
  static constexpr bool kRowSum = false;
  struct Ctx {
    const float* arow;
    int n0;
  };
  MQ_DEV Ctx make_ctx(int m0, int n0, int, int tid) const {
    const int64_t m = m0 + KPat::row(tid);
    return Ctx{m < M ? dH2 + m * Hc : nullptr, n0};
  }
  MQ_DEV void krange(int, int& kb, int& ke) const { kb = 0; ke = Hc; }
  MQ_DEV void load_a(const Ctx& c, int k0, int, float (&r)[4]) const {
    ld4(c.arow ? c.arow + k0 + KPat::kq(threadIdx.x) : nullptr, r);
  }
  MQ_DEV void load_b(const Ctx& c, int, int k0, int, float (&r)[4]) const {
    const int nn = c.n0 + MPat::row(threadIdx.x), k = k0 + MPat::kq(threadIdx.x);   // nn < Hc: Hc % 64 == 0
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = W2[(int64_t)(k + i) * Hc + nn];
  }
  MQ_DEV void epilogue(const Ctx&, const f32x16& acc, int mrow0, int ncol0, int, int lane) const {
    for_tile(acc, mrow0, ncol0, lane, [&](int m, int j, float v) {
      if (m < M) {
        const int64_t o = (int64_t)m * Hc + j;
        dH1[o] = H1[o] > 0.0f ? v : 0.0f;
      }
    });
  }
  MQ_DEV void rowsum_out(int, int, float) const {}
};

// [dW | db] slab = dY^T Xin over rows tr (split-K): out row j (unit of the layer, < Hc), out col f (its input, < ncol),
// db the row sum of the A operand, as Dw1Prob. BN = 128 for fc1's wide input, 64 for fc2.
template <int BN_>
struct A2cDwProb {
  static constexpr int BN = BN_;
  const float* dY;    // [K][Hc]
  int Hc;
  const float* Xin;   // [K][ldx]
  int ldx, ncol;
  float* slab;        // [nsplit][Hc * ncol + Hc]
  int64_t K;          // rows
  int nsplit;
  using APat = MPat;
  using BPat = MPat;
  static constexpr bool kRowSum = true;
  struct Ctx {
    int j, f0;
  };
  MQ_DEV int64_t len() const { return (int64_t)Hc * ncol + Hc; }
  MQ_DEV Ctx make_ctx(int m0, int n0, int, int tid) const { return Ctx{m0 + MPat::row(tid), n0 + MPat::row(tid)}; }
  MQ_DEV void krange(int z, int& kb, int& ke) const { krange_split((int)K, nsplit, z, kb, ke); }
  MQ_DEV void load_a(const Ctx& c, int k0, int ke, float (&r)[4]) const {
    const int k = k0 + MPat::kq(threadIdx.x);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (c.j < Hc && k + i < ke) ? dY[(int64_t)(k + i) * Hc + c.j] : 0.0f;
  }
  MQ_DEV void load_b(const Ctx& c, int pass, int k0, int ke, float (&r)[4]) const {
    const int f = c.f0 + 64 * pass, k = k0 + MPat::kq(threadIdx.x);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (f < ncol && k + i < ke) ? Xin[(int64_t)(k + i) * ldx + f] : 0.0f;
  }
  MQ_DEV void epilogue(const Ctx&, const f32x16& acc, int mrow0, int ncol0, int z, int lane) const {
    const int f = ncol0 + (lane & 31);
    if (f >= ncol) return;
    float* out = slab + (int64_t)z * len();
    for_tile(acc, mrow0, ncol0, lane, [&](int j, int ff, float v) {
      if (j < Hc) out[(int64_t)j * ncol + ff] = v;
    });
  }
  MQ_DEV void rowsum_out(int j, int z, float v) const {
    if (j < Hc) slab[(int64_t)z * len() + (int64_t)Hc * ncol + j] = v;
  }
};

// ------------------------------------------------------------------------------------------------- actor
// One wave per (t, row), lanes = actions (A <= 64): coma_policy_kernel's shape. p = softmax(logits), unavailable
// actions at -1e10 first when mbs; there is no epsilon floor. pi = p on live rows (m != 0) and 1 everywhere on dead
// ones; H = -sum_j pi_j log(pi_j + 1e-10); the row's loss term is -(adv log(pi_u + 1e-10) + ec H) m with adv = td,
// the critic's masked TD error, a constant here. Down to the logits (unnormalised: the apply divides by M), live rows:
//   g_j = -m [adv [j == u] / (p_j + 1e-10) - ec (log(p_j + 1e-10) + p_j / (p_j + 1e-10))]
//   dlogit_k = p_k (g_k - sum_j p_j g_j), zero at masked-before-softmax actions and on dead rows.
// Writes dL [RT][Ap] (pad columns zero), pi [RT][A] (= p), per-block sums part[b][0..4]:
// the loss terms, sum m, sum adv m, sum max(pi) m, sum H m.
__global__ __launch_bounds__(256) void a2c_policy_kernel(Dims d, Rep rp, const float* __restrict__ logits,
                                                         const float* __restrict__ td, float ec, int mbs, int Ap,
                                                         float* __restrict__ dL, float* __restrict__ pi_out,
                                                         float* __restrict__ part) {
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t tr = (int64_t)blockIdx.x * 4 + wv;
  const int A = d.A, n = d.n;
  const int64_t RT = d.RT();
  __shared__ float red[4][5];
  float s_loss = 0.0f, s_m = 0.0f, s_adv = 0.0f, s_pmax = 0.0f, s_ent = 0.0f;
  if (tr < RT) {
    const int t = (int)fdiv((uint32_t)tr, d.dR), r = (int)(tr - (int64_t)t * d.R);
    const int b = (int)fdiv((uint32_t)r, d.dN), ag = r - b * n;
    const int64_t slot = rp.ep(b) * d.t_stride + t;
    const bool on = lane < A;
    const int av = on ? rp.avail[(slot * n + ag) * A + lane] : 0;
    float l = on ? logits[tr * A + lane] : -INFINITY;
    if (mbs && on && !av) l = -1e10f;
    const float mx = wave_max(l);
    const float ex = on ? expf(l - mx) : 0.0f;
    const float p = ex / wave_sum(ex);
    const float m = coma_mask(rp, slot, t);
    const bool live = m != 0.0f;
    const int at = min(max((int)rp.actions[slot * n + ag], 0), A - 1);   // clamped before it selects a lane
    const float pe = on ? (live ? p : 1.0f) : 0.0f;
    const float lg = on ? logf(pe + 1e-10f) : 0.0f;
    const float ent = -wave_sum(pe * lg);
    const float lp_u = __shfl(lg, at, 64);
    const float adv = td[tr];
    const float pmax = wave_max(on ? pe : -INFINITY);
    s_loss = -((adv * lp_u + ec * ent) * m); s_m = m; s_adv = adv * m; s_pmax = pmax * m; s_ent = ent * m;
    float g = 0.0f;
    if (live && on) {
      const float den = p + 1e-10f;
      g = -m * ((lane == at ? adv / den : 0.0f) - ec * (lg + p / den));
    }
    const float dot = wave_sum(on ? p * g : 0.0f);
    float dl = on ? p * (g - dot) : 0.0f;
    if (!live || (mbs && !av)) dl = 0.0f;
    if (lane < Ap) dL[tr * Ap + lane] = dl;
    if (on) pi_out[tr * A + lane] = p;
  }
  if (lane == 0) { red[wv][0] = s_loss; red[wv][1] = s_m; red[wv][2] = s_adv; red[wv][3] = s_pmax; red[wv][4] = s_ent; }
  __syncthreads();
  if (threadIdx.x < 8) {
    const int k = threadIdx.x;
    part[(int64_t)blockIdx.x * 8 + k] = k < 5 ? ((red[0][k] + red[1][k]) + (red[2][k] + red[3][k])) : 0.0f;
  }
}

// After both reductions, ONE workgroup: every thread reads the step's mask elements M (the critic sums' [1]), then a
// barrier, so no thread writes before all have read. M > 0: the halt word both applies read is cleared, nothing else
// happens. M == 0 (an empty batch): the word is set, the stats are zeroed, so the host reads M = 0, and both gradient
// buffers, which the reductions have overwritten with the empty step's sums, are put back to the copies taken before
// the reductions (tails included), and the running reward statistics (rew != NULL: reward standardisation is on, and
// reward_norm_kernel has merged the batch's rewards into them) to theirs: such a step leaves every bound buffer but
// stats as it found it. bak = [na floats of agrad | nc floats of cgrad], rew_bak = [mean, var, count].
constexpr int A2C_GATE_THREADS = 1024;
__global__ __launch_bounds__(A2C_GATE_THREADS) void a2c_gate_kernel(const float* __restrict__ csums,
                                                                    int* __restrict__ halt, float* __restrict__ stats,
                                                                    const float* __restrict__ bak,
                                                                    float* __restrict__ agrad, int64_t na,
                                                                    float* __restrict__ cgrad, int64_t nc,
                                                                    double* __restrict__ rew,
                                                                    const double* __restrict__ rew_bak) {
  if (blockIdx.x != 0) return;
  const bool live = csums[1] > 0.0f;
  __syncthreads();
  if (threadIdx.x == 0) *halt = live ? 0 : 1;
  if (live) return;
  if (threadIdx.x < MA_NSTATS) stats[threadIdx.x] = 0.0f;
  if (rew && threadIdx.x < 3) rew[threadIdx.x] = rew_bak[threadIdx.x];
  for (int64_t i = threadIdx.x; i < na + nc; i += A2C_GATE_THREADS) {
    if (i < na) agrad[i] = bak[i];
    else cgrad[i - na] = bak[i];
  }
}

}  // namespace mq
