// The feed-forward agent (mq_config.agent = MQ_AGENT_FFN; epymarl's use_rnn: False): rnn is Linear(64, 64) + ReLU,
//   x1 = relu(fc1(xin));  h = relu(rnn(x1));  q = fc2(h)
// so there is no chain over t: every one of the (T + 1) R rows is independent and the agent's work is row-parallel.
//
// Forward (both nets):  Fc1Prob (learner_gemms.hpp, writes X1 and XIN)  ->  FfnHidProb  Hh = relu(X1 Wr^T + br)
//                       ->  Fc2Prob over Hh (Work::Hs holds Hh: the layout of the GRU's hidden states)
// Backward (online net), from the mixer tail's dQ/dchosen [t][row]:
//   ffn_dp2_kernel  dP2[row][j] = dchosen[row] W2[a_row][j] [Hh > 0]  (0 at t = T), and the fc2 gradients
//                   dW2[a_row] += dchosen Hh, db2[a_row] += dchosen as one slab per workgroup
//   FfnDx1Prob      dP1 = (dP2 Wr) [X1 > 0]
//   FfnDwrProb      [dWr | dbr] = dP2^T X1                split-K over (t, row)
//   Dw1Prob         [dW1 | db1] = dP1^T XIN               (learner_gemms.hpp)
// ffn_step_kernel is one acting step (mq_mac_forward / mq_agent_forward on such a handle).
#pragma once
#include "learner_gemms.hpp"

namespace mq {

// Hh = relu(X1 Wr^T + br), grid.z = net.
struct FfnHidProb {
  static constexpr int BN = 64;
  const float* X1;   // [2][M][H]
  const float* P0;
  const float* P1;
  int64_t o_w, o_b;
  float* Hh;         // [2][M][H]
  int64_t M;
  using APat = KPat;
  using BPat = KPat;
  static constexpr bool kRowSum = false;
  struct Ctx {
    const float* arow;
    const float* brow;
  };
  MQ_DEV Ctx make_ctx(int m0, int n0, int z, int tid) const {
    Ctx c;
    const int m = m0 + KPat::row(tid);
    c.arow = (m < M) ? X1 + ((int64_t)z * M + m) * H : nullptr;
    c.brow = (z ? P1 : P0) + o_w + (int64_t)(n0 + KPat::row(tid)) * H;   // N = H = BN: n0 is 0
    return c;
  }
  MQ_DEV void krange(int, int& kb, int& ke) const { kb = 0; ke = H; }
  MQ_DEV void load_a(const Ctx& c, int k0, int, float (&r)[4]) const {
    ld4(c.arow ? c.arow + k0 + KPat::kq(threadIdx.x) : nullptr, r);
  }
  MQ_DEV void load_b(const Ctx& c, int, int k0, int, float (&r)[4]) const {
    ld4(c.brow + k0 + KPat::kq(threadIdx.x), r);
  }
  MQ_DEV void epilogue(const Ctx&, const f32x16& acc, int mrow0, int ncol0, int z, int lane) const {
    const float bj = (z ? P1 : P0)[o_b + ncol0 + (lane & 31)];
    float* out = Hh + (int64_t)z * M * H;
    for_tile(acc, mrow0, ncol0, lane, [&](int m, int jj, float v) {
      if (m < M) out[(int64_t)m * H + jj] = fmaxf(v + bj, 0.0f);
    });
  }
  MQ_DEV void rowsum_out(int, int, float) const {}
};

// dP1 = (dP2 Wr) * [X1 > 0]: Dx1Prob with the contraction over rnn's 64 outputs.
struct FfnDx1Prob {
  static constexpr int BN = 64;
  const float* dP2;   // [M][H]
  const float* Wr;    // online rnn.weight [H][H]
  const float* X1o;   // online X1 [M][H]
  float* dP1;         // [M][H]
  int64_t M;
  using APat = KPat;
  using BPat = MPat;
  static constexpr bool kRowSum = false;
  struct Ctx {
    const float* arow;
  };
  MQ_DEV Ctx make_ctx(int m0, int, int, int tid) const {
    Ctx c;
    const int m = m0 + KPat::row(tid);
    c.arow = (m < M) ? dP2 + (int64_t)m * H : nullptr;
    return c;
  }
  MQ_DEV void krange(int, int& kb, int& ke) const { kb = 0; ke = H; }
  MQ_DEV void load_a(const Ctx& c, int k0, int, float (&r)[4]) const {
    ld4(c.arow ? c.arow + k0 + KPat::kq(threadIdx.x) : nullptr, r);
  }
  MQ_DEV void load_b(const Ctx&, int, int k0, int, float (&r)[4]) const {
    const int nn = MPat::row(threadIdx.x), k = k0 + MPat::kq(threadIdx.x);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = Wr[(int64_t)(k + i) * H + nn];
  }
  MQ_DEV void epilogue(const Ctx&, const f32x16& acc, int mrow0, int ncol0, int, int lane) const {
    for_tile(acc, mrow0, ncol0, lane, [&](int m, int j, float v) {
      if (m < M) {
        const int64_t o = (int64_t)m * H + j;
        dP1[o] = X1o[o] > 0.0f ? v : 0.0f;
      }
    });
  }
  MQ_DEV void rowsum_out(int, int, float) const {}
};

// [dWr | dbr] slab: out row j (rnn output unit), out col k (rnn input unit), reduction over rows tr (Dw1Prob's shape
// with the 64 columns of X1 in XIN's place).
struct FfnDwrProb {
  static constexpr int BN = 64;
  static constexpr int LEN = H * H + H;
  const float* dP2;   // [RT][H]
  const float* X1o;   // [RT][H]
  float* slab;        // [nsplit][LEN]
  int64_t K;          // RT
  int nsplit;
  using APat = MPat;
  using BPat = MPat;
  static constexpr bool kRowSum = true;
  struct Ctx {};
  MQ_DEV Ctx make_ctx(int, int, int, int) const { return Ctx{}; }
  MQ_DEV void krange(int z, int& kb, int& ke) const { krange_split((int)K, nsplit, z, kb, ke); }
  MQ_DEV void load_a(const Ctx&, int k0, int ke, float (&r)[4]) const {
    const int j = MPat::row(threadIdx.x), k = k0 + MPat::kq(threadIdx.x);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (k + i < ke) ? dP2[(int64_t)(k + i) * H + j] : 0.0f;
  }
  MQ_DEV void load_b(const Ctx&, int, int k0, int ke, float (&r)[4]) const {
    const int f = MPat::row(threadIdx.x), k = k0 + MPat::kq(threadIdx.x);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (k + i < ke) ? X1o[(int64_t)(k + i) * H + f] : 0.0f;
  }
  MQ_DEV void epilogue(const Ctx&, const f32x16& acc, int mrow0, int ncol0, int z, int lane) const {
    float* out = slab + (int64_t)z * LEN;
    for_tile(acc, mrow0, ncol0, lane, [&](int j, int ff, float v) {
      if (j < H && ff < H) out[(int64_t)j * H + ff] = v;
    });
  }
  MQ_DEV void rowsum_out(int j, int z, float v) const {
    if (j < H) slab[(int64_t)z * LEN + H * H + j] = v;
  }
};

// dP2 and the fc2 gradients. Workgroup b owns rows [b rpb, (b + 1) rpb) of the RT = (T + 1) R rows (rpb a multiple of
// 4) and walks them four at a time: thread (k = tid % 64, q = tid / 64) loads unit k of the four rows, group q stores
// row q's dP2, and the fc2 gradients go to LDS accumulators where word (a, k) belongs to the one thread with
// q = a % 4, which adds its rows in order: no two threads touch a word, and the sums are the same on every run.
// The slab [dW2 (A x 64) | db2 (A)] is written once at the end. Dynamic LDS: W2 | dW2 | db2.
constexpr int FFN_DP2_STEP = 4;
inline size_t ffn_dp2_lds_bytes(int A) { return ((size_t)2 * A * H + A) * sizeof(float); }

__global__ __launch_bounds__(256) void ffn_dp2_kernel(Dims d, Rep rp, const float* __restrict__ W2,
                                                      const float* __restrict__ dch, const float* __restrict__ Hh,
                                                      float* __restrict__ dP2, float* __restrict__ slab, int rpb) {
  extern __shared__ __attribute__((aligned(16))) float ffn_dyn[];
  const int A = d.A, tid = threadIdx.x, k = tid & 63, q = tid >> 6;
  float* w2_s = ffn_dyn;
  float* dw2_s = ffn_dyn + A * H;
  float* db2_s = ffn_dyn + 2 * A * H;
  for (int i = tid; i < A * H; i += 256) { w2_s[i] = W2[i]; dw2_s[i] = 0.0f; }
  for (int i = tid; i < A; i += 256) db2_s[i] = 0.0f;
  __syncthreads();
  const int64_t RT = d.RT(), TR = (int64_t)d.T * d.R;   // rows with a transition: t < T
  const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = min(RT, r0 + (int64_t)rpb);
  for (int64_t base = r0; base < r1; base += FFN_DP2_STEP) {
    float dv[FFN_DP2_STEP], hv[FFN_DP2_STEP];
    int av[FFN_DP2_STEP];
#pragma unroll
    for (int i = 0; i < FFN_DP2_STEP; ++i) {
      const int64_t tr = base + i;
      dv[i] = 0.0f; hv[i] = 0.0f; av[i] = 0;
      if (tr < r1) {
        hv[i] = Hh[tr * H + k];
        if (tr < TR) {
          int t, r, b, ag;
          split_tr(d, (uint32_t)tr, t, r, b, ag);
          dv[i] = dch[tr];
          av[i] = min(max((int)rp.actions[(rp.ep(b) * d.t_stride + t) * d.n + ag], 0), A - 1);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < FFN_DP2_STEP; ++i) {
      if (i == q && base + i < r1) dP2[(base + i) * H + k] = hv[i] > 0.0f ? dv[i] * w2_s[av[i] * H + k] : 0.0f;
      if ((av[i] & 3) == q && base + i < TR && base + i < r1) {
        dw2_s[av[i] * H + k] += dv[i] * hv[i];
        if (k == 0) db2_s[av[i]] += dv[i];
      }
    }
  }
  __syncthreads();
  float* out = slab + (int64_t)blockIdx.x * ((int64_t)A * H + A);
  for (int i = tid; i < A * H; i += 256) out[i] = dw2_s[i];
  for (int i = tid; i < A; i += 256) out[A * H + i] = db2_s[i];
}

// One BasicMAC.forward / RNNAgent.forward step of the feed-forward agent for every row: mac_step_kernel
// (optim_kernels.hpp) with the Linear + ReLU in the GRU cell's place. One 256-thread workgroup per row; h_in is not
// an argument: the incoming hidden state is ignored. Dynamic LDS: xin [I rounded up to 4] | x1 [H] | h [H].
inline size_t ffn_step_lds_bytes(int I) { return (size_t)(((I + 3) & ~3) + 2 * H) * sizeof(float); }

__global__ __launch_bounds__(256) void ffn_step_kernel(Dims d, Rep rp, const float* __restrict__ P, int64_t o_w1,
                                                       int64_t o_b1, int64_t o_wr, int64_t o_br, int64_t o_w2,
                                                       int64_t o_b2, int t, const float* __restrict__ xin_dense,
                                                       float* __restrict__ h_out, float* __restrict__ q_out) {
  extern __shared__ __attribute__((aligned(16))) float ffn_sm[];
  float* xin = ffn_sm;
  float* x1 = xin + ((d.I + 3) & ~3);
  float* hh = x1 + H;
  const int row = blockIdx.x, b = row / d.n, ag = row - b * d.n, tid = threadIdx.x;
  const int64_t slot = xin_dense ? 0 : rp.ep(b) * d.t_stride + t;
  for (int f = tid; f < d.I; f += 256) {
    float v;
    if (xin_dense) {
      v = xin_dense[(int64_t)row * d.I + f];
    } else if (f < d.O) {
      v = rp.obs[(slot * d.n + ag) * d.O + f];
    } else {
      int g = f - d.O;
      v = 0.0f;
      bool done = false;
      if (d.last_action) {
        if (g < d.A) {
          if (t > 0 && rp.filled[slot - 1]) v = (int)rp.actions[(slot - 1) * d.n + ag] == g ? 1.0f : 0.0f;
          done = true;
        }
        g -= d.A;
      }
      if (!done) v = (d.agent_id && g == ag) ? 1.0f : 0.0f;
    }
    xin[f] = v;
  }
  __syncthreads();
  if (tid < H) {
    const float* w = P + o_w1 + (int64_t)tid * d.I;
    float s = 0.0f;
    for (int k = 0; k < d.I; ++k) s = fmaf(w[k], xin[k], s);
    x1[tid] = fmaxf(s + P[o_b1 + tid], 0.0f);
  }
  __syncthreads();
  if (tid < H) {
    const float* w = P + o_wr + tid * H;
    float s = 0.0f;
    for (int k = 0; k < H; ++k) s = fmaf(w[k], x1[k], s);
    const float v = fmaxf(s + P[o_br + tid], 0.0f);
    hh[tid] = v;
    h_out[(int64_t)row * H + tid] = v;
  }
  __syncthreads();
  if (tid < d.A) {
    const float* w = P + o_w2 + tid * H;
    float s = 0.0f;
    for (int k = 0; k < H; ++k) s = fmaf(w[k], hh[k], s);
    q_out[(int64_t)row * d.A + tid] = s + P[o_b2 + tid];
  }
}

}  // namespace mq
