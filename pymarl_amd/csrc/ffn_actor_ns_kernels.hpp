// The non-shared feed-forward actor of the actor-critic and PPO learners (ma_config.agent = MQ_AGENT_FFN_NS; epymarl's
// agent: rnn_ns with use_rnn: False): ffn_actor_kernels.hpp's agent with one parameter set per agent index g,
//   x1 = relu(fc1_g(xin));  h = relu(rnn_g(x1));  logits = fc2_g(h)
// as a grouped form of that file's two kernels. The parameters are n blocks of Pa1 floats, block g in the
// single-agent order fc1.weight, fc1.bias, rnn.weight, rnn.bias, fc2.weight, fc2.bias. fa_mma, the [64][68] pitch, the
// 2 x 2 wave split and the LDS maps are that file's; what is new is the work split.
//
// Tiles. With TB = T B, agent g owns the rows e = t B + b < TB. A tile is (g, 64 consecutive e): tpa = ceil(TB / 64)
// tiles per agent, the last one partial. Its rows sit at tr = e n + g in the arrays the policy kernels share (the
// logits Work::Q and dL, 64 rows n A floats apart) and at g TB + e in the actor's own X1, Hh, XIN and dP1, which are
// agent-major [n][TB][.]: one agent's rows are contiguous for the backward's loads and for the split-K dW1. Rows
// e >= TB are zero in every LDS operand and are never stored.
//
// ffn_actor_ns_fwd_kernel   grid (fpa, n), LDS as ffn_actor_fwd_kernel: workgroup (j, g) loads agent g's Wr, W2 and
//   resident W1 once and walks g's tiles j, j + fpa, ..; a streamed W1 (I > 248) streams g's chunk. t0: the stored step
//   of e's t = 0 (the acting path runs one step, TB = B).
// ffn_actor_ns_bwd_kernel   grid (bpa, n), LDS as ffn_actor_bwd_kernel: workgroup (j, g) keeps agent g's W2T / WrT
//   resident and walks g's tiles [j tpb, (j + 1) tpb) in order with dW2 / dWr in registers. It writes
//   [dWr | dbr | dW2 | db2] behind agent g's [dW1 | db1] in gradient slab j: a slab is one whole actor gradient
//   [n][Pa1], so the two-pass reduction sums the bpa slabs as ONE region straight into agrad, whatever n is.
// FfnNsDw1Prob              gemm_f32_kernel policy, grid.z = g bpa + s: slice s of agent g is the rows of workgroup
//   (s, g)'s tiles, a non-empty range inside agent g's TB rows, and lands in slab s at g Pa1.
// No atomics: the same plan gives the same bits on every run.
#pragma once
#include "ffn_actor_kernels.hpp"

namespace mq {

struct FfnNsFwd {
  Dims d;
  Rep rp;
  const float* P;   // [n][Pa1]
  int64_t Pa1, o_w1, o_b1, o_wr, o_br, o_w2, o_b2;   // a tensor's offset inside an agent's block
  float* X1;    // [n][TB][H]
  float* Hh;    // [n][TB][H]
  float* Q;     // [TB n][A], row e n + g
  float* XIN;   // [n][TB][I]
  int TB, tpa, t0, resident;
};

__global__ __launch_bounds__(256) void ffn_actor_ns_fwd_kernel(const FfnNsFwd p) {
  extern __shared__ __attribute__((aligned(16))) float fa_sm[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1, hh = lane >> 5, l31 = lane & 31;
  const Dims& d = p.d;
  const int I = d.I, A = d.A, Ip = (I + 7) & ~7, w1p = p.resident ? Ip + 4 : FA_LD;
  const int g = blockIdx.y;   // < d.n: the grid's y extent
  const float* Pg = p.P + (int64_t)g * p.Pa1;
  const int64_t r0 = (int64_t)g * p.TB;   // agent g's first row of X1 / Hh / XIN
  float* wr_s = fa_sm;
  float* w2_s = wr_s + FA_TILE;
  float* xs = w2_s + FA_TILE;
  float* as = xs + FA_TILE;
  float* w1_s = as + FA_TILE;
  const float* W1 = Pg + p.o_w1;
  for (int i = tid; i < H * H; i += 256) {
    const int j = i >> 6, k = i & 63;
    wr_s[j * FA_LD + k] = Pg[p.o_wr + i];
    w2_s[j * FA_LD + k] = j < A ? Pg[p.o_w2 + i] : 0.0f;
  }
  if (p.resident)
    for (int i = tid; i < H * Ip; i += 256) {
      const int j = i / Ip, k = i - j * Ip;
      w1_s[j * w1p + k] = k < I ? W1[(int64_t)j * I + k] : 0.0f;
    }
  const int col = 32 * wn + l31;
  const float b1 = Pg[p.o_b1 + col], br = Pg[p.o_br + col], b2 = col < A ? Pg[p.o_b2 + col] : 0.0f;
  const int grow = tid >> 2, gk = (tid & 3) * 16;   // the gather: row, first k within the chunk
  const float* a_xs = xs + (32 * wm + l31) * FA_LD + 4 * hh;
  const float* a_as = as + (32 * wm + l31) * FA_LD + 4 * hh;
  const int brow = 32 * wn + l31;

  for (int tile = blockIdx.x; tile < p.tpa; tile += gridDim.x) {
    const int e0 = tile * FA_ROWS, e = e0 + grow;
    const float* orow = nullptr;
    int aprev = -1;
    if (e < p.TB) {   // the row test before the row's first access
      const int tl = (int)fdiv((uint32_t)e, d.dB), b = e - tl * d.B, t = p.t0 + tl;
      const int64_t slot = p.rp.ep(b) * d.t_stride + t;
      orow = p.rp.obs + (slot * d.n + g) * (int64_t)d.O;
      if (d.last_action && t > 0 && p.rp.filled[slot - 1]) aprev = (int)p.rp.actions[(slot - 1) * d.n + g];
    }
    // ---- fc1, one 64-wide K chunk at a time
    f32x16 acc = fa_zero();
    for (int kc = 0; kc < Ip; kc += H) {
      __syncthreads();   // XS (and a streamed W1 chunk) are free: the last reads were the previous chunk's / tile's
      if (!p.resident)
        for (int i = tid; i < H * H; i += 256) {
          const int j = i >> 6, k = kc + (i & 63);
          w1_s[j * FA_LD + (i & 63)] = k < I ? W1[(int64_t)j * I + k] : 0.0f;
        }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k = kc + gk + 4 * q;
        float r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (orow) {
          if (k + 3 < d.O) {
            ld4u(orow + k, r);
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int kk = k + i;
              if (kk < d.O) {
                r[i] = orow[kk];
              } else if (kk < I) {
                int f = kk - d.O;
                if (d.last_action) {
                  if (f < A) r[i] = f == aprev ? 1.0f : 0.0f;
                  f -= A;
                }
                if (f >= 0 && f == g) r[i] = 1.0f;
              }
            }
          }
          float* dst = p.XIN + (r0 + e) * I + k;
          if ((I & 3) == 0 && k + 3 < I) {
            *(f32x4*)dst = f32x4{r[0], r[1], r[2], r[3]};
          } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (k + i < I) dst[i] = r[i];
          }
        }
        *(f32x4*)&xs[grow * FA_LD + gk + 4 * q] = f32x4{r[0], r[1], r[2], r[3]};
      }
      __syncthreads();
      fa_mma(acc, a_xs, w1_s + brow * w1p + (p.resident ? kc : 0) + 4 * hh, min(H, Ip - kc));
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = 32 * wm + acc_row(reg, lane);
      const float v = fmaxf(acc[reg] + b1, 0.0f);
      as[row * FA_LD + col] = v;
      if (e0 + row < p.TB) p.X1[(r0 + e0 + row) * H + col] = v;
    }
    __syncthreads();   // X1 is in AS; every wave is past its last read of XS
    // ---- rnn: Hh = relu(X1 Wr^T + br) into XS
    acc = fa_zero();
    fa_mma(acc, a_as, wr_s + brow * FA_LD + 4 * hh, H);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = 32 * wm + acc_row(reg, lane);
      const float v = fmaxf(acc[reg] + br, 0.0f);
      xs[row * FA_LD + col] = v;
      if (e0 + row < p.TB) p.Hh[(r0 + e0 + row) * H + col] = v;
    }
    __syncthreads();
    // ---- fc2: logits = Hh W2^T + b2, columns < A, to row e n + g
    if (32 * wn < A) {
      acc = fa_zero();
      fa_mma(acc, a_xs, w2_s + brow * FA_LD + 4 * hh, H);
      if (col < A) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int row = 32 * wm + acc_row(reg, lane);
          if (e0 + row < p.TB) p.Q[((int64_t)(e0 + row) * d.n + g) * A + col] = acc[reg] + b2;
        }
      }
    }
  }
}

struct FfnNsBwd {
  const float* dL;   // [TB n][Ap], row e n + g, pad columns zero
  int Ap, A, n;
  const float* P;    // [n][Pa1]
  int64_t Pa1, o_wr, o_w2;
  const float* Hh;   // [n][TB][H]
  const float* X1;   // [n][TB][H]
  float* dP1;        // [n][TB][H]
  float* slab;       // [gridDim.x][n][Pa1]: this kernel writes [dWr | dbr | dW2 | db2] at o_wr of block g
  int TB, tpa, tpb;  // rows and tiles per agent, tiles per workgroup
};

__global__ __launch_bounds__(256) void ffn_actor_ns_bwd_kernel(const FfnNsBwd p) {
  extern __shared__ __attribute__((aligned(16))) float fa_sm[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1, hh = lane >> 5, l31 = lane & 31;
  const int A = p.A, Ap = p.Ap, A8 = (A + 7) & ~7;
  const int g = blockIdx.y;   // < p.n: the grid's y extent
  const float* Pg = p.P + (int64_t)g * p.Pa1;
  const int64_t r0 = (int64_t)g * p.TB;
  float* w2t = fa_sm;
  float* wrt = w2t + FA_TILE;
  float* dl = wrt + FA_TILE;
  float* dlt = dl + FA_TILE;
  float* hht = dlt + FA_TILE;
  float* x1t = hht + FA_TILE;
  float* dp2 = x1t + FA_TILE;
  float* dp2t = dp2 + FA_TILE;
  for (int i = tid; i < H * H; i += 256) {   // T[k][j] = src[j][k]
    const int j = i >> 6, k = i & 63;
    wrt[k * FA_LD + j] = Pg[p.o_wr + i];
    w2t[k * FA_LD + j] = j < A ? Pg[p.o_w2 + i] : 0.0f;
  }
  const int ao = (32 * wm + l31) * FA_LD + 4 * hh, bo = (32 * wn + l31) * FA_LD + 4 * hh, col = 32 * wn + l31;
  f32x16 acc_w2 = fa_zero(), acc_wr = fa_zero();
  float bsum = 0.0f;   // threads 0-63: db2[tid]; 64-127: dbr[tid - 64]
  const int t0 = blockIdx.x * p.tpb, t1 = min(p.tpa, t0 + p.tpb);
  for (int tile = t0; tile < t1; ++tile) {
    const int e0 = tile * FA_ROWS;
    __syncthreads();   // the previous tile's reads are over (first tile: the weights are in)
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int row = (tid >> 4) + 16 * ps, c4 = (tid & 15) * 4;
      const int e = e0 + row;
      const bool live = e < p.TB;   // before the row's first access
      float r[4];
      ld4(live && c4 < Ap ? p.dL + ((int64_t)e * p.n + g) * Ap + c4 : nullptr, r);
      *(f32x4*)&dl[row * FA_LD + c4] = f32x4{r[0], r[1], r[2], r[3]};
#pragma unroll
      for (int i = 0; i < 4; ++i) dlt[(c4 + i) * FA_LD + row] = r[i];
      ld4(live ? p.Hh + (r0 + e) * H + c4 : nullptr, r);
#pragma unroll
      for (int i = 0; i < 4; ++i) hht[(c4 + i) * FA_LD + row] = r[i];
      ld4(live ? p.X1 + (r0 + e) * H + c4 : nullptr, r);
#pragma unroll
      for (int i = 0; i < 4; ++i) x1t[(c4 + i) * FA_LD + row] = r[i];
    }
    __syncthreads();
    // ---- dP2 = (dL W2) [Hh > 0]
    f32x16 acc = fa_zero();
    fa_mma(acc, dl + ao, w2t + bo, A8);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = 32 * wm + acc_row(reg, lane);
      const float v = hht[col * FA_LD + row] > 0.0f ? acc[reg] : 0.0f;
      dp2[row * FA_LD + col] = v;
      dp2t[col * FA_LD + row] = v;
    }
    __syncthreads();
    // ---- dP1 = (dP2 Wr) [X1 > 0]
    acc = fa_zero();
    fa_mma(acc, dp2 + ao, wrt + bo, H);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = 32 * wm + acc_row(reg, lane);
      if (e0 + row < p.TB) p.dP1[(r0 + e0 + row) * H + col] = x1t[col * FA_LD + row] > 0.0f ? acc[reg] : 0.0f;
    }
    // ---- the weight gradients: dW2 += dL^T Hh, dWr += dP2^T X1, and the two bias sums
    if (32 * wm < A) fa_mma(acc_w2, dlt + ao, hht + bo, FA_ROWS);
    fa_mma(acc_wr, dp2t + ao, x1t + bo, FA_ROWS);
    if (tid < 2 * H) {
      const f32x4* rr = (const f32x4*)((tid < H ? dlt : dp2t) + (tid & 63) * FA_LD);
      float s = 0.0f;
#pragma unroll
      for (int i = 0; i < FA_ROWS / 4; ++i) s += (rr[i][0] + rr[i][1]) + (rr[i][2] + rr[i][3]);
      bsum += s;
    }
  }
  float* out = p.slab + ((int64_t)blockIdx.x * p.n + g) * p.Pa1 + p.o_wr;
  float* ow2 = out + H * H + H;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int row = 32 * wm + acc_row(reg, lane);
    out[row * H + col] = acc_wr[reg];
    if (row < A) ow2[row * H + col] = acc_w2[reg];
  }
  if (tid < H) {
    if (tid < A) ow2[A * H + tid] = bsum;
  } else if (tid < 2 * H) {
    out[H * H + tid - H] = bsum;
  }
}

// Rows [kb, ke) of the agent-major arrays that slice s of agent g sums: `rps` = 64 tpb consecutive e of the agent's TB,
// the last slice the rest (the host probe tests/host/actor_ns_probe.cpp reads the same function).
__host__ __device__ inline void ffn_ns_slice(int TB, int rps, int g, int s, int& kb, int& ke) {
  kb = g * TB + s * rps;
  ke = g * TB + ((s + 1) * rps < TB ? (s + 1) * rps : TB);
}

// [dW1 | db1] of agent g = z / ns over slice s = z % ns of its rows: Dw1Prob over the agent-major dP1 / XIN, into the
// head of block g of gradient slab s.
struct FfnNsDw1Prob {
  static constexpr int BN = 128;
  int I;
  const float* dP1;   // [n][TB][H]
  const float* XIN;   // [n][TB][I]
  float* slab;        // [ns][n][Pa1]
  int64_t Pa1;
  int n, ns, TB, rps;
  using APat = MPat;
  using BPat = MPat;
  static constexpr bool kRowSum = true;
  struct Ctx {
    int f0;
  };
  MQ_DEV Ctx make_ctx(int, int n0, int, int tid) const { return Ctx{n0 + MPat::row(tid)}; }
  MQ_DEV void krange(int z, int& kb, int& ke) const {   // rows of the agent-major arrays: inside [g TB, (g + 1) TB)
    const int g = z / ns;
    ffn_ns_slice(TB, rps, g, z - g * ns, kb, ke);
  }
  MQ_DEV float* out(int z) const {
    const int g = z / ns, s = z - g * ns;
    return slab + ((int64_t)s * n + g) * Pa1;
  }
  MQ_DEV void load_a(const Ctx&, int k0, int ke, float (&r)[4]) const {
    const int j = MPat::row(threadIdx.x), k = k0 + MPat::kq(threadIdx.x);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (k + i < ke) ? dP1[(int64_t)(k + i) * H + j] : 0.0f;
  }
  MQ_DEV void load_b(const Ctx& c, int pass, int k0, int ke, float (&r)[4]) const {
    const int f = c.f0 + 64 * pass, k = k0 + MPat::kq(threadIdx.x);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (f < I && k + i < ke) ? XIN[(int64_t)(k + i) * I + f] : 0.0f;
  }
  MQ_DEV void epilogue(const Ctx&, const f32x16& acc, int mrow0, int ncol0, int z, int lane) const {
    const int f = ncol0 + (lane & 31);
    if (f >= I) return;
    float* o = out(z);
    for_tile(acc, mrow0, ncol0, lane, [&](int j, int ff, float v) {
      if (j < H) o[(int64_t)j * I + ff] = v;
    });
  }
  MQ_DEV void rowsum_out(int j, int z, float v) const {
    if (j < H) out(z)[H * I + j] = v;
  }
};

}  // namespace mq
