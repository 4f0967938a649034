// The feed-forward actor of the actor-critic and PPO learners (ma_config.agent = MQ_AGENT_FFN; epymarl's
// use_rnn: False), fused: ffn_kernels.hpp's agent
//   x1 = relu(fc1(xin));  h = relu(rnn(x1));  logits = fc2(h)          rnn = Linear(64, 64)
// over the RT = T R independent rows of the online net, as one forward and one backward launch with the activations
// and their gradients handed from layer to layer through LDS. fp32 throughout, v_mfma_f32_32x32x2_f32.
//
// Both kernels work on 64-row tiles with 256 threads = 4 waves as 2 x 2: wave w owns the 32 x 32 output tile
// (rows 32 (w >> 1), columns 32 (w & 1)) of every 64 x 64 product, one f32x16 accumulator each. Every LDS operand is
// [64][k] with k contiguous and a pitch of k + 4 floats, k a multiple of 8: the pitch is 4 x an odd number, so the
// eight rows a ds_read_b128 serves at once start 16 bytes apart modulo 128 and cover the banks without a conflict.
// A lane reads four consecutive k of its row per b128 (lanes 0-31 k .. k + 3, lanes 32-63 k + 4 .. k + 7) and feeds
// them to four MFMAs: MFMA m of an 8-deep step pairs k + m with k + 4 + m in both operands, a permutation of the sum.
//
// ffn_actor_fwd_kernel   LDS (floats, FA_TILE = 64 * 68 = 4352):
//   Wr [64][68] | W2 [64][68], rows >= A zero | XS [64][68] | AS [64][68] | W1
//   XS holds the tile's xin one 64-wide K chunk at a time (gathered as Fc1Prob gathers it, rows >= RT and k >= I
//   zero, and written to XIN on the way), then Hh; AS holds X1. W1 is resident as [64][Ip + 4], Ip = I rounded up to
//   8, when those 256 (Ip + 4) bytes fit kFfnActorW1Budget = 64 KB (I <= 248); else it is streamed as the [64][68]
//   chunk that goes with XS. Bytes: 4 * 17408 + 256 (Ip + 4) resident (at most 135,168), 5 * 17408 = 87,040
//   streamed: any obs_dim is served. Wr and W2 (and a resident W1) are loaded once per workgroup, which walks tiles
//   blockIdx.x, blockIdx.x + gridDim.x, ..; logits columns >= A are never stored, and a wave whose 32 columns lie at
//   or past A skips fc2.
//
// ffn_actor_bwd_kernel   LDS: eight [64][68] arrays = 139,264 B, whatever I and A are:
//   W2T [j][a] | WrT [k][j] | DL [row][a] | DLT [a][row] | HhT [j][row] | X1T [k][row] | DP2 [row][j] | DP2T [j][row]
//   W2T (columns a >= A zero) and WrT are resident. Per tile: dP2 = (DL W2T^T) [HhT > 0] to DP2 / DP2T,
//   dP1 = (DP2 WrT^T) [X1T > 0] to Work::dP1 (the one operand that reaches HBM: Dw1Prob reads it), then
//   dW2 += DLT HhT^T, dWr += DP2T X1T^T, db2 += rowsum DLT, dbr += rowsum DP2T. Rows >= RT are zero in all six tile
//   arrays, so a partial tile adds nothing. A workgroup owns the contiguous tiles [b tpb, (b + 1) tpb) and walks them
//   in order; its dW2 and dWr tiles stay in registers across them: at A = 64 each lane holds 2 x 16 = 32 accumulator
//   registers (and threads 0-127 one bias sum); waves 2 and 3 skip dW2 when A <= 32. One slab
//   [dWr | dbr | dW2 | db2] per workgroup, no atomics: the same plan gives the same sums on every run.
#pragma once
#include "learner_gemms.hpp"

namespace mq {

constexpr int FA_ROWS = 64;               // rows of a tile
constexpr int FA_LD = H + 4;              // pitch of a 64-deep LDS operand
constexpr int FA_TILE = FA_ROWS * FA_LD;  // floats of one [64][68] array
constexpr size_t kFfnActorW1Budget = 64 * 1024;   // W1 resident in LDS up to this many bytes
constexpr size_t kFfnActorLdsMax = 160 * 1024;    // a gfx950 workgroup's LDS
constexpr int kFfnActorFwdBlocks = 512;   // the forward's grid cap
constexpr int kFfnActorBlocks = 256;      // the backward's workgroup (slab) cap: one per CU

inline int ffn_actor_ip(int I) { return (I + 7) & ~7; }
inline bool ffn_actor_w1_resident(int I) { return (size_t)H * (ffn_actor_ip(I) + 4) * sizeof(float) <= kFfnActorW1Budget; }
inline size_t ffn_actor_fwd_lds_bytes(int I) {
  const size_t w1 = ffn_actor_w1_resident(I) ? (size_t)H * (ffn_actor_ip(I) + 4) : (size_t)FA_TILE;
  return (4 * (size_t)FA_TILE + w1) * sizeof(float);
}
constexpr size_t kFfnActorBwdLds = 8 * (size_t)FA_TILE * sizeof(float);

// acc += A B^T over kn (a multiple of 8) k: a / b point at this lane's operand row, 4 (lane >> 5) floats in.
MQ_DEV void fa_mma(f32x16& acc, const float* a, const float* b, int kn) {
  for (int k = 0; k < kn; k += 8) {
    const f32x4 av = *(const f32x4*)(a + k), bv = *(const f32x4*)(b + k);
#pragma unroll
    for (int m = 0; m < 4; ++m) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv[m], acc, 0, 0, 0);
  }
}

MQ_DEV f32x16 fa_zero() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.0f;
  return z;
}

struct FfnActorFwd {
  Dims d;
  Rep rp;
  const float* P;   // the agent's parameters
  int64_t o_w1, o_b1, o_wr, o_br, o_w2, o_b2;
  float* X1;    // [RT][H]
  float* Hh;    // [RT][H]
  float* Q;     // [RT][A]
  float* XIN;   // [RT][I]
  int64_t RT;
  int ntiles, resident;
};

__global__ __launch_bounds__(256) void ffn_actor_fwd_kernel(const FfnActorFwd p) {
  extern __shared__ __attribute__((aligned(16))) float fa_sm[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1, hh = lane >> 5, l31 = lane & 31;
  const Dims& d = p.d;
  const int I = d.I, A = d.A, Ip = (I + 7) & ~7, w1p = p.resident ? Ip + 4 : FA_LD;
  float* wr_s = fa_sm;
  float* w2_s = wr_s + FA_TILE;
  float* xs = w2_s + FA_TILE;
  float* as = xs + FA_TILE;
  float* w1_s = as + FA_TILE;
  const float* W1 = p.P + p.o_w1;
  for (int i = tid; i < H * H; i += 256) {
    const int j = i >> 6, k = i & 63;
    wr_s[j * FA_LD + k] = p.P[p.o_wr + i];
    w2_s[j * FA_LD + k] = j < A ? p.P[p.o_w2 + i] : 0.0f;
  }
  if (p.resident)
    for (int i = tid; i < H * Ip; i += 256) {
      const int j = i / Ip, k = i - j * Ip;
      w1_s[j * w1p + k] = k < I ? W1[(int64_t)j * I + k] : 0.0f;
    }
  const int col = 32 * wn + l31;
  const float b1 = p.P[p.o_b1 + col], br = p.P[p.o_br + col], b2 = col < A ? p.P[p.o_b2 + col] : 0.0f;
  const int grow = tid >> 2, gk = (tid & 3) * 16;   // the gather: row, first k within the chunk
  const float* a_xs = xs + (32 * wm + l31) * FA_LD + 4 * hh;   // A operand out of XS / AS, B out of a weight
  const float* a_as = as + (32 * wm + l31) * FA_LD + 4 * hh;
  const int brow = (32 * wn + l31);

  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int64_t m0 = (int64_t)tile * FA_ROWS, m = m0 + grow;
    const float* orow = nullptr;
    int aprev = -1, ag = -1;
    if (m < p.RT) {   // the row test before the row's first access
      int t, r, b;
      split_tr(d, (uint32_t)m, t, r, b, ag);
      const int64_t slot = p.rp.ep(b) * d.t_stride + t;
      orow = p.rp.obs + (slot * d.n + ag) * (int64_t)d.O;
      if (d.last_action && t > 0 && p.rp.filled[slot - 1]) aprev = (int)p.rp.actions[(slot - 1) * d.n + ag];
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
                if (f >= 0 && f == ag) r[i] = 1.0f;
              }
            }
          }
          float* dst = p.XIN + m * I + k;
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
      if (m0 + row < p.RT) p.X1[(m0 + row) * H + col] = v;
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
      if (m0 + row < p.RT) p.Hh[(m0 + row) * H + col] = v;
    }
    __syncthreads();
    // ---- fc2: logits = Hh W2^T + b2, columns < A
    if (32 * wn < A) {
      acc = fa_zero();
      fa_mma(acc, a_xs, w2_s + brow * FA_LD + 4 * hh, H);
      if (col < A) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int row = 32 * wm + acc_row(reg, lane);
          if (m0 + row < p.RT) p.Q[(m0 + row) * A + col] = acc[reg] + b2;
        }
      }
    }
  }
}

struct FfnActorBwd {
  const float* dL;   // [RT][Ap], pad columns zero
  int Ap, A;
  const float* W2;   // fc2.weight [A][H]
  const float* Wr;   // rnn.weight [H][H]
  const float* Hh;   // [RT][H]
  const float* X1;   // [RT][H]
  float* dP1;        // [RT][H]
  float* slab;       // [gridDim.x][len]: dWr (H H) | dbr (H) | dW2 (A H) | db2 (A)
  int64_t len, RT;
  int ntiles, tpb;   // tiles in all, tiles per workgroup
};

__global__ __launch_bounds__(256) void ffn_actor_bwd_kernel(const FfnActorBwd p) {
  extern __shared__ __attribute__((aligned(16))) float fa_sm[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1, hh = lane >> 5, l31 = lane & 31;
  const int A = p.A, Ap = p.Ap, A8 = (A + 7) & ~7;
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
    wrt[k * FA_LD + j] = p.Wr[i];
    w2t[k * FA_LD + j] = j < A ? p.W2[i] : 0.0f;
  }
  const int ao = (32 * wm + l31) * FA_LD + 4 * hh, bo = (32 * wn + l31) * FA_LD + 4 * hh, col = 32 * wn + l31;
  f32x16 acc_w2 = fa_zero(), acc_wr = fa_zero();
  float bsum = 0.0f;   // threads 0-63: db2[tid]; 64-127: dbr[tid - 64]
  const int t0 = blockIdx.x * p.tpb, t1 = min(p.ntiles, t0 + p.tpb);
  for (int tile = t0; tile < t1; ++tile) {
    const int64_t m0 = (int64_t)tile * FA_ROWS;
    __syncthreads();   // the previous tile's reads are over (first tile: the weights are in)
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int row = (tid >> 4) + 16 * ps, c4 = (tid & 15) * 4;
      const int64_t m = m0 + row;
      const bool live = m < p.RT;   // before the row's first access
      float r[4];
      ld4(live && c4 < Ap ? p.dL + m * Ap + c4 : nullptr, r);
      *(f32x4*)&dl[row * FA_LD + c4] = f32x4{r[0], r[1], r[2], r[3]};
#pragma unroll
      for (int i = 0; i < 4; ++i) dlt[(c4 + i) * FA_LD + row] = r[i];
      ld4(live ? p.Hh + m * H + c4 : nullptr, r);
#pragma unroll
      for (int i = 0; i < 4; ++i) hht[(c4 + i) * FA_LD + row] = r[i];
      ld4(live ? p.X1 + m * H + c4 : nullptr, r);
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
      if (m0 + row < p.RT) p.dP1[(m0 + row) * H + col] = x1t[col * FA_LD + row] > 0.0f ? acc[reg] : 0.0f;
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
  float* out = p.slab + (int64_t)blockIdx.x * p.len;
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

}  // namespace mq
