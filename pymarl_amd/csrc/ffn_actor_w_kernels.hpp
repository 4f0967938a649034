// The feed-forward actor of the actor-critic and PPO learners at hidden width 128 (ma_config.rnn_hidden_dim = 128 with
// agent = MQ_AGENT_FFN; epymarl's hidden_dim: 128 under use_rnn: False):
//   x1 = relu(fc1(xin));  h = relu(rnn(x1));  logits = fc2(h)          rnn = Linear(128, 128)
// as one forward and one backward launch over the RT = T R rows, fp32 on v_mfma_f32_32x32x2_f32. ffn_actor_kernels.hpp's
// eight [64][68] arrays would be 275 KB at this width, so neither kernel keeps a transposed copy of anything: every LDS
// array is row-major as its source is stored, with a pitch of 4 x an odd number of floats (132, 36, 68).
//
// An MFMA operand whose reduction index runs along the row (xin, X1, Hh, dL, dP2 as the A operand of a row-parallel
// product; W1, Wr, W2 rows as the B operand of the forward) is read as ffn_actor_kernels.hpp reads it: one ds_read_b128
// per lane feeds four MFMAs (fa_mma's k pairing). An operand whose reduction index is the ROW of the stored array (Wr
// and W2 in the backward's dP products; dL, dP2, Hh, X1 in the weight gradients) is read with ds_read_b32, the 32 lanes
// of a half wave along the contiguous column: 32 consecutive banks, no conflict, at four times the LDS instructions.
//
// ffn_actor_w_fwd_kernel   64-row tiles, 256 threads = 4 waves as 2 x 2: wave w owns rows 32 (w >> 1) and the 64 columns
//   64 (w & 1) .. of each 64 x 128 product as two f32x16 accumulators that share their A fragment. LDS (floats):
//   Wr [128][132] 16896 | W2 [64][132] 8448, rows >= A zero | ACT [64][132] 8448 | XS [64][36] 2304 | W1C [128][36] 4608
//   = 40,704 floats = 162,816 B. fc1 streams K in chunks of 32: XS is the tile's gathered xin chunk (rows >= RT and
//   k >= I zero, written to XIN on the way, ffn_actor_fwd_kernel's gather), W1C the chunk of W1. ACT holds X1; once
//   every wave's rnn accumulators are complete (a barrier) Hh overwrites it, and fc2 reads it: a 64 x 64 product, one
//   accumulator per wave, skipped by a wave whose 32 columns lie at or past A. Logits columns >= A are never stored.
//
// ffn_actor_w_bwd_kernel   32-row tiles, 4 waves, wave w owns the 32 columns 32 w .. of every product. LDS (floats):
//   W2 [64][132] 8448, rows >= A zero | Wr [128][132] 16896 | DL [32][68] 2176 | Hh, X1, DP2 [32][132] 3 x 4224
//   = 40,192 floats = 160,768 B. Per tile: dP2 = (DL W2) [Hh > 0] into DP2, dP1 = (DP2 Wr) [X1 > 0] to global (the one
//   operand Dw1's GEMM reads from HBM), then dWr += DP2^T X1 (four accumulators per wave), dW2 += DL^T Hh (two, the
//   second only when A > 32), dbr and db2 as column sums by threads 64-191 and 0-63. Rows >= RT are zero in DL, Hh and
//   X1, hence in DP2: a partial tile adds nothing. A workgroup owns the contiguous tiles [b tpb, (b + 1) tpb) and keeps
//   its 96 accumulator registers across them; one slab [dWr | dbr | dW2 | db2] per workgroup, no atomics: the same plan
//   gives the same bits on every run.
#pragma once
#include "ffn_actor_kernels.hpp"

namespace mq {

constexpr int HW = 128;            // the wide actor's hidden width
constexpr int FW_LD = HW + 4;      // pitch of a 128-deep LDS row
constexpr int FW_ROWS = 64;        // rows of a forward tile
constexpr int FW_KC = 32;          // fc1's K chunk
constexpr int FW_KLD = FW_KC + 4;  // pitch of XS and W1C
constexpr int FWB_ROWS = 32;       // rows of a backward tile
constexpr int FWB_DLD = 64 + 4;    // pitch of DL
constexpr size_t kFfnActorWFwdLds =
    ((size_t)HW * FW_LD + 64 * FW_LD + FW_ROWS * FW_LD + FW_ROWS * FW_KLD + HW * FW_KLD) * sizeof(float);
constexpr size_t kFfnActorWBwdLds =
    ((size_t)64 * FW_LD + HW * FW_LD + FWB_ROWS * FWB_DLD + 3 * FWB_ROWS * FW_LD) * sizeof(float);
static_assert(kFfnActorWFwdLds == 162816 && kFfnActorWBwdLds == 160768, "DESIGN.md §3o's byte counts");
static_assert(kFfnActorWFwdLds <= kFfnActorLdsMax && kFfnActorWBwdLds <= kFfnActorLdsMax, "a workgroup's LDS");

// c0 += A B0^T, c1 += A B1^T over kn (a multiple of 8) k, fa_mma's operand addressing: one A fragment, two B's.
MQ_DEV void fw_mma2(f32x16& c0, f32x16& c1, const float* a, const float* b0, const float* b1, int kn) {
  for (int k = 0; k < kn; k += 8) {
    const f32x4 av = *(const f32x4*)(a + k), bv0 = *(const f32x4*)(b0 + k), bv1 = *(const f32x4*)(b1 + k);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      c0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv0[m], c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv1[m], c1, 0, 0, 0);
    }
  }
}

// acc += A B over kn (a multiple of 8) k with B stored [k][column]: `a` is this lane's A row 4 (lane >> 5) floats in
// (one b128), `b` this lane's column of B's row 4 (lane >> 5) (four b32, ld floats apart). fa_mma's k pairing.
MQ_DEV void fw_mma_kb(f32x16& acc, const float* a, const float* b, int ld, int kn) {
  for (int k = 0; k < kn; k += 8) {
    const f32x4 av = *(const f32x4*)(a + k);
#pragma unroll
    for (int m = 0; m < 4; ++m) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], b[(k + m) * ld], acc, 0, 0, 0);
  }
}

struct FfnActorWFwd {
  Dims d;
  Rep rp;
  const float* P;   // the agent's parameters
  int64_t o_w1, o_b1, o_wr, o_br, o_w2, o_b2;
  float* X1;    // [RT][HW]
  float* Hh;    // [RT][HW]
  float* Q;     // [RT][A]
  float* XIN;   // [RT][I]
  int64_t RT;
  int ntiles, t0;   // 64-row tiles; the stored step of row block t = 0 (acting: one step of the batch)
};

__global__ __launch_bounds__(256) void ffn_actor_w_fwd_kernel(const FfnActorWFwd p) {
  extern __shared__ __attribute__((aligned(16))) float fw_sm[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1, hh = lane >> 5, l31 = lane & 31;
  const Dims& d = p.d;
  const int I = d.I, A = d.A, Ip = (I + 7) & ~7;
  float* wr_s = fw_sm;
  float* w2_s = wr_s + HW * FW_LD;
  float* act = w2_s + 64 * FW_LD;
  float* xs = act + FW_ROWS * FW_LD;
  float* w1c = xs + FW_ROWS * FW_KLD;
  const float* W1 = p.P + p.o_w1;
  for (int i = tid; i < HW * HW; i += 256) wr_s[(i >> 7) * FW_LD + (i & 127)] = p.P[p.o_wr + i];
  for (int i = tid; i < 64 * HW; i += 256) w2_s[(i >> 7) * FW_LD + (i & 127)] = (i >> 7) < A ? p.P[p.o_w2 + i] : 0.0f;
  const int c0 = 64 * wn + l31, c2 = 32 * wn + l31;   // this lane's columns: c0 and c0 + 32 of 128; c2 of fc2's 64
  const float b1[2] = {p.P[p.o_b1 + c0], p.P[p.o_b1 + c0 + 32]}, br[2] = {p.P[p.o_br + c0], p.P[p.o_br + c0 + 32]};
  const float b2 = c2 < A ? p.P[p.o_b2 + c2] : 0.0f;
  const int grow = tid >> 2, gk = (tid & 3) * 8;   // the gather: row, first k within the chunk
  const float* a_xs = xs + (32 * wm + l31) * FW_KLD + 4 * hh;
  const float* a_act = act + (32 * wm + l31) * FW_LD + 4 * hh;
  const float* b_w1 = w1c + c0 * FW_KLD + 4 * hh;
  const float* b_wr = wr_s + c0 * FW_LD + 4 * hh;

  for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
    const int64_t m0 = (int64_t)tile * FW_ROWS, m = m0 + grow;
    const float* orow = nullptr;
    int aprev = -1, ag = -1;
    if (m < p.RT) {   // the row test before the row's first access
      int t, r, b;
      split_tr(d, (uint32_t)m, t, r, b, ag);
      const int64_t slot = p.rp.ep(b) * d.t_stride + t + p.t0;
      orow = p.rp.obs + (slot * d.n + ag) * (int64_t)d.O;
      if (d.last_action && t + p.t0 > 0 && p.rp.filled[slot - 1]) aprev = (int)p.rp.actions[(slot - 1) * d.n + ag];
    }
    // ---- fc1, one 32-wide K chunk at a time
    f32x16 acc0 = fa_zero(), acc1 = fa_zero();
    for (int kc = 0; kc < Ip; kc += FW_KC) {
      __syncthreads();   // XS and W1C are free, and (first chunk) every wave is past the previous tile's fc2
      for (int i = tid; i < HW * FW_KC; i += 256) {
        const int j = i >> 5, k = kc + (i & 31);
        w1c[j * FW_KLD + (i & 31)] = k < I ? W1[(int64_t)j * I + k] : 0.0f;
      }
#pragma unroll
      for (int q = 0; q < 2; ++q) {
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
        *(f32x4*)&xs[grow * FW_KLD + gk + 4 * q] = f32x4{r[0], r[1], r[2], r[3]};
      }
      __syncthreads();
      fw_mma2(acc0, acc1, a_xs, b_w1, b_w1 + 32 * FW_KLD, min(FW_KC, Ip - kc));
    }
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = 32 * wm + acc_row(reg, lane);
      const float v0 = fmaxf(acc0[reg] + b1[0], 0.0f), v1 = fmaxf(acc1[reg] + b1[1], 0.0f);
      act[row * FW_LD + c0] = v0;
      act[row * FW_LD + c0 + 32] = v1;
      if (m0 + row < p.RT) {
        p.X1[(m0 + row) * HW + c0] = v0;
        p.X1[(m0 + row) * HW + c0 + 32] = v1;
      }
    }
    __syncthreads();   // X1 is in ACT
    // ---- rnn: Hh = relu(X1 Wr^T + br), over X1 in ACT once every wave has read it
    acc0 = fa_zero();
    acc1 = fa_zero();
    fw_mma2(acc0, acc1, a_act, b_wr, b_wr + 32 * FW_LD, HW);
    __syncthreads();   // every wave's rnn accumulators are complete: ACT is free
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = 32 * wm + acc_row(reg, lane);
      const float v0 = fmaxf(acc0[reg] + br[0], 0.0f), v1 = fmaxf(acc1[reg] + br[1], 0.0f);
      act[row * FW_LD + c0] = v0;
      act[row * FW_LD + c0 + 32] = v1;
      if (m0 + row < p.RT) {
        p.Hh[(m0 + row) * HW + c0] = v0;
        p.Hh[(m0 + row) * HW + c0 + 32] = v1;
      }
    }
    __syncthreads();
    // ---- fc2: logits = Hh W2^T + b2, columns < A
    if (32 * wn < A) {
      acc0 = fa_zero();
      fa_mma(acc0, a_act, w2_s + c2 * FW_LD + 4 * hh, HW);
      if (c2 < A) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int row = 32 * wm + acc_row(reg, lane);
          if (m0 + row < p.RT) p.Q[(m0 + row) * A + c2] = acc0[reg] + b2;
        }
      }
    }
  }
}

struct FfnActorWBwd {
  const float* dL;   // [RT][Ap], pad columns zero
  int Ap, A;
  const float* W2;   // fc2.weight [A][HW]
  const float* Wr;   // rnn.weight [HW][HW]
  const float* Hh;   // [RT][HW]
  const float* X1;   // [RT][HW]
  float* dP1;        // [RT][HW]
  float* slab;       // [gridDim.x][len]: dWr (HW HW) | dbr (HW) | dW2 (A HW) | db2 (A)
  int64_t len, RT;
  int ntiles, tpb;   // 32-row tiles in all, tiles per workgroup
};

__global__ __launch_bounds__(256) void ffn_actor_w_bwd_kernel(const FfnActorWBwd p) {
  extern __shared__ __attribute__((aligned(16))) float fw_sm[];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, hh = lane >> 5, l31 = lane & 31;
  const int A = p.A, Ap = p.Ap, A8 = (A + 7) & ~7;
  float* w2_s = fw_sm;
  float* wr_s = w2_s + 64 * FW_LD;
  float* dl = wr_s + HW * FW_LD;
  float* hh_s = dl + FWB_ROWS * FWB_DLD;
  float* x1_s = hh_s + FWB_ROWS * FW_LD;
  float* dp2 = x1_s + FWB_ROWS * FW_LD;
  for (int i = tid; i < HW * HW; i += 256) wr_s[(i >> 7) * FW_LD + (i & 127)] = p.Wr[i];
  for (int i = tid; i < 64 * HW; i += 256) w2_s[(i >> 7) * FW_LD + (i & 127)] = (i >> 7) < A ? p.W2[i] : 0.0f;
  const int col = 32 * w + l31;   // this lane's column of every product
  f32x16 acc_wr[4], acc_w2[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc_wr[i] = fa_zero();
  acc_w2[0] = fa_zero();
  acc_w2[1] = fa_zero();
  float bsum = 0.0f;   // threads 0-63: db2[tid]; 64-191: dbr[tid - 64]
  const int t0 = blockIdx.x * p.tpb, t1 = min(p.ntiles, t0 + p.tpb);
  for (int tile = t0; tile < t1; ++tile) {
    const int64_t m0 = (int64_t)tile * FWB_ROWS;
    __syncthreads();   // the previous tile's reads are over (first tile: the weights are in)
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int idx = tid + 256 * ps, row = idx >> 5, c4 = (idx & 31) * 4;
      const int64_t m = m0 + row;
      const bool live = m < p.RT;   // before the row's first access
      float r[4];
      ld4(live ? p.Hh + m * HW + c4 : nullptr, r);
      *(f32x4*)&hh_s[row * FW_LD + c4] = f32x4{r[0], r[1], r[2], r[3]};
      ld4(live ? p.X1 + m * HW + c4 : nullptr, r);
      *(f32x4*)&x1_s[row * FW_LD + c4] = f32x4{r[0], r[1], r[2], r[3]};
    }
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
      const int idx = tid + 256 * ps, row = idx >> 4, c4 = (idx & 15) * 4;
      const int64_t m = m0 + row;
      float r[4];
      ld4(m < p.RT && c4 < Ap ? p.dL + m * Ap + c4 : nullptr, r);
      *(f32x4*)&dl[row * FWB_DLD + c4] = f32x4{r[0], r[1], r[2], r[3]};
    }
    __syncthreads();
    // ---- dP2 = (dL W2) [Hh > 0]: the reduction index a is W2's row
    f32x16 acc = fa_zero();
    fw_mma_kb(acc, dl + l31 * FWB_DLD + 4 * hh, w2_s + 4 * hh * FW_LD + col, FW_LD, A8);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = acc_row(reg, lane);
      dp2[row * FW_LD + col] = hh_s[row * FW_LD + col] > 0.0f ? acc[reg] : 0.0f;
    }
    __syncthreads();
    // ---- dP1 = (dP2 Wr) [X1 > 0]: the reduction index j is Wr's row
    acc = fa_zero();
    fw_mma_kb(acc, dp2 + l31 * FW_LD + 4 * hh, wr_s + 4 * hh * FW_LD + col, FW_LD, HW);
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int row = acc_row(reg, lane);
      if (m0 + row < p.RT) p.dP1[(m0 + row) * HW + col] = x1_s[row * FW_LD + col] > 0.0f ? acc[reg] : 0.0f;
    }
    // ---- the weight gradients, the reduction index the tile row: dWr += dP2^T X1, dW2 += dL^T Hh
    for (int r = hh; r < FWB_ROWS; r += 2) {   // an MFMA takes row r from lanes 0-31 and r + 1 from lanes 32-63
      const float bx = x1_s[r * FW_LD + col], bh = hh_s[r * FW_LD + col];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
        acc_wr[jt] = __builtin_amdgcn_mfma_f32_32x32x2f32(dp2[r * FW_LD + 32 * jt + l31], bx, acc_wr[jt], 0, 0, 0);
      acc_w2[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(dl[r * FWB_DLD + l31], bh, acc_w2[0], 0, 0, 0);
      if (A > 32) acc_w2[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(dl[r * FWB_DLD + 32 + l31], bh, acc_w2[1], 0, 0, 0);
    }
    if (tid < 64 + HW) {   // the two bias sums, rows in order
      const float* src = tid < 64 ? dl + tid : dp2 + (tid - 64);
      const int ld = tid < 64 ? FWB_DLD : FW_LD;
      float s = 0.0f;
#pragma unroll
      for (int r = 0; r < FWB_ROWS; ++r) s += src[r * ld];
      bsum += s;
    }
  }
  float* out = p.slab + (int64_t)blockIdx.x * p.len;
  float* ow2 = out + HW * HW + HW;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int row = acc_row(reg, lane);
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) out[(32 * jt + row) * HW + col] = acc_wr[jt][reg];
    if (row < A) ow2[row * HW + col] = acc_w2[0][reg];
    if (32 + row < A) ow2[(32 + row) * HW + col] = acc_w2[1][reg];
  }
  if (tid < 64) {
    if (tid < A) ow2[A * HW + tid] = bsum;
  } else if (tid < 64 + HW) {
    out[HW * HW + tid - 64] = bsum;
  }
}

}  // namespace mq
