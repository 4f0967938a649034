// The two-layer QMIX hypernetwork (upstream PyMARL's hypernet_layers: 2), fp32 on the MFMA GEMM core (gemm_f32.hpp):
//   hyper_w_1     = Linear(S, He) -> ReLU -> Linear(He, E n)
//   hyper_w_final = Linear(S, He) -> ReLU -> Linear(He, E)
// hyper_b_1 and V.0 stay single state-fed layers. The mixer tail (mix_kernels.hpp) reads HYP[z][m][NH] and writes
// dHYP[m][NH], NH = E (n + 3) columns [hyper_w_1 | hyper_w_final | hyper_b_1 | V.0], exactly as with one layer; the
// launches here produce that HYP and consume that dHYP, so no mixer, TD(lambda), PER, GRU or BPTT kernel changes.
//
// Layer-1 tensor A1[z][m][N1], N1 = 2 He + 2 E columns [hyper_w_1.0 | hyper_w_final.0 | hyper_b_1 | V.0]
// (pre-activations: the ReLU is applied where A1 is read).
//
//   Hyp1Prob     A1[z] = state_{t+z} W1^T + b1 for both nets (HypProb with this layout's segments); z = 0 writes S0
//   Hyp2FwdProb  HYP[z][m][0:nE]    = relu(A1[z][m][0:He])   W12^T + b12
//                HYP[z][m][nE:nE+E] = relu(A1[z][m][He:2He]) Wf2^T + bf2,  the last 2 E columns copied from A1
//   Hyp2BwdProb  dA1[m][k] = [A1[0][m][k] > 0] sum_j dHYP[m][j] W2[j][k] per branch, the last 2 E columns copied
//   Hyp2DwProb   dW12 = dHYP[:, :nE]^T relu(A1), dWf2 likewise, dW1 = dA1^T S0 over the N1 columns, each bias as the
//                row sum of its left operand; split over m into `ns` slabs of slab_mix (the two-pass reduction sums
//                them in a fixed order: bitwise repeatable)
//
// The two branches of layer 2 read different K ranges of A1 (columns 0 .. He and He .. 2 He), and an output tile may
// hold columns of both (n E is a multiple of 64 only by luck). So layer 2's K axis is the concatenation [0, 2 He): a
// weight row has its He values in its own branch's half and exact zeros in the other (a zero B operand leaves the
// accumulator as it is), and a tile that lies within one branch walks that branch's half only (krange). The weights
// never sit in LDS whole: a workgroup stages its 64 output columns' rows in K stages of 32, so (n E + E) x He floats
// past a CU's 160 KB (n = 27: 229 KB) are streamed like any other B operand.
//
// Bounds, read from the code: every policy guards rows with m < M, columns with their segment's width and K with the
// range's end, loads return 0 past them and nothing is stored past them; the scalar loads need no alignment, so
// He % 4 != 0 and S % 4 != 0 are ordinary cases. He <= MQ_HYPERNET_EMBED_MAX is checked in mq_create.
#pragma once
#include "learner_gemms.hpp"

namespace mq {

// Where the two-layer mixer's state-fed and second-layer tensors lie in the flat buffer, and its widths.
struct Hyp2Lay {
  int64_t w1a, b1a, w12, b12, wfa, bfa, wf2, bf2, hbw, hbb, v0w, v0b;   // hyper_w_1.0 / .2, hyper_w_final.0 / .2, ..
  int He, E, nE, N1;   // hypernet_embed, embed, n * embed, 2 He + 2 E
};

// Layer-1 row c of the concatenation [hyper_w_1.0 (He) | hyper_w_final.0 (He) | hyper_b_1 (E) | V.0 (E)].
MQ_DEV HypSeg hyp1_seg(const Hyp2Lay& Y, int c) {
  HypSeg s;
  if (c < Y.He) { s.w = Y.w1a; s.b = Y.b1a; s.row = c; }
  else if (c < 2 * Y.He) { s.w = Y.wfa; s.b = Y.bfa; s.row = c - Y.He; }
  else if (c < 2 * Y.He + Y.E) { s.w = Y.hbw; s.b = Y.hbb; s.row = c - 2 * Y.He; }
  else { s.w = Y.v0w; s.b = Y.v0b; s.row = c - 2 * Y.He - Y.E; }
  return s;
}

// ---------------------------------------------------------------------------------------------- layer 1
struct Hyp1Prob {
  static constexpr int BN = 64;
  Dims d;
  Rep rp;
  Hyp2Lay Y;
  const float* P0;
  const float* P1;
  float* A1;   // [2][M][N1]
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
    c.brow = nullptr;
    if (nn < Y.N1) {
      const HypSeg s = hyp1_seg(Y, nn);
      c.brow = (z ? P1 : P0) + s.w + (int64_t)s.row * d.S;
    }
    return c;
  }
  MQ_DEV void krange(int, int& kb, int& ke) const { kb = 0; ke = d.S; }
  MQ_DEV void load_a(const Ctx& c, int k0, int ke, float (&r)[4]) const {
    const int k = k0 + KPat::kq(threadIdx.x);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (c.arow && k + i < ke) ? c.arow[k + i] : 0.0f;
    if (S0 && c.arow && blockIdx.z == 0 && blockIdx.y == 0) {
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
    if (j >= Y.N1) return;
    const HypSeg s = hyp1_seg(Y, j);
    const float bj = (z ? P1 : P0)[s.b + s.row];
    float* out = A1 + (int64_t)z * d.M * Y.N1;
    for_tile(acc, mrow0, ncol0, lane, [&](int m, int jj, float v) {
      if (m < d.M) out[(int64_t)m * Y.N1 + jj] = v + bj;
    });
  }
  MQ_DEV void rowsum_out(int, int, float) const {}
};

// ---------------------------------------------------------------------------------------------- layer 2 forward
// grid = (ceil(M / 64), ceil(NH / 64), 2 nets).
struct Hyp2FwdProb {
  static constexpr int BN = 64;
  Hyp2Lay Y;
  const float* P0;
  const float* P1;
  const float* A1;   // [2][M][N1]
  float* HYP;        // [2][M][NH]
  int M, NH;
  using APat = KPat;
  using BPat = KPat;
  static constexpr bool kRowSum = false;
  struct Ctx {
    const float* arow;   // A1[z][m], or NULL past M
    const float* brow;   // this output column's He second-layer weights, or NULL for a copied column
    int boff;            // first K index (in [0, 2 He)) of brow's values
  };
  MQ_DEV Ctx make_ctx(int m0, int n0, int z, int tid) const {
    Ctx c;
    const int m = m0 + KPat::row(tid), j = n0 + KPat::row(tid);
    c.arow = m < M ? A1 + ((int64_t)z * M + m) * Y.N1 : nullptr;
    const float* P = z ? P1 : P0;
    c.brow = nullptr;
    c.boff = 0;
    if (j < Y.nE) { c.brow = P + Y.w12 + (int64_t)j * Y.He; }
    else if (j < Y.nE + Y.E) { c.brow = P + Y.wf2 + (int64_t)(j - Y.nE) * Y.He; c.boff = Y.He; }
    return c;
  }
  // the K range of this workgroup's 64 output columns: its branch's half of [0, 2 He), both halves for a tile that
  // holds columns of both, nothing for a tile of copied columns only
  MQ_DEV void krange(int, int& kb, int& ke) const {
    const int n0 = blockIdx.y * BN, n1 = min(n0 + BN, NH);
    if (n0 >= Y.nE + Y.E) { kb = ke = 0; return; }
    kb = n0 < Y.nE ? 0 : Y.He;
    ke = n1 <= Y.nE ? Y.He : 2 * Y.He;
  }
  MQ_DEV void load_a(const Ctx& c, int k0, int ke, float (&r)[4]) const {
    const int k = k0 + KPat::kq(threadIdx.x);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (c.arow && k + i < ke) ? fmaxf(c.arow[k + i], 0.0f) : 0.0f;
  }
  MQ_DEV void load_b(const Ctx& c, int, int k0, int ke, float (&r)[4]) const {
    const int k = k0 + KPat::kq(threadIdx.x) - c.boff;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      r[i] = (c.brow && k + i >= 0 && k + i < Y.He && k + i + c.boff < ke) ? c.brow[k + i] : 0.0f;
  }
  MQ_DEV void epilogue(const Ctx&, const f32x16& acc, int mrow0, int ncol0, int z, int lane) const {
    const int j = ncol0 + (lane & 31);
    if (j >= NH) return;
    const float* P = z ? P1 : P0;
    const float* a1 = A1 + (int64_t)z * M * Y.N1;
    float* out = HYP + (int64_t)z * M * NH;
    if (j < Y.nE + Y.E) {
      const float bj = j < Y.nE ? P[Y.b12 + j] : P[Y.bf2 + j - Y.nE];
      for_tile(acc, mrow0, ncol0, lane, [&](int m, int jj, float v) {
        if (m < M) out[(int64_t)m * NH + jj] = v + bj;
      });
    } else {   // hyper_b_1 / V.0: layer 1's value as it is
      const int c = 2 * Y.He + j - Y.nE - Y.E;
      for_tile(acc, mrow0, ncol0, lane, [&](int m, int jj, float) {
        if (m < M) out[(int64_t)m * NH + jj] = a1[(int64_t)m * Y.N1 + c];
      });
    }
  }
  MQ_DEV void rowsum_out(int, int, float) const {}
};

// ---------------------------------------------------------------------------------------------- layer 2 backward
// dA1 [M][N1] from dHYP [M][NH] (online net). grid = (ceil(M / 64), ceil(N1 / 64), 1). K runs over the NH columns of
// dHYP that feed a second layer, [0, nE + E): output column c < He takes W12[j][c] for j < nE and zeros beyond, column
// He <= c < 2 He takes Wf2[j - nE][c - He] for j >= nE.
struct Hyp2BwdProb {
  static constexpr int BN = 64;
  Hyp2Lay Y;
  const float* P0;
  const float* A1;     // [M][N1], the online net's
  const float* dHYP;   // [M][NH]
  float* dA1;          // [M][N1]
  int M, NH;
  using APat = KPat;
  using BPat = MPat;
  static constexpr bool kRowSum = false;
  struct Ctx {
    const float* arow;
    int c;   // this thread's B row: output column c
  };
  MQ_DEV Ctx make_ctx(int m0, int n0, int, int tid) const {
    Ctx c;
    const int m = m0 + KPat::row(tid);
    c.arow = m < M ? dHYP + (int64_t)m * NH : nullptr;
    c.c = n0 + MPat::row(tid);
    return c;
  }
  MQ_DEV void krange(int, int& kb, int& ke) const {
    const int n0 = blockIdx.y * BN, n1 = min(n0 + BN, Y.N1);
    if (n0 >= 2 * Y.He) { kb = ke = 0; return; }
    kb = n0 < Y.He ? 0 : Y.nE;
    ke = n1 <= Y.He ? Y.nE : Y.nE + Y.E;
  }
  MQ_DEV void load_a(const Ctx& c, int k0, int ke, float (&r)[4]) const {
    const int k = k0 + KPat::kq(threadIdx.x);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (c.arow && k + i < ke) ? c.arow[k + i] : 0.0f;
  }
  MQ_DEV void load_b(const Ctx& c, int, int k0, int ke, float (&r)[4]) const {
    const int j = k0 + MPat::kq(threadIdx.x);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int jj = j + i;
      float v = 0.0f;
      if (jj < ke) {
        if (c.c < Y.He) { if (jj < Y.nE) v = P0[Y.w12 + (int64_t)jj * Y.He + c.c]; }
        else if (c.c < 2 * Y.He) { if (jj >= Y.nE) v = P0[Y.wf2 + (int64_t)(jj - Y.nE) * Y.He + c.c - Y.He]; }
      }
      r[i] = v;
    }
  }
  MQ_DEV void epilogue(const Ctx&, const f32x16& acc, int mrow0, int ncol0, int, int lane) const {
    const int c = ncol0 + (lane & 31);
    if (c >= Y.N1) return;
    if (c < 2 * Y.He) {
      for_tile(acc, mrow0, ncol0, lane, [&](int m, int cc, float v) {
        if (m < M) {
          const int64_t o = (int64_t)m * Y.N1 + cc;
          dA1[o] = A1[o] > 0.0f ? v : 0.0f;
        }
      });
    } else {   // hyper_b_1 / V.0: the mixer tail's gradient as it is
      const int j = Y.nE + Y.E + c - 2 * Y.He;
      for_tile(acc, mrow0, ncol0, lane, [&](int m, int cc, float) {
        if (m < M) dA1[(int64_t)m * Y.N1 + cc] = dHYP[(int64_t)m * NH + j];
      });
    }
  }
  MQ_DEV void rowsum_out(int, int, float) const {}
};

// ---------------------------------------------------------------------------------------------- weight gradients
// One launch for the three contractions over the mixer rows m, each [out rows j] x [out columns f]:
//   segment 0: dW12 [nE][He] = dHYP[:, 0:nE]^T relu(A1[:, 0:He]),        db12 = column sums of dHYP[:, 0:nE]
//   segment 1: dWf2 [E][He]  = dHYP[:, nE:nE+E]^T relu(A1[:, He:2He]),   dbf2 likewise
//   segment 2: dW1  [N1][S]  = dA1^T S0,                                 db1 = column sums of dA1
// Row tiles of 64: t0 = ceil(nE / 64) tiles of segment 0, then t1 of segment 1, then t2 of segment 2; grid =
// (t0 + t1 + t2, ceil(max(He, S) / 64), ns m-slices). Slice z writes slab z (every element of the mixer's block up to
// V.0.bias, zeros where a slice is empty), in the parameter layout relative to `base` (hyper_w_1.0.weight).
struct Hyp2DwProb {
  static constexpr int BN = 64;
  Hyp2Lay Y;
  const float* A1;     // [M][N1] online
  const float* dA1;    // [M][N1]
  const float* dHYP;   // [M][NH]
  const float* S0;     // [M][S]
  float* slab;         // [ns][len]
  int64_t len, base;
  int M, NH, S, ns, t0, t1;
  using APat = MPat;
  using BPat = MPat;
  static constexpr bool kRowSum = true;
  struct Seg {
    const float* X;   // left operand, column 0 of the segment; row pitch ldx
    const float* Yv;  // right operand
    int ldx, ldy, J, F, relu, seg, j0;   // j0: the tile's first row within the segment
  };
  MQ_DEV Seg seg_of(int row) const {   // row: the launch's global output row (64 per tile)
    Seg s;
    const int tile = row / GBM;
    if (tile < t0) {
      s.seg = 0; s.j0 = row; s.X = dHYP; s.ldx = NH; s.J = Y.nE; s.Yv = A1; s.ldy = Y.N1; s.F = Y.He; s.relu = 1;
    } else if (tile < t0 + t1) {
      s.seg = 1; s.j0 = row - t0 * GBM; s.X = dHYP + Y.nE; s.ldx = NH; s.J = Y.E; s.Yv = A1 + Y.He; s.ldy = Y.N1;
      s.F = Y.He; s.relu = 1;
    } else {
      s.seg = 2; s.j0 = row - (t0 + t1) * GBM; s.X = dA1; s.ldx = Y.N1; s.J = Y.N1; s.Yv = S0; s.ldy = S; s.F = S;
      s.relu = 0;
    }
    return s;
  }
  struct Ctx {
    Seg s;
    int m0, f;
  };
  MQ_DEV Ctx make_ctx(int m0, int n0, int, int tid) const { return Ctx{seg_of(m0), m0, n0 + MPat::row(tid)}; }
  MQ_DEV void krange(int z, int& kb, int& ke) const { krange_split(M, ns, z, kb, ke); }
  MQ_DEV void load_a(const Ctx& c, int k0, int ke, float (&r)[4]) const {
    const int j = c.s.j0 + MPat::row(threadIdx.x), k = k0 + MPat::kq(threadIdx.x);
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = (j < c.s.J && k + i < ke) ? c.s.X[(int64_t)(k + i) * c.s.ldx + j] : 0.0f;
  }
  MQ_DEV void load_b(const Ctx& c, int, int k0, int ke, float (&r)[4]) const {
    const int k = k0 + MPat::kq(threadIdx.x);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = (c.f < c.s.F && k + i < ke) ? c.s.Yv[(int64_t)(k + i) * c.s.ldy + c.f] : 0.0f;
      r[i] = c.s.relu ? fmaxf(v, 0.0f) : v;
    }
  }
  // offsets (weight row start, bias) of segment row j in the slab
  MQ_DEV void out_of(const Seg& s, int j, int64_t& ow, int64_t& ob) const {
    if (s.seg == 0) { ow = Y.w12 + (int64_t)j * Y.He; ob = Y.b12 + j; }
    else if (s.seg == 1) { ow = Y.wf2 + (int64_t)j * Y.He; ob = Y.bf2 + j; }
    else { const HypSeg g = hyp1_seg(Y, j); ow = g.w + (int64_t)g.row * S; ob = g.b + g.row; }
    ow -= base; ob -= base;
  }
  MQ_DEV void epilogue(const Ctx& c, const f32x16& acc, int mrow0, int ncol0, int z, int lane) const {
    const int f = ncol0 + (lane & 31);
    if (f >= c.s.F) return;
    float* out = slab + (int64_t)z * len;
    for_tile(acc, mrow0, ncol0, lane, [&](int m, int ff, float v) {
      const int j = c.s.j0 + (m - c.m0);
      if (j < c.s.J) {
        int64_t ow, ob;
        out_of(c.s, j, ow, ob);
        out[ow + ff] = v;
      }
    });
  }
  MQ_DEV void rowsum_out(int row, int z, float v) const {
    const Seg s = seg_of(row / GBM * GBM);
    const int j = s.j0 + row % GBM;
    if (j < s.J) {
      int64_t ow, ob;
      out_of(s, j, ow, ob);
      slab[(int64_t)z * len + ob] = v;
    }
  }
};

// ---------------------------------------------------------------------------------------------- standalone forward
// QMixer.forward of a two-layer mixer outside train() (mq_qmix_forward2): qmix_forward_kernel (module_fwd.hpp) with the
// hypernet's two phases. W: the mixer's parameters in parameters() order; o: offsets relative to W.
constexpr int QMF2_ROWS = 4;
struct Qmix2Off {
  Hyp2Lay Y;
  int64_t v2w, v2b;
};
inline size_t qmix_forward2_lds(int n, int S, int E, int He) {
  return (size_t)QMF2_ROWS * (S + 2 * (size_t)He + 2 * E + (size_t)E * (n + 3)) * sizeof(float);
}

__global__ __launch_bounds__(256) void qmix_forward2_kernel(const float* __restrict__ W, Qmix2Off o, int n, int S,
                                                            const float* __restrict__ qs,
                                                            const float* __restrict__ st, float* __restrict__ out,
                                                            int rows) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const Hyp2Lay& Y = o.Y;
  const int E = Y.E, He = Y.He, N1 = Y.N1, nE = Y.nE, NH = E * (n + 3);
  float* s_st = lds;                        // [QMF2_ROWS][S]
  float* s_a1 = s_st + QMF2_ROWS * S;       // [QMF2_ROWS][N1]
  float* s_h = s_a1 + QMF2_ROWS * N1;       // [QMF2_ROWS][NH]
  const int m0 = blockIdx.x * QMF2_ROWS;
  for (int e = threadIdx.x; e < QMF2_ROWS * S; e += 256) {
    const int i = e / S, k = e - i * S;
    s_st[e] = m0 + i < rows ? st[(int64_t)(m0 + i) * S + k] : 0.0f;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < N1; c += 256) {   // layer 1 (pre-activations)
    const HypSeg g = hyp1_seg(Y, c);
    const float* wrow = W + g.w + (int64_t)g.row * S;
    float acc[QMF2_ROWS];
#pragma unroll
    for (int i = 0; i < QMF2_ROWS; ++i) acc[i] = 0.0f;
    for (int k = 0; k < S; ++k) {
      const float wk = wrow[k];
#pragma unroll
      for (int i = 0; i < QMF2_ROWS; ++i) acc[i] = fmaf(wk, s_st[i * S + k], acc[i]);
    }
    const float bias = W[g.b + g.row];
#pragma unroll
    for (int i = 0; i < QMF2_ROWS; ++i) s_a1[i * N1 + c] = acc[i] + bias;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < NH; j += 256) {   // layer 2, and the copied columns
    if (j >= nE + E) {
#pragma unroll
      for (int i = 0; i < QMF2_ROWS; ++i) s_h[i * NH + j] = s_a1[i * N1 + 2 * He + j - nE - E];
      continue;
    }
    const float* wrow = j < nE ? W + Y.w12 + (int64_t)j * He : W + Y.wf2 + (int64_t)(j - nE) * He;
    const float bias = j < nE ? W[Y.b12 + j] : W[Y.bf2 + j - nE];
    const int a0 = j < nE ? 0 : He;
    float acc[QMF2_ROWS];
#pragma unroll
    for (int i = 0; i < QMF2_ROWS; ++i) acc[i] = 0.0f;
    for (int k = 0; k < He; ++k) {
      const float wk = wrow[k];
#pragma unroll
      for (int i = 0; i < QMF2_ROWS; ++i) acc[i] = fmaf(wk, fmaxf(s_a1[i * N1 + a0 + k], 0.0f), acc[i]);
    }
#pragma unroll
    for (int i = 0; i < QMF2_ROWS; ++i) s_h[i * NH + j] = acc[i] + bias;
  }
  __syncthreads();
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, m = m0 + wv;
  if (wv >= QMF2_ROWS || m >= rows) return;
  const float* h = s_h + wv * NH;
  float part = 0.0f, vpart = 0.0f;
  if (lane < E) {
    float pre = 0.0f;
    for (int i = 0; i < n; ++i) pre = fmaf(qs[(int64_t)m * n + i], fabsf(h[i * E + lane]), pre);
    pre += h[nE + E + lane];                                       // + b1
    const float hid = pre > 0.0f ? pre : expm1f(pre);              // F.elu
    part = hid * fabsf(h[nE + lane]);                              // bmm(hidden, |w_final|)
    vpart = fmaxf(h[nE + 2 * E + lane], 0.0f) * W[o.v2w + lane];   // V.2(relu(V.0 s))
  }
#pragma unroll
  for (int sh = 32; sh > 0; sh >>= 1) {
    part += __shfl_xor(part, sh, 64);
    vpart += __shfl_xor(vpart, sh, 64);
  }
  if (lane == 0) out[m] = part + (vpart + W[o.v2b]);
}

}  // namespace mq
