// Two opt-ins of the QMIX / VDN / IQL learner that epymarl's configs carry and the reference lacks: Polyak (soft)
// target updates (target_update_interval_or_tau <= 1, mq_set_soft_target) and reward standardisation with running
// statistics (standardise_rewards, mq_set_reward_norm). Neither touches the forward recurrence or the BPTT.
//
// soft_update_kernel, the step's last launch (after the apply): over the flat [P] buffers
//   target = target * (1 - tau) + online * tau
// in fp32, both products and the sum rounded separately (contraction off), 1 - tau formed in double on the host and
// cast once: bitwise what torch's CPU fp32 gives for t * (1.0 - tau) + p * tau. The elements between the first and the
// last 16-byte boundary go as float4 when both pointers agree modulo 16 bytes (else everything is scalar), head and
// tail as scalars: apply_adam_kernel's scheme (optim_kernels.hpp). Elementwise, so the result does not depend on the
// vector width or the grid. A non-zero halt word (the apply's) leaves the target untouched.
//
// reward_norm_kernel, one workgroup of RN_THREADS ahead of the mixer tail: x = reward[:, :-1] of the batch, M = B T
// values gathered by episode id, unmasked (padded steps hold the storage's zeros and count; duplicate ids count twice).
//   bm = sum x / M;  bv = sum (x - bm)^2 / (M - 1)   (M = 1: 0)
//   delta = bm - mean;  tot = count + M
//   mean' = mean + delta M / tot;  var' = (var count + bv M + delta^2 count M / tot) / tot;  count' = tot
//   RS[t B + b] = (x - (float)mean') / sqrtf((float)var')
// Sums, bm, bv and the merge are fp64: thread j adds the elements i = j, j + RN_THREADS, .. (i = b T + t, so a wave
// reads runs of consecutive t) serially in ascending i, a butterfly over the wave's lanes and an ascending sum of the
// RN_THREADS / 64 wave totals follow: a fixed order, bitwise reproducible, and every partial sum is of at most M
// terms. Thread 0 merges into the three doubles of `st` ([mean, var, count], a float32 count would stop counting at
// 2^24) and rounds mean' and var' to fp32 once each; RS is then formed in fp32 (correctly rounded subtract, sqrt,
// divide). There is no LDS staging, so M is bounded by the RS workspace alone: up to RN_THREADS * RN_REG rewards a
// thread keeps its (at most RN_REG) elements in registers, every episode-id load and then every reward load of the
// workgroup in flight at once (two dependent round trips for the whole kernel: 8.6 us added to the mix phase at cfg2's
// M = 3840, where the first form, a loop of dependent loads per pass, added 11.0); past that it re-reads them from
// global memory in each of the three passes (M floats, L2-resident after the first). Both forms add the same elements
// in the same order. Nothing comes back to the host.
#pragma once
#include "learner_types.hpp"

namespace mq {

MQ_DEV float soft_elem(float t, float p, float omt, float tau) {
#pragma clang fp contract(off)
  const float a = t * omt;
  const float b = p * tau;
  return a + b;
}

__global__ __launch_bounds__(256) void soft_update_kernel(float* __restrict__ tg, const float* __restrict__ on,
                                                          int64_t n, float omt, float tau,
                                                          const int* __restrict__ halt) {
  if (halt && *halt != 0) return;
  const uintptr_t at = (uintptr_t)tg & 15;
  const bool same = ((uintptr_t)on & 15) == at;
  const int64_t lead = (int64_t)(((16 - at) >> 2) & 3);
  const int64_t head = same && lead < n ? lead : n;             // scalars before the float4 body
  const int64_t nv = (n - head) >> 2;                           // float4 items of the body
  const int64_t tail0 = head + 4 * nv, ns = head + (n - tail0); // scalar items: head, then tail
  const int64_t q0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  for (int64_t q = q0; q < nv; q += stride) {
    const int64_t i = head + 4 * q;
    const f32x4 t = *(const f32x4*)(tg + i), p = *(const f32x4*)(on + i);
    *(f32x4*)(tg + i) = f32x4{soft_elem(t.x, p.x, omt, tau), soft_elem(t.y, p.y, omt, tau),
                              soft_elem(t.z, p.z, omt, tau), soft_elem(t.w, p.w, omt, tau)};
  }
  for (int64_t j = q0; j < ns; j += stride) {
    const int64_t i = j < head ? j : tail0 + (j - head);
    tg[i] = soft_elem(tg[i], on[i], omt, tau);
  }
}

constexpr int RN_THREADS = 1024;
constexpr int RN_REG = 8;   // rewards a thread keeps in registers (M <= RN_THREADS * RN_REG = 8192: read once)

MQ_DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(RN_THREADS) void reward_norm_kernel(Dims d, Rep rp, double* __restrict__ st,
                                                                 float* __restrict__ RS) {
#pragma clang fp contract(off)
  __shared__ double part[RN_THREADS / 64];
  __shared__ float ms[2];
  const int tid = threadIdx.x, T = d.T, B = d.B, M = d.M;
  // element i = b T + t: its storage slot and its place in RS ([t][b], the mixer tail's row m)
  auto slot = [&](int i, int& m) {
    const int b = i / T, t = i - b * T;
    m = t * B + b;
    return rp.ep(b) * d.t_stride + t;
  };
  auto block_sum = [&](double v) {
    v = wave_sum_f64(v);
    __syncthreads();   // the readers of the sum before this one are done with `part`
    if ((tid & 63) == 0) part[tid >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < RN_THREADS / 64; ++k) s += part[k];
    return s;
  };
  // thread 0's statistics, in flight with the rewards (only it uses them)
  double mean = 0.0, var = 0.0, count = 0.0;
  if (tid == 0) { mean = st[0]; var = st[1]; count = st[2]; }
  const bool cached = M <= RN_THREADS * RN_REG;   // workgroup-uniform
  float xr[RN_REG];
  int mr[RN_REG];
  if (cached) {   // element u of this thread: i = tid + u RN_THREADS (clamped to M - 1 past the end, never used)
    // rp.ep(b) with its (workgroup-uniform) case taken once, outside the unrolled loops: inside them its branches
    // kept each element's id load and reward load from leaving before the previous element's had come back
    int br[RN_REG], tr[RN_REG];
    int64_t er[RN_REG];
#pragma unroll
    for (int u = 0; u < RN_REG; ++u) {
      const int i = min(tid + u * RN_THREADS, M - 1);
      br[u] = i / T;
      tr[u] = i - br[u] * T;
      mr[u] = tr[u] * B + br[u];
    }
    if (rp.nids) {
#pragma unroll
      for (int u = 0; u < RN_REG; ++u) er[u] = (int64_t)rp.ids[br[u]];
    } else if (rp.ep_ids) {
#pragma unroll
      for (int u = 0; u < RN_REG; ++u) er[u] = rp.ep_ids[br[u]];
    } else {
#pragma unroll
      for (int u = 0; u < RN_REG; ++u) er[u] = (int64_t)br[u];
    }
#pragma unroll
    for (int u = 0; u < RN_REG; ++u) xr[u] = rp.reward[er[u] * d.t_stride + tr[u]];
  }
  int m;
  double s = 0.0;
  if (cached) {
#pragma unroll
    for (int u = 0; u < RN_REG; ++u)
      if (tid + u * RN_THREADS < M) s += (double)xr[u];
  } else {
    for (int i = tid; i < M; i += RN_THREADS) s += (double)rp.reward[slot(i, m)];
  }
  const double bm = block_sum(s) / (double)M;
  double q = 0.0;
  if (cached) {
#pragma unroll
    for (int u = 0; u < RN_REG; ++u) {
      const double dv = (double)xr[u] - bm;
      if (tid + u * RN_THREADS < M) q += dv * dv;
    }
  } else {
    for (int i = tid; i < M; i += RN_THREADS) {
      const double dv = (double)rp.reward[slot(i, m)] - bm;
      q += dv * dv;
    }
  }
  const double ss = block_sum(q);
  if (tid == 0) {
    const double bv = M > 1 ? ss / (double)(M - 1) : 0.0;
    const double Md = (double)M;
    const double delta = bm - mean, tot = count + Md;
    const double mean1 = mean + delta * Md / tot;
    const double var1 = (var * count + bv * Md + delta * delta * count * Md / tot) / tot;
    st[0] = mean1;
    st[1] = var1;
    st[2] = tot;
    ms[0] = (float)mean1;
    ms[1] = (float)var1;
  }
  __syncthreads();
  const float mean32 = ms[0], sd = sqrtf(ms[1]);
  if (cached) {
#pragma unroll
    for (int u = 0; u < RN_REG; ++u)
      if (tid + u * RN_THREADS < M) RS[mr[u]] = (xr[u] - mean32) / sd;
  } else {
    for (int i = tid; i < M; i += RN_THREADS) {
      const float r = rp.reward[slot(i, m)];
      RS[m] = (r - mean32) / sd;
    }
  }
}

}  // namespace mq
