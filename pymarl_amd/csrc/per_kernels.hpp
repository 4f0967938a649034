// Prioritized episode replay (PER) for the QMIX / VDN / IQL learner, an opt-in the reference lacks: episodes are drawn
// in proportion to (TD error)^alpha, the loss carries importance weights, and every step writes the new TD errors back
// into the priorities. Priorities are produced on the device each step and consumed by the next draw, so the sampler
// and the write-back are kernels: no id, weight or priority is ever read by the host.
//
// per_sample_kernel, one workgroup of PER_THREADS: stratified draw of B episodes from the N live slots.
//   q_i = p_i^alpha (alpha == 1: p_i, no powf), cum = inclusive scan of q, total = cum[N-1]
//   seg = total / (float)B, tau_b = ((float)b + u[b]) * seg
//   id_b = min(N-1, #{i < N : cum[i] <= tau_b})        (the first i with cum[i] > tau_b)
//   w_b  = (N q_{id_b} / total)^(-beta) / max_b(...)   (beta == 0: exactly 1, no powf)
// Thread j sums the contiguous chunk [j C, (j+1) C) of q serially in ascending order, C = per_chunk(N) =
// ceil(N / PER_THREADS); a Hillis-Steele scan in LDS (PER_SCAN_DEPTH = log2 PER_THREADS steps) makes the inclusive
// thread totals. A draw binary-searches the thread totals for the first one above tau, then walks that thread's chunk
// from the total before it. Contraction is off: every sum is one rounded f32 addition.
//   The longest addition chain behind any cum[i]: D = per_chain_len(N) = 2 C + PER_SCAN_DEPTH
//   (C - 1 additions of the chunk sums, PER_SCAN_DEPTH of the scan, up to C of the walk), so every cum the kernel
//   compares against is within D 2^-24 total of the exact prefix sum. Where all sums are exact in f32 the ids are the
//   exact ones, whatever the order.
// The walk of a chunk starts from the scanned total before it, not from the thread's own chunk sum, so its last value
// may round below the scanned total the search compared against: a draw that then finds no element above tau takes the
// chunk's last one (inside the same error band). Slots >= N are never read.
//
// per_priority_kernel, one wave per batch row b, after the mixer tail stored TDA[t][b] = |td m| (mix_kernels.hpp):
//   a_b = sum_t TDA[t][b] (ascending t, serial), c_b = sum_t m[t][b] (x n_agents without a mixer)
//   p_b = a_b / max(c_b, 1) + eps;  prio[id_b] = p_b;  prio_max = max(prio_max, p_b)
// with the mask rebuilt from filled / terminated as td_lambda_kernel does. The maximum is an integer atomic max on
// the bit pattern: the values are positive floats, whose order is their bit patterns' order, so the result does not
// depend on the order of the rows. Duplicate ids write the same value.
#pragma once
#include "learner_types.hpp"

namespace mq {

constexpr int PER_THREADS = 1024;
constexpr int PER_SCAN_DEPTH = 10;   // log2(PER_THREADS)
constexpr int PER_NMAX = 32768;      // live episodes one draw supports (a chunk of 32 per thread)
constexpr int PER_LD = 8;            // independent loads per round trip of a chunk
inline int per_chunk(int n) { return (n + PER_THREADS - 1) / PER_THREADS; }
inline int per_chain_len(int n) { return 2 * per_chunk(n) + PER_SCAN_DEPTH; }

MQ_DEV float per_q(float p, float alpha) { return alpha == 1.0f ? p : powf(p, alpha); }

MQ_DEV float per_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(PER_THREADS) void per_sample_kernel(const float* __restrict__ prio, int N,
                                                                 const float* __restrict__ u, int B, float alpha,
                                                                 float beta, int64_t* __restrict__ ids,
                                                                 float* __restrict__ weights) {
#pragma clang fp contract(off)
  __shared__ float sc[2][PER_THREADS];
  __shared__ float wmx[PER_THREADS / 64];
  const int tid = threadIdx.x;
  const int C = (N + PER_THREADS - 1) / PER_THREADS;
  {
    const int i0 = min(tid * C, N), i1 = min(i0 + C, N);
    float tot = 0.0f;
    for (int i = i0; i < i1; i += PER_LD) {
      float v[PER_LD];
#pragma unroll
      for (int k = 0; k < PER_LD; ++k) v[k] = prio[min(i + k, i1 - 1)];
#pragma unroll
      for (int k = 0; k < PER_LD; ++k)
        if (i + k < i1) tot += per_q(v[k], alpha);
    }
    sc[0][tid] = tot;
  }
  __syncthreads();
  int cur = 0;
  for (int off = 1; off < PER_THREADS; off <<= 1) {
    float v = sc[cur][tid];
    if (tid >= off) v += sc[cur][tid - off];
    sc[cur ^ 1][tid] = v;
    __syncthreads();
    cur ^= 1;
  }
  const float* incl = sc[cur];
  const float total = incl[PER_THREADS - 1];
  const float seg = total / (float)B;
  const int jl = (N - 1) / C;   // the last thread with a live element
  float wmax = 0.0f, w0 = 0.0f;   // w0: the weight of this thread's first draw (the only one when B <= PER_THREADS)
  for (int b = tid; b < B; b += PER_THREADS) {
    const float tau = ((float)b + u[b]) * seg;
    int lo = 0, hi = jl;   // the first thread total above tau (the last live thread when none is)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (incl[mid] <= tau) lo = mid + 1;
      else hi = mid;
    }
    const int j = lo;
    const int i0 = j * C, i1 = min(i0 + C, N);
    float run = j > 0 ? incl[j - 1] : 0.0f;
    int id = i1 - 1;
    float qid = 0.0f;
    bool found = false;
    for (int i = i0; i < i1 && !found; i += PER_LD) {
      float v[PER_LD];
#pragma unroll
      for (int k = 0; k < PER_LD; ++k) v[k] = prio[min(i + k, i1 - 1)];
#pragma unroll
      for (int k = 0; k < PER_LD; ++k) {
        if (!found && i + k < i1) {
          const float q = per_q(v[k], alpha);
          run += q;
          qid = q;   // the chunk's last element when no cum passes tau
          if (run > tau) { found = true; id = i + k; }
        }
      }
    }
    float wt = 1.0f;
    if (beta != 0.0f) wt = powf(((float)N * qid) / total, -beta);
    ids[b] = (int64_t)id;
    if (b == tid) w0 = wt;
    else weights[b] = wt;
    wmax = fmaxf(wmax, wt);
  }
  wmax = per_wave_max(wmax);
  if ((tid & 63) == 0) wmx[tid >> 6] = wmax;
  __syncthreads();
  wmax = wmx[0];
#pragma unroll
  for (int k = 1; k < PER_THREADS / 64; ++k) wmax = fmaxf(wmax, wmx[k]);
  if (tid < B) weights[tid] = w0 / wmax;
  for (int b = tid + PER_THREADS; b < B; b += PER_THREADS) weights[b] = weights[b] / wmax;   // this thread's stores
}

// TDA: [T][B] |td m| of the step's mixer tail; the batch's episode ids (rp.ep) are the priorities' slots.
// One wave per batch row, 4 rows per workgroup. Lane l loads the row's values of t = t0 + 64 k + l, k < PRI_K: the
// replay's filled / terminated words coalesced over t, every load of a pass in flight at once (T = 120: one round
// trip). The sum of |td m| is then taken serially in ascending t by every lane alike, one v_readlane and one add per
// t (lanes past T hold +0, and a + 0 is a), so it is the same rounded chain as one lane walking t; the mask count is
// a sum of 0 / 1 values, exact in any order, taken as a wave reduction. (A first form with one lane per row, its loads
// coalesced over b, walked T in 15 dependent round trips and measured 15.0 us at T = 120, B = 32.)
constexpr int PRI_K = 4;
__global__ __launch_bounds__(256) void per_priority_kernel(Dims d, Rep rp, const float* __restrict__ TDA,
                                                           float* __restrict__ prio, float* __restrict__ prio_max,
                                                           int64_t n_prio, float eps) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);   // wave-uniform
  if (b >= d.B) return;
  const int T = d.T, B = d.B;
  const int64_t ep = rp.ep(b);
  if (ep < 0 || ep >= n_prio) return;   // never an id the sampler wrote; keeps a caller's bad id inside prio
  const int64_t e0 = ep * d.t_stride;
  float a = 0.0f, cs = 0.0f;
  for (int t0 = 0; t0 < T; t0 += 64 * PRI_K) {
    float av[PRI_K];
#pragma unroll
    for (int k = 0; k < PRI_K; ++k) {
      const int t = t0 + 64 * k + lane;
      const bool ok = t < T;
      const int tt = min(t, T - 1);
      const float v = TDA[(int64_t)tt * B + b];
      const float f = (float)rp.filled[e0 + tt];
      const float tp = tt > 0 ? (float)rp.term[e0 + tt - 1] : 0.0f;   // q_learner.py:42-43
      av[k] = ok ? v : 0.0f;
      cs += ok ? f * (1.0f - tp) : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < PRI_K; ++k) {
      if (t0 + 64 * k < T) {   // wave-uniform
#pragma unroll
        for (int j = 0; j < 64; ++j)
          a += __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, av[k]), j));
      }
    }
  }
  float c = wave_sum(cs);
  if (d.mixer == MQ_MIXER_NONE) c *= (float)d.n;
  const float p = a / fmaxf(c, 1.0f) + eps;
  if (lane == 0) {
    prio[ep] = p;
    atomicMax((int*)prio_max, __float_as_int(p));
  }
}

}  // namespace mq
