// TD(lambda) critic targets of the actor-critic and PPO learners (ma_set_td_lambda): the reference's
// build_td_lambda_targets (rl_utils.py:4-14) per agent, with the target critic's V' in the target Q's place. The
// return minus V is the GAE(lambda) advantage. a2c_lambda_kernel takes a2c_nstep_kernel's place in the step.
//
//   ret_T = V'_T (1 - sum_{t<T} term_t)
//   ret_t = (lg ret_{t+1}) + m_t (r_t + (og V'_{t+1}) (1 - term_t)),   t = T-1 .. 0,   lg = lambda gamma,
//                                                                      og = (1 - lambda) gamma
// every product and sum rounded to fp32 on its own in this order (torch's evaluation order of the reference's
// expression; td_lambda_kernel.hpp's, so tests/lambda_oracle.py serves both). ret[0..T) is stored.
//
// The n-step pass is parallel over (t0, agent) and gives an episode a workgroup. This return is a chain over t, so the
// only parallelism is across episodes and agents: one WAVE owns one episode and its lanes are the agents (n <= 64).
// A workgroup is `epw` waves (4; 2 or 1 where four episodes do not fit 64 KB: a2c_lambda_plan decides, not the kernel)
// and each wave works out of its own Tp (n + 3) floats of the dynamic LDS:
//   vt [Tp][n]  V' of the episode, staged with lane e -> (t, agent) = (e / n, e % n): n consecutive floats per t
//   rw [Tp]     r_t (RS != NULL: the standardised rewards [t][b], reward_norm_kernel's output), t < T
//   om [Tp]     1 - term_t, t < T
//   mk [Tp]     m_t = filled_t (1 - term_{t-1}), t < T
// While it stages, lane l counts term over its own t = l, l + 64, .. as integers; a butterfly adds the lanes' counts
// (integer sums: exact in any order, so 1 - sum term is the reference's float sum of zeros and ones bit for bit).
// After one barrier lane l < n runs agent l's scan T-1 .. 0 with the return in a register: rw / om / mk reads are
// LDS broadcasts (every lane the same word), V' reads are n consecutive words (no bank conflict), and ret is stored
// as rows [t][b n + agent]: n consecutive floats a step. No atomics, nothing depends on the launch's timing.
//
// Bounds, from the code: a wave returns nowhere before the barrier, but touches memory only under wv < epw and b < B;
// staging indexes e < Tp n and t < T; the scan runs under lane < n over t < T and reads V'[t + 1], t + 1 <= T < Tp.
// LDS: wave wv's region is [wv Tp (n + 3), (wv + 1) Tp (n + 3)) floats of the epw Tp (n + 3) the launch asked for.
#pragma once
#include "a2c_kernels.hpp"

namespace mq {

__global__ __launch_bounds__(256) void a2c_lambda_kernel(ADims d, Rep rp, const float* __restrict__ Vt,
                                                         const float* __restrict__ RS, float lg, float og, int epw,
                                                         float* __restrict__ ret) {
  // plain operators with contraction off, for a2c_nstep_kernel's reason: every product and sum is rounded on its own
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float a2c_lam_sm[];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = d.n, Tp = d.Tp, T = d.T;
  const int b = blockIdx.x * epw + wv;
  const bool live = wv < epw && b < d.B;
  float* vt = a2c_lam_sm + (size_t)wv * Tp * (n + 3);   // [Tp][n]
  float* rw = vt + Tp * n;                               // [Tp]
  float* om = rw + Tp;                                   // [Tp]
  float* mk = om + Tp;                                   // [Tp]
  int cnt = 0;
  if (live) {
    const int64_t e0 = rp.ep(b) * d.t_stride;
    const float* vsrc = Vt + (int64_t)b * n;
    for (int e = lane; e < Tp * n; e += 64) {
      const int t = (int)fdiv((uint32_t)e, d.dN), ag = e - t * n;
      vt[e] = vsrc[(int64_t)t * d.R + ag];
    }
    for (int t = lane; t < T; t += 64) {
      const int tm = (int)rp.term[e0 + t];
      cnt += tm;
      rw[t] = RS ? RS[(int64_t)t * d.B + b] : rp.reward[e0 + t];
      om[t] = 1.0f - (float)tm;
      mk[t] = coma_mask(rp, e0 + t, t);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  }
  __syncthreads();
  if (!live || lane >= n) return;
  const float* v = vt + lane;
  float acc = v[T * n] * (1.0f - (float)cnt);
  float* out = ret + (int64_t)b * n + lane;
#pragma unroll 4
  for (int t = T - 1; t >= 0; --t) {
    const float boot = (og * v[(t + 1) * n]) * om[t];
    const float inner = rw[t] + boot;
    const float carry = lg * acc;
    acc = carry + mk[t] * inner;
    out[(int64_t)t * d.R] = acc;
  }
}

}  // namespace mq
