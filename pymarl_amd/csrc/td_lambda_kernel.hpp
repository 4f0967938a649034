// TD(lambda) targets for the QMIX / VDN / IQL learner (mq_config.td_lambda): build_td_lambda_targets
// (rl_utils.py:4-14) applied as COMALearner applies it, to the target network's mixed values and the learner's own
// mask (q_learner.py:42-43). The reference's Q learner has the one-step target only; coma_td_kernel
// (coma_kernels.hpp) is the same recurrence on the COMA critic.
//
// The mixer tail is parallel over (t, b); a lambda-return is a backward recurrence over t inside an episode. So the
// tail runs as three launches: mix_*<MIX_LAMBDA_TARGETS> stores y'[t][b] (the target net's value at step t + 1),
// this kernel turns it into G[t][b], and mix_*<MIX_LAMBDA_LOSS> takes target = G[m] (mix_kernels.hpp).
//
// One workgroup per episode b. Every thread stages the episode's y', reward, 1 - terminated and mask for t < L into
// LDS; after one barrier lane j < k runs the recurrence of value j out of LDS (k = 1 with a mixer, k = n agents
// without one):
//   ret_L = y'_{L-1} (1 - sum_{t<L} term_t)
//   ret_t = (lg ret_{t+1}) + mask_t (r_t + (og y'_t) (1 - term_t)),   lg = lambda gamma, og = (1 - lambda) gamma
// every product and sum rounded separately to f32 in this order (torch's evaluation order; contraction is switched
// off for the kernel), so the output equals the reference function's bitwise. Padded steps are part of the
// recurrence as in the reference: their y' comes from fully masked rows and mask = 0 removes it.
// LDS: L (k + 3) floats, at most 64 KB (mq_create refuses a max_seq past it). The chain is L dependent steps
// (L <= 180 in the shipped configs) on B workgroups: a few microseconds, no parallel scan needed.
#pragma once
#include "learner_types.hpp"

namespace mq {

inline size_t td_lambda_lds_bytes(int L, int k) { return (size_t)L * (k + 3) * sizeof(float); }

__global__ __launch_bounds__(256) void td_lambda_kernel(Dims d, Rep rp, const float* __restrict__ YT,
                                                        float* __restrict__ G, int k, float lg, float og) {
  // No FMA contraction in this kernel. The arithmetic is written with plain * and + under this pragma, not with
  // __fmul_rn / __fadd_rn: HIP defines those as inline * and + compiled under the default -ffp-contract=fast, and the
  // backend fuses them once inlined (v_fma / v_fmac in the recurrence, 1 ulp off the reference).
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lam_sm[];
  const int b = blockIdx.x, L = d.T, B = d.B;
  float* yq = lam_sm;        // [L][k]
  float* rw = yq + L * k;    // [L]
  float* om = rw + L;        // [L] 1 - terminated
  float* mk = om + L;        // [L] mask
  const int64_t e0 = rp.ep(b) * d.t_stride;
  for (int e = threadIdx.x; e < L * k; e += 256) {
    const int t = e / k, j = e - t * k;
    yq[e] = YT[((int64_t)t * B + b) * k + j];
  }
  for (int t = threadIdx.x; t < L; t += 256) {
    rw[t] = rp.reward[e0 + t];
    om[t] = 1.0f - (float)rp.term[e0 + t];
    float m = (float)rp.filled[e0 + t];
    if (t > 0) m *= 1.0f - (float)rp.term[e0 + t - 1];   // q_learner.py:42-43
    mk[t] = m;
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j >= k) return;
  float tsum = 0.0f;
  for (int t = 0; t < L; ++t) tsum += 1.0f - om[t];
  float ret = yq[(L - 1) * k + j] * (1.0f - tsum);
  float* out = G + (int64_t)b * k + j;
  for (int t = L - 1; t >= 0; --t) {
    const float boot = (og * yq[t * k + j]) * om[t];
    const float inner = rw[t] + boot;
    const float carry = lg * ret;
    ret = carry + mk[t] * inner;
    out[(int64_t)t * B * k] = ret;
  }
}

// The same scan over standardised rewards (mq_set_reward_norm): r_t is RS[t][b], what reward_norm_kernel
// (epymarl_kernels.hpp) wrote, not the storage's reward; everything else is td_lambda_kernel's, line for line. It is a
// kernel of its own, not a shared inlined body: with the body shared, td_lambda_kernel's instruction schedule changed,
// and the default path's device code is held identical from commit to commit (scripts/compare_device_code.py).
__global__ __launch_bounds__(256) void td_lambda_rs_kernel(Dims d, Rep rp, const float* __restrict__ YT,
                                                           float* __restrict__ G, int k, float lg, float og,
                                                           const float* __restrict__ RS) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) float lam_sm[];
  const int b = blockIdx.x, L = d.T, B = d.B;
  float* yq = lam_sm;        // [L][k]
  float* rw = yq + L * k;    // [L]
  float* om = rw + L;        // [L] 1 - terminated
  float* mk = om + L;        // [L] mask
  const int64_t e0 = rp.ep(b) * d.t_stride;
  for (int e = threadIdx.x; e < L * k; e += 256) {
    const int t = e / k, j = e - t * k;
    yq[e] = YT[((int64_t)t * B + b) * k + j];
  }
  for (int t = threadIdx.x; t < L; t += 256) {
    rw[t] = RS[(int64_t)t * B + b];
    om[t] = 1.0f - (float)rp.term[e0 + t];
    float m = (float)rp.filled[e0 + t];
    if (t > 0) m *= 1.0f - (float)rp.term[e0 + t - 1];   // q_learner.py:42-43
    mk[t] = m;
  }
  __syncthreads();
  const int j = threadIdx.x;
  if (j >= k) return;
  float tsum = 0.0f;
  for (int t = 0; t < L; ++t) tsum += 1.0f - om[t];
  float ret = yq[(L - 1) * k + j] * (1.0f - tsum);
  float* out = G + (int64_t)b * k + j;
  for (int t = L - 1; t >= 0; --t) {
    const float boot = (og * yq[t * k + j]) * om[t];
    const float inner = rw[t] + boot;
    const float carry = lg * ret;
    ret = carry + mk[t] * inner;
    out[(int64_t)t * B * k] = ret;
  }
}

}  // namespace mq
