// The optimisers' host side: Adam's argument checks and per-step scalars (apply_adam_kernel), and the grid of the
// float4 element-wise kernels (apply_adam_kernel, soft_update_kernel), and the launcher of the two-pass slab reduction
// for the learners whose norm_part has a fixed size (launch_reduce).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "host_util.hpp"
#include "optim_kernels.hpp"
#include "reduce_plan.hpp"

namespace {

int check_adam(const char* who, float beta1, float beta2, float eps, float wd) {
  if (!(beta1 >= 0.0f && beta1 < 1.0f) || !(beta2 >= 0.0f && beta2 < 1.0f))
    return set_err(MQ_ERR_ARG, std::string(who) + ": adam betas must be in [0, 1)");
  if (!(eps > 0.0f)) return set_err(MQ_ERR_ARG, std::string(who) + ": adam eps must be > 0");
  if (!(wd >= 0.0f)) return set_err(MQ_ERR_ARG, std::string(who) + ": weight_decay must be >= 0");
  return MQ_OK;
}

// The kernel's scalars for step t (1-based): the bias corrections in double, as torch forms them in Python floats,
// each cast to float once.
// The double a float hyper-parameter stands for: the shortest decimal that rounds to it (0.999f is 0.999, as numpy
// prints a float32), which is the Python float the host's config held. The plain widening of 0.999f is off by 1.3e-8,
// and that is 1.3e-5 of 1 - beta2: more than the whole error budget of exp_avg_sq.
double decimal_of(float x) {
  char buf[40];
  for (int prec = 1; prec <= 9; ++prec) {
    std::snprintf(buf, sizeof(buf), "%.*g", prec, (double)x);
    if (std::strtof(buf, nullptr) == x) return std::strtod(buf, nullptr);
  }
  return (double)x;
}

AdamHP make_adam_hp(float lr, float beta1, float beta2, float eps, float wd, int64_t t, float clip, int n_agents) {
  const double b1 = decimal_of(beta1), b2 = decimal_of(beta2);
  const double bc1 = 1.0 - std::pow(b1, (double)t), bc2 = 1.0 - std::pow(b2, (double)t);
  AdamHP hp;
  hp.step_size = (float)(decimal_of(lr) / bc1);
  hp.bc2_sqrt = (float)std::sqrt(bc2);
  hp.beta2 = beta2;
  hp.omb1 = (float)(1.0 - b1);
  hp.omb2 = (float)(1.0 - b2);
  hp.eps = eps;
  hp.wd = wd;
  hp.clip = clip;
  hp.n_agents = n_agents;
  return hp;
}

// The grid of apply_adam_kernel and soft_update_kernel over n floats at the given pointers: a thread per float4 of the
// body (or per scalar when the pointers disagree modulo 16 bytes), at most 1024 blocks of 256
int vec4_blocks(std::initializer_list<const float*> ptrs, int64_t n) {
  bool same = true;
  for (const float* p : ptrs) same = same && ((uintptr_t)p & 15) == ((uintptr_t)*ptrs.begin() & 15);
  const int64_t items = same ? n / 4 + 6 : n;
  return (int)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 1024));
}

// The two-pass reduction of rb's regions (red_pass1_kernel, red_pass2_kernel) for `who` ("agent" / "critic"), checked
// against the region table and the norm-partial cap before the first launch; *nnorm = the partials left in norm_part.
int launch_reduce(const RedBuilder& rb, float* norm_part, const char* who, hipStream_t s, int* nnorm) {
  if (!rb.ok) return set_err(MQ_ERR_STATE, std::string(who) + ": more reduction regions than the plan holds");
  if (rb.b2 > kNormPartMax) return set_err(MQ_ERR_ARG, std::string(who) + " too large for the norm partial buffer");
  hipLaunchKernelGGL(red_pass1_kernel, dim3(rb.b1), dim3(256), 0, s, rb.pl);
  MQ_HIP(hipGetLastError());
  hipLaunchKernelGGL(red_pass2_kernel, dim3(rb.b2), dim3(256), 0, s, rb.pl, norm_part);
  MQ_HIP(hipGetLastError());
  *nnorm = rb.b2;
  return MQ_OK;
}

}  // namespace
