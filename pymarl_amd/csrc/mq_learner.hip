// libmq_learner: MI355X-native QMIX/VDN learner step behind the C ABI of include/mq_learner.h.
//
// One train step (QLearner.train, q_learner.py:37-116) is this stream-ordered launch sequence:
//   fc1      gemm  X1 = relu(W1 [obs | a_{t-1} | id] + b1)               both nets, rows gathered by episode id
//   gi       gemm  GI = W_ih X1 + b_ih                                    both nets
//   gru_fwd  recur h_t = GRU(GI_t, h_{t-1})                              both nets, serial over T
//   fc2      gemm  Q = W2 H + b2                                          both nets
//   hyper    gemm  QMIX hypernet outputs of state[:, :-1] / state[:, 1:] both nets (QMIX only)
//            (two-layer hypernet, mq_config.hypernet_layers = 2: layer 1 and layer 2 as two launches here, layer 2's
//            backward and the hypernet's weight gradients as two more in `dwh`, hyper2_kernels.hpp)
//   mix      per (t, episode): chosen gather, double-Q select, mixer fwd, TD, masked L2 sums, mixer bwd
//            (TD(lambda) targets, mq_config.td_lambda > 0: three launches, td_lambda_kernel.hpp)
//            (prioritized replay, mq_set_per: the loss-bearing pass in its PER form, then per_priority_kernel;
//            mq_per_sample draws the next batch, per_kernels.hpp)
//   gru_bwd  recur BPTT; dW_hh, dW_ih, dW2 and biases accumulated in-kernel, dGI written out
//   dx1      gemm  dP1 = (dGI W_ih) * [X1 > 0]
//   dw1      gemm  [dW1 | db1] = dP1^T xin                                split-K
//   dwh      gemm  [dW_hyper | db_hyper] = dHYP^T state                   split-K (QMIX only)
//   reduce   deterministic two-pass slab sums -> flat gradient buffer (+ loss sums), per-block sums of squares
//   --- (data-parallel all-reduce of the gradient buffer happens here, in the caller)
//   apply    / sum(mask), clip_grad_norm_, RMSprop (mq_set_adam: Adam, apply_adam_kernel)
// The feed-forward agent (mq_config.agent = MQ_AGENT_FFN, ffn_kernels.hpp) has no recurrence: fc1 / rnn / fc2 are three
// GEMMs forward (gi and gru_fwd are absent), and gru_bwd's place is taken by ffn_dp2_kernel (dP2 and the fc2 gradients),
// dx1 by the dP1 GEMM, dw1 by [dW_rnn | db_rnn] and dW1; everything from `hyper` to `apply` is untouched.
//            (soft target updates, mq_set_soft_target: soft_update_kernel as the step's last launch)
// Reward standardisation (mq_set_reward_norm): reward_norm_kernel ahead of `mix`, whose one-step pass and TD(lambda)
// scan then read its output in place of the storage's rewards (epymarl_kernels.hpp).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include <rccl/rccl.h>
#include "learner_gemms.hpp"
#include "gru_kernels.hpp"
#include "gru_fwd_fused.hpp"
#include "gru_fwd_pair.hpp"
#include "gru_bwd_fused.hpp"
#include "gru_tiles.hpp"
#include "mix_kernels.hpp"
#include "td_lambda_kernel.hpp"
#include "per_kernels.hpp"
#include "epymarl_kernels.hpp"
#include "hyper_kernel.hpp"
#include "hyper2_kernels.hpp"
#include "ffn_kernels.hpp"
#include "dwh_kernel.hpp"
#include "optim_kernels.hpp"
#include "module_fwd.hpp"
#include "switches.hpp"
#include "step_plan.hpp"

using namespace mq;

namespace {

std::mutex g_err_mu;
std::string g_err;

int set_err(int code, const std::string& msg) {
  std::lock_guard<std::mutex> lk(g_err_mu);
  g_err = msg;
  return code;
}

// A kernel's static LDS plus a launch's dynamic LDS against the CU's LDS (160 KB on gfx950), checked before the
// launch (the static size is looked up once per kernel). A dispatch past it aborts the whole queue
// (HSA_STATUS_ERROR_INVALID_ALLOCATION), which HIP then reports at the next runtime call as "an illegal memory access
// was encountered", far from its cause: the round-5 fault of a stamped BPTT build was exactly that.
int lds_fits(const void* fn, size_t dyn, const char* what) {
  static std::mutex mu;
  static std::vector<std::pair<const void*, size_t>> known;
  static int limit = 0;
  size_t st = 0;
  bool found = false;
  {
    std::lock_guard<std::mutex> lk(mu);
    for (const auto& k : known)
      if (k.first == fn) { st = k.second; found = true; break; }
  }
  if (!found) {
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, fn) != hipSuccess) return set_err(MQ_ERR_HIP, std::string(what) + ": hipFuncGetAttributes");
    st = fa.sharedSizeBytes;
    std::lock_guard<std::mutex> lk(mu);
    known.emplace_back(fn, st);
    if (limit == 0) {
      int dev = 0, v = 0;
      limit = (hipGetDevice(&dev) == hipSuccess &&
               hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, dev) == hipSuccess && v > 0)
                  ? v : 160 * 1024;
    }
  }
  if (st + dyn > (size_t)limit)
    return set_err(MQ_ERR_ARG, std::string(what) + " needs " + std::to_string(st) + " B of static + " +
                                   std::to_string(dyn) + " B of dynamic LDS, past the " + std::to_string(limit) +
                                   " B a workgroup can have");
  return MQ_OK;
}
#define MQ_LDS(fn, dyn)                                                        \
  do {                                                                         \
    const int _rc = lds_fits((const void*)(fn), (size_t)(dyn), #fn);          \
    if (_rc) return _rc;                                                       \
  } while (0)

#define MQ_HIP(expr)                                                                        \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return set_err(MQ_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));        \
  } while (0)

constexpr size_t kLambdaLdsMax = 64 * 1024;   // dynamic LDS of td_lambda_kernel (checked in mq_create)
enum Phase { PH_FC1, PH_GI, PH_GRUF, PH_FC2, PH_HYP, PH_MIX, PH_GRUB, PH_DX1, PH_DW1, PH_DWH, PH_RED, PH_APPLY,
             PH_N };
const char* kPhaseNames = "fc1;gi;gru_fwd;fc2;hyper;mix;gru_bwd;dx1;dw1;dwh;reduce;apply";

}  // namespace

struct mq_handle {
  mq_config cfg;
  int I, E, NH;
  int64_t off[MQ_P_COUNT + 1];
  int64_t P;
  int64_t len_rnn, len_mix;
  int64_t pitch_rnn;   // the fused BPTT's slab pitch: len_rnn rounded up to 4 floats (16-byte slab rows)
  // bound (caller-owned)
  float *on = nullptr, *tg = nullptr, *grad = nullptr, *sq = nullptr, *stats = nullptr;
  int32_t* curmax_user = nullptr;
  // workspace (handle-owned)
  void* ws = nullptr;
  Work w;
  int32_t* curmax_ws = nullptr;
  // last step bookkeeping
  bool have_fb = false;
  Dims last;
  mq_plan plan{};
  int n_norm_part = 0;
  PlanOverrides ov;   // MQ_PLAN, read once in mq_create (step_plan.hpp)
  bool dp = false;   // gradient buffer is summed across ranks between mq_forward_backward and mq_apply
  ncclComm_t comm = nullptr;   // mq_comm_attach / mq_comm_use: the library all-reduces the grad buffer itself
  int comm_world = 0;
  bool comm_owned = false;     // mq_comm_attach created it (freed on detach); mq_comm_use borrows the caller's
  hipStream_t side = nullptr;   // COMA: the actor's side stream (coma_host.hpp)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // the TD(lambda) passes' workspace, allocated only for a handle that runs them: y' and the lambda targets,
  // [max_seq * max_batch] (no mixer: x n_agents) floats each
  float *YT = nullptr, *G = nullptr;
  bool have_lambda = false;   // the last step ran them (mq_copy_intermediate 4 / 5)
  // prioritized replay (mq_set_per): armed for the next step only; TDA [max_seq * max_batch] is the tail's |td m|
  // record, allocated by the first mq_set_per
  mq_per per{};
  bool per_armed = false;
  float* TDA = nullptr;
  bool have_per = false;   // the last step was a PER step (mq_copy_intermediate 6)
  // the two-layer hypernet (cfg.hypernet_layers = 2): its layout, and the layer-1 tensors A1 [2][max M][N1] and dA1
  // [max M][N1], allocated only for such a handle
  bool hyper2 = false;
  Hyp2Lay y2{};
  float *A1 = nullptr, *dA1 = nullptr;
  bool have_h2 = false;   // the last step ran it (mq_copy_intermediate 7)
  int hyper_layers = 0;   // of the last step (mq_last_hyper_layers)
  bool ffn = false;       // cfg.agent = MQ_AGENT_FFN: the feed-forward agent
  int last_agent = 0;     // of the last step (mq_last_agent)
  // Adam (mq_set_adam): mq_apply launches apply_adam_kernel with ad.exp_avg beside sq; adam_step counts the steps applied
  bool adam = false;
  mq_adam ad{};
  int64_t adam_step = 0;
  // soft target updates (mq_set_soft_target): soft_update_kernel behind the apply, target = target omt + online tau
  bool soft = false;
  float soft_omt = 0.0f, soft_tau = 0.0f;
  int last_soft = -1;   // of the last mq_apply (mq_last_soft_target)
  // reward standardisation (mq_set_reward_norm): the caller's [mean, var, count] doubles, and RS [max_seq * max_batch],
  // the step's standardised rewards, allocated by the first mq_set_reward_norm
  double* rew_state = nullptr;
  float* RS = nullptr;
  bool have_rs = false;   // the last step standardised (mq_copy_intermediate 8, mq_last_reward_norm)
  int num_cu = 0;
  // timing: a ring of `slots` steps x PH_N (start, stop) event pairs; phases outside `mask` are not recorded
  int slots = 0;
  uint32_t mask = 0;
  int64_t tstep = 0;
  std::vector<hipEvent_t> ev0, ev1;
  std::vector<uint8_t> ev_used;
};

namespace {

void compute_layout(mq_handle* h) {
  const mq_config& c = h->cfg;
  const int Hd = mq::H, n = c.n_agents, A = c.n_actions, S = c.state_dim, E = h->E, I = h->I;
  int64_t sz[MQ_P_COUNT] = {};
  sz[MQ_P_FC1_W] = (int64_t)Hd * I; sz[MQ_P_FC1_B] = Hd;
  sz[MQ_P_RNN_W_IH] = 3LL * Hd * Hd; sz[MQ_P_RNN_W_HH] = 3LL * Hd * Hd;
  sz[MQ_P_RNN_B_IH] = 3 * Hd; sz[MQ_P_RNN_B_HH] = 3 * Hd;
  sz[MQ_P_FC2_W] = (int64_t)A * Hd; sz[MQ_P_FC2_B] = A;
  const bool ffn = c.agent == MQ_AGENT_FFN;
  if (ffn) {   // rnn is Linear(64, 64): the GRU's four tensors are empty
    sz[MQ_P_RNN_W_IH] = sz[MQ_P_RNN_W_HH] = sz[MQ_P_RNN_B_IH] = sz[MQ_P_RNN_B_HH] = 0;
    sz[MQ_P_FFN_W] = (int64_t)Hd * Hd; sz[MQ_P_FFN_B] = Hd;
  }
  // the buffer's order: the enum's, with the two-layer hypernet's second layers behind their first layers
  // (parameters() order of upstream's QMixer) and the feed-forward agent's rnn.weight / rnn.bias in the GRU tensors'
  // place; the entries a configuration lacks are empty and come last
  int order[MQ_P_COUNT];
  int no = 0;
  for (int i = 0; i <= MQ_P_V2_B; ++i) {
    if (ffn && i >= MQ_P_RNN_W_IH && i <= MQ_P_RNN_B_HH) continue;
    order[no++] = i;
    if (ffn && i == MQ_P_FC1_B) { order[no++] = MQ_P_FFN_W; order[no++] = MQ_P_FFN_B; }
    if (h->hyper2 && i == MQ_P_HW1_B) { order[no++] = MQ_P_HW1_W2; order[no++] = MQ_P_HW1_B2; }
    if (h->hyper2 && i == MQ_P_HWF_B) { order[no++] = MQ_P_HWF_W2; order[no++] = MQ_P_HWF_B2; }
  }
  if (!h->hyper2)
    for (int i = MQ_P_HW1_W2; i <= MQ_P_HWF_B2; ++i) order[no++] = i;
  if (ffn)
    for (int i = MQ_P_RNN_W_IH; i <= MQ_P_RNN_B_HH; ++i) order[no++] = i;
  else { order[no++] = MQ_P_FFN_W; order[no++] = MQ_P_FFN_B; }
  if (c.mixer == MQ_MIXER_QMIX) {
    sz[MQ_P_HW1_W] = (int64_t)E * n * S; sz[MQ_P_HW1_B] = (int64_t)E * n;
    sz[MQ_P_HWF_W] = (int64_t)E * S; sz[MQ_P_HWF_B] = E;
    if (h->hyper2) {
      const int64_t He = c.hypernet_embed;
      sz[MQ_P_HW1_W] = He * S; sz[MQ_P_HW1_B] = He;
      sz[MQ_P_HWF_W] = He * S; sz[MQ_P_HWF_B] = He;
      sz[MQ_P_HW1_W2] = (int64_t)E * n * He; sz[MQ_P_HW1_B2] = (int64_t)E * n;
      sz[MQ_P_HWF_W2] = (int64_t)E * He; sz[MQ_P_HWF_B2] = E;
    }
    sz[MQ_P_HB1_W] = (int64_t)E * S; sz[MQ_P_HB1_B] = E;
    sz[MQ_P_V0_W] = (int64_t)E * S; sz[MQ_P_V0_B] = E;
    sz[MQ_P_V2_W] = E; sz[MQ_P_V2_B] = 1;
  }
  int64_t o = 0;
  for (int i = 0; i < MQ_P_COUNT; ++i) { h->off[order[i]] = o; o += sz[order[i]]; }
  h->off[MQ_P_COUNT] = o;
  h->P = o;
  if (h->hyper2) {
    Hyp2Lay& y = h->y2;
    y.w1a = h->off[MQ_P_HW1_W]; y.b1a = h->off[MQ_P_HW1_B]; y.w12 = h->off[MQ_P_HW1_W2]; y.b12 = h->off[MQ_P_HW1_B2];
    y.wfa = h->off[MQ_P_HWF_W]; y.bfa = h->off[MQ_P_HWF_B]; y.wf2 = h->off[MQ_P_HWF_W2]; y.bf2 = h->off[MQ_P_HWF_B2];
    y.hbw = h->off[MQ_P_HB1_W]; y.hbb = h->off[MQ_P_HB1_B]; y.v0w = h->off[MQ_P_V0_W]; y.v0b = h->off[MQ_P_V0_B];
    y.He = c.hypernet_embed; y.E = E; y.nE = n * E; y.N1 = 2 * y.He + 2 * E;
  }
  // the BPTT's slab: [w_ih | w_hh | b_ih | b_hh | fc2.w | fc2.b]; feed-forward agent: [rnn.w | rnn.b | fc2.w | fc2.b]
  h->len_rnn = h->off[MQ_P_FC2_B] + A - h->off[ffn ? MQ_P_FFN_W : MQ_P_RNN_W_IH];
  h->pitch_rnn = (h->len_rnn + 3) & ~int64_t(3);
  h->len_mix = h->off[MQ_P_V2_W] - h->off[MQ_P_HW1_W];
}

int64_t align_up(int64_t x) { return (x + 63) & ~int64_t(63); }

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

// apply_adam_kernel's grid: a thread per float4 of the body (or per scalar when the pointers disagree modulo 16 bytes),
// at most 1024 blocks of 256
int adam_blocks(const float* p, const float* g, const float* m, const float* v, int64_t n) {
  const uintptr_t a = (uintptr_t)p & 15;
  const bool same = ((uintptr_t)g & 15) == a && ((uintptr_t)m & 15) == a && ((uintptr_t)v & 15) == a;
  const int64_t items = same ? n / 4 + 6 : n;
  return (int)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 1024));
}

// soft_update_kernel's grid, by the same rule
int soft_blocks(const float* tg, const float* on, int64_t n) {
  const bool same = ((uintptr_t)tg & 15) == ((uintptr_t)on & 15);
  const int64_t items = same ? n / 4 + 6 : n;
  return (int)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, 1024));
}

Dims make_dims(const mq_handle* h, const mq_replay* b) {
  return mq::make_dims(h->cfg, b->batch_size, b->t_len, b->t_stride);
}

Rep make_rep(const mq_replay* b) {
  Rep r;
  r.obs = b->obs; r.state = b->state; r.actions = b->actions; r.avail = b->avail_actions; r.reward = b->reward;
  r.term = b->terminated; r.filled = b->filled; r.ep_ids = b->ep_ids; r.avail_bits = b->avail_bits;
  r.nids = 0;
  if (b->ep_ids_host && b->batch_size <= MQ_INLINE_IDS) {   // ids in the kernel arguments (check_ids validated)
    r.nids = b->batch_size;
    for (int i = 0; i < b->batch_size; ++i) r.ids[i] = (int32_t)b->ep_ids_host[i];
  }
  return r;
}

Lay make_lay(const mq_handle* h) {
  Lay L;
  for (int i = 0; i < LAY_N; ++i) L.o[i] = h->off[i];
  L.o[LAY_N] = h->P;
  return L;
}

// The episodes a batch names lie inside its storage: host ids (the ones make_rep copies into the kernel arguments) in
// [0, n_episodes); a dense batch no longer than the storage. Device ids are not read on the host. Every entry point
// that hands a batch to make_rep calls this first (check_batch for the train steps, mq_mac_forward on its own).
int check_ids(const mq_replay* b) {
  if (b->ep_ids_host && b->batch_size <= MQ_INLINE_IDS) {
    for (int i = 0; i < b->batch_size; ++i)
      if (b->ep_ids_host[i] < 0 || b->ep_ids_host[i] >= b->n_episodes)
        return set_err(MQ_ERR_ARG, "episode id " + std::to_string(b->ep_ids_host[i]) + " outside [0, n_episodes)");
  } else if (!b->ep_ids && b->batch_size > b->n_episodes) {
    return set_err(MQ_ERR_ARG, "batch_size exceeds n_episodes with no episode ids");
  }
  return MQ_OK;
}

int check_batch(const mq_handle* h, const mq_replay* b) {
  if (!b) return set_err(MQ_ERR_ARG, "batch is NULL");
  if (!b->obs || !b->actions || !b->avail_actions || !b->reward || !b->terminated || !b->filled)
    return set_err(MQ_ERR_ARG, "batch is missing a required field pointer");
  if (h->cfg.mixer == MQ_MIXER_QMIX && !b->state) return set_err(MQ_ERR_ARG, "QMIX needs batch.state");
  if (b->batch_size < 1 || b->batch_size > h->cfg.max_batch)
    return set_err(MQ_ERR_ARG, "batch_size " + std::to_string(b->batch_size) + " outside [1, max_batch=" +
                                   std::to_string(h->cfg.max_batch) + "]");
  if (b->t_len < 2 || b->t_len > h->cfg.max_seq || b->t_len > b->t_stride)
    return set_err(MQ_ERR_ARG, "t_len " + std::to_string(b->t_len) + " must be in [2, min(max_seq, t_stride)]");
  if ((int64_t)b->t_len * b->batch_size * h->cfg.n_agents >= (1LL << 31))
    return set_err(MQ_ERR_ARG, "batch too large for 32-bit row indices");
  return check_ids(b);
}

struct PhaseTimer {
  mq_handle* h;
  hipStream_t s;
  int cur = -1;
  int idx(int p) const { return (int)(h->tstep % h->slots) * PH_N + p; }
  void begin(int p) {
    end();
    if (h->slots <= 0 || !((h->mask >> p) & 1u)) return;
    (void)hipEventRecord(h->ev0[idx(p)], s);
    h->ev_used[idx(p)] = 1;
    cur = p;
  }
  void end() {
    if (cur < 0) return;
    (void)hipEventRecord(h->ev1[idx(cur)], s);
    cur = -1;
  }
};

template <int RW>
hipError_t launch_gru_fwd(const Dims& d, const mq_handle* h, const Lay& L, const Work& w, hipStream_t s) {
  dim3 grid((d.R + RW - 1) / RW, 2);
  hipLaunchKernelGGL(gru_fwd_kernel<RW>, grid, dim3(256), 0, s, d, (const float*)h->on, (const float*)h->tg, L, w);
  return hipGetLastError();
}

template <int RW>
hipError_t launch_gru_bwd(const Dims& d, const Rep& rp, const mq_handle* h, const Lay& L, const Work& w,
                          hipStream_t s, int nblk, size_t dyn) {
  hipLaunchKernelGGL(gru_bwd_kernel<RW>, dim3(nblk), dim3(512), dyn, s, d, rp, (const float*)h->on, L, w,
                     h->len_rnn);
  return hipGetLastError();
}

// The mixer tail's kernel for plan `mix` (MQ_MIX_*) in pass MODE (mix_kernels.hpp: the one-step tail, or one of the two
// TD(lambda) passes around td_lambda_kernel).
template <int MODE>
void launch_mix(int mix, int nblk, const mq_handle* h, const Dims& d, const Rep& rp, const Lay& L, const Work& w,
                int32_t* curmax, hipStream_t s) {
  const dim3 grid(nblk), block(256);
  const float *P0 = h->on, *P1 = h->tg;
  if constexpr (MODE == MIX_ONE_STEP) {
    if (mix == MQ_MIX_FAST16)
      hipLaunchKernelGGL((mix_fast_kernel<16, 16>), grid, block, 0, s, d, rp, P0, P1, L, w, curmax);
    else if (mix == MQ_MIX_FAST32)
      hipLaunchKernelGGL((mix_fast_kernel<32, 16>), grid, block, 0, s, d, rp, P0, P1, L, w, curmax);
    else if (mix == MQ_MIX_STREAM)
      hipLaunchKernelGGL(mix_kernel<true>, grid, block, 0, s, d, rp, P0, P1, L, w, curmax);
    else
      hipLaunchKernelGGL(mix_kernel<false>, grid, block, 0, s, d, rp, P0, P1, L, w, curmax);
  } else {   // the lambda passes: y' out (YT) or the targets in (G) as two trailing arguments
    float* YT = h->YT;
    const float* G = h->G;
    if (mix == MQ_MIX_FAST16)
      hipLaunchKernelGGL((mix_fast_kernel<16, 16, MODE, float*, const float*>), grid, block, 0, s, d, rp, P0, P1, L,
                         w, curmax, YT, G);
    else if (mix == MQ_MIX_FAST32)
      hipLaunchKernelGGL((mix_fast_kernel<32, 16, MODE, float*, const float*>), grid, block, 0, s, d, rp, P0, P1, L,
                         w, curmax, YT, G);
    else if (mix == MQ_MIX_STREAM)
      hipLaunchKernelGGL((mix_kernel<true, MODE, float*, const float*>), grid, block, 0, s, d, rp, P0, P1, L, w,
                         curmax, YT, G);
    else
      hipLaunchKernelGGL((mix_kernel<false, MODE, float*, const float*>), grid, block, 0, s, d, rp, P0, P1, L, w,
                         curmax, YT, G);
  }
}

// The loss-bearing pass MODE (MIX_ONE_STEP or MIX_LAMBDA_LOSS) in its PER form: (W, TDA) trail the pass's arguments.
template <int MODE>
void launch_mix_per(int mix, int nblk, const mq_handle* h, const Dims& d, const Rep& rp, const Lay& L, const Work& w,
                    int32_t* curmax, hipStream_t s) {
  const dim3 grid(nblk), block(256);
  const float *P0 = h->on, *P1 = h->tg;
  const float* W = h->per.weights;
  float* TDA = h->TDA;
  constexpr int M = MODE | MIX_PER;
  if constexpr (MODE == MIX_ONE_STEP) {
    if (mix == MQ_MIX_FAST16)
      hipLaunchKernelGGL((mix_fast_kernel<16, 16, M, const float*, float*>), grid, block, 0, s, d, rp, P0, P1, L, w,
                         curmax, W, TDA);
    else if (mix == MQ_MIX_FAST32)
      hipLaunchKernelGGL((mix_fast_kernel<32, 16, M, const float*, float*>), grid, block, 0, s, d, rp, P0, P1, L, w,
                         curmax, W, TDA);
    else if (mix == MQ_MIX_STREAM)
      hipLaunchKernelGGL((mix_kernel<true, M, const float*, float*>), grid, block, 0, s, d, rp, P0, P1, L, w, curmax,
                         W, TDA);
    else
      hipLaunchKernelGGL((mix_kernel<false, M, const float*, float*>), grid, block, 0, s, d, rp, P0, P1, L, w, curmax,
                         W, TDA);
  } else {
    float* YT = h->YT;
    const float* G = h->G;
    if (mix == MQ_MIX_FAST16)
      hipLaunchKernelGGL((mix_fast_kernel<16, 16, M, float*, const float*, const float*, float*>), grid, block, 0, s,
                         d, rp, P0, P1, L, w, curmax, YT, G, W, TDA);
    else if (mix == MQ_MIX_FAST32)
      hipLaunchKernelGGL((mix_fast_kernel<32, 16, M, float*, const float*, const float*, float*>), grid, block, 0, s,
                         d, rp, P0, P1, L, w, curmax, YT, G, W, TDA);
    else if (mix == MQ_MIX_STREAM)
      hipLaunchKernelGGL((mix_kernel<true, M, float*, const float*, const float*, float*>), grid, block, 0, s, d, rp,
                         P0, P1, L, w, curmax, YT, G, W, TDA);
    else
      hipLaunchKernelGGL((mix_kernel<false, M, float*, const float*, const float*, float*>), grid, block, 0, s, d, rp,
                         P0, P1, L, w, curmax, YT, G, W, TDA);
  }
}

// The one-step pass reading the standardised rewards (MIX_RS; PER: its PER form too): RS leads the trailing arguments.
template <int FULL, typename... X>
void launch_mix_rs(int mix, int nblk, const mq_handle* h, const Dims& d, const Rep& rp, const Lay& L, const Work& w,
                   int32_t* curmax, hipStream_t s, X... x) {
  const dim3 grid(nblk), block(256);
  const float *P0 = h->on, *P1 = h->tg;
  const float* RS = h->RS;
  if (mix == MQ_MIX_FAST16)
    hipLaunchKernelGGL((mix_fast_kernel<16, 16, FULL, const float*, X...>), grid, block, 0, s, d, rp, P0, P1, L, w,
                       curmax, RS, x...);
  else if (mix == MQ_MIX_FAST32)
    hipLaunchKernelGGL((mix_fast_kernel<32, 16, FULL, const float*, X...>), grid, block, 0, s, d, rp, P0, P1, L, w,
                       curmax, RS, x...);
  else if (mix == MQ_MIX_STREAM)
    hipLaunchKernelGGL((mix_kernel<true, FULL, const float*, X...>), grid, block, 0, s, d, rp, P0, P1, L, w, curmax,
                       RS, x...);
  else
    hipLaunchKernelGGL((mix_kernel<false, FULL, const float*, X...>), grid, block, 0, s, d, rp, P0, P1, L, w, curmax,
                       RS, x...);
}

// Plan the slab reductions of one step: regions in gradient order, then the loss sums (not part of the norm).
struct RedBuilder {
  RedPlan pl{};
  int b1 = 0, b2 = 0;
  float* tmp;
  explicit RedBuilder(float* t) : tmp(t) {}
  // returns true when the region is summed by pass 2 straight from its slabs (no pass-1 blocks read them)
  bool add(const float* src, int nslab, int64_t len, float* dst, bool sq, int64_t pitch = 0, bool direct_ok = false,
           int perm = 0) {
    if (len <= 0 || nslab <= 0) return false;
    RedRegion& R = pl.r[pl.nr++];
    R.src = src; R.dst = dst; R.len = len; R.pitch = pitch > 0 ? pitch : len; R.nslab = nslab; R.sq = sq ? 1 : 0;
    R.perm = perm;
    if (direct_ok && nslab <= kRedZ) {   // pass 2 sums the slabs themselves: no pass-1 blocks, no tmp
      R.zc = 1; R.ng = nslab; R.tmp = (float*)src; R.tpitch = R.pitch; R.vec = 0; R.xcd = 0;
      R.blk1 = b1;
      R.blk2 = b2; b2 += (int)((len + 255) / 256);
      return true;
    }
    R.tpitch = len;
    // at most kRedZ groups, so pass 2 sums <= 16 partials per element with all loads in flight
    R.zc = (nslab + kRedZ - 1) / kRedZ;
    R.ng = (nslab + R.zc - 1) / R.zc;
    R.tmp = tmp;
    tmp += R.ng * len;
    R.vec = (len % 4 == 0 && R.pitch % 4 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)R.tmp & 15) == 0) ? 1 : 0;
    R.xcd = (nslab % 128 == 0 && R.ng == kRedZ && b1 % 16 == 0) ? 1 : 0;
    const int nb = (int)((len + 255) / 256), nb1 = R.vec ? (int)((len + 1023) / 1024) : nb;
    R.blk1 = b1; b1 += nb1 * R.ng;
    R.blk2 = b2; b2 += nb;
    return false;
  }
};

// Side stream and fork / join events (COMA's actor overlap), created on first use. Lowest stream priority: the
// work on the caller's stream keeps the arbiter's preference.
hipError_t ensure_side(mq_handle* h) {
  if (h->side) return hipSuccess;
  int least = 0, greatest = 0;
  hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
  if (e == hipSuccess) e = hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, least);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming);
  return e;
}

int device_cus(mq_handle* h) {
  if (h->num_cu == 0) {
    int dev = 0, ncu = 0;
    h->num_cu = (hipGetDevice(&dev) == hipSuccess &&
                 hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) ? ncu : -1;
  }
  return h->num_cu;
}

// The tile kernels' <KQ1> instantiations (gru_tiles.hpp tile_kq1), named once: f(std::integral_constant<int, KQ1>).
template <class F>
void dispatch_kq1(int kq1, F&& f) {
  if (kq1 == 8) f(std::integral_constant<int, 8>{});
  else if (kq1 == 20) f(std::integral_constant<int, 20>{});
  else if (kq1 == 40) f(std::integral_constant<int, 40>{});
  else if (kq1 == 72) f(std::integral_constant<int, 72>{});
  else f(std::integral_constant<int, 80>{});
}

// One train step's launches, phase by phase in stream order. Which kernels run is plan_step's answer `p`
// (step_plan.hpp), fixed before the first launch; nothing here decides.
struct Step {
  mq_handle* h;
  const Dims d;
  const Rep rp;
  const Lay L;
  Work w;
  int32_t* curmax;
  hipStream_t s;
  PhaseTimer pt;
  const bool rnorm = false;   // reward standardisation is set (mq_set_reward_norm)
  const int64_t RT = (int64_t)d.Tp * d.R;

  int forward(const StepPlan& p);
  int hypernet(const StepPlan& p);
  int mixer_tail(const StepPlan& p);
  int hypernet2_backward(const StepPlan& p);
  int bptt(const StepPlan& p);
  int reduce(const StepPlan& p);
  // feed-forward agent: slab_rnn holds the step's [dWr | dbr] split-K slabs, then ffn_dp2_kernel's [dW2 | db2] slabs
  static int64_t ffn_w2_slabs(const StepPlan& p) { return (int64_t)p.ffn_wr_ns * FfnDwrProb::LEN; }
};

int Step::forward(const StepPlan& p) {
  const float *P0 = h->on, *P1 = h->tg;
  if (p.ffn) {
    // the feed-forward agent: three row-parallel GEMMs, both nets each (ffn_kernels.hpp)
    pt.begin(PH_FC1);
    {
      Fc1Prob p1{d, rp, h->on, h->tg, h->off[MQ_P_FC1_W], h->off[MQ_P_FC1_B], w.X1, w.XIN, RT};
      MQ_HIP(launch_gemm(p1, (int)RT, 2 * mq::H, 1, s));
    }
    pt.begin(PH_GRUF);
    {
      FfnHidProb ph{w.X1, h->on, h->tg, h->off[MQ_P_FFN_W], h->off[MQ_P_FFN_B], w.Hs, RT};
      MQ_HIP(launch_gemm(ph, (int)RT, mq::H, 2, s));
    }
    pt.begin(PH_FC2);
    {
      Fc2Prob p2{w.Hs, h->on, h->tg, h->off[MQ_P_FC2_W], h->off[MQ_P_FC2_B], w.Q, RT, d.A};
      MQ_HIP(launch_gemm(p2, (int)RT, d.A, 2, s));
    }
    return MQ_OK;
  }
  if (p.fwd == FWD_TILES) {
    // row tiles of 32 (two M-tiles) per workgroup, both nets: the recurrence and fc1 / W_ih / fc2 on MFMA
    pt.begin(PH_GRUF);
    const dim3 grid(16 * (((d.R + TR_F - 1) / TR_F + 7) / 8));   // row tiles x 2 nets, XCD-paired (gru_tiles.hpp)
    dispatch_kq1(p.kq1, [&](auto K) {
      hipLaunchKernelGGL(gru_fwd_tile_kernel<decltype(K)::value>, grid, dim3(512), 0, s, d, rp, P0, P1, L, w);
    });
    MQ_HIP(hipGetLastError());
  } else if (p.fwd != FWD_UNFUSED) {
    // one row per workgroup: fc1 / W_ih / fc2 ride on the recurrence's idle matrix cores (gru_fwd_fused.hpp)
    pt.begin(PH_GRUF);
    if (p.hyp_place == HYP_FWD_GRID) {
      launch_fwd_fused_hyp(s, d, rp, P0, P1, L, w);
    } else if (p.fwd == FWD_PAIR) {
      std::string stamp_path;   // diagnostic (MQ_DIAG pair_stamp=<file>): step stamps of the first 8 workgroups
      const bool want_stamp = env_item("MQ_DIAG", "pair_stamp", &stamp_path) && !stamp_path.empty();
      const int hsched = env_int("MQ_DIAG", "hyp_sched", kHypSched, 16);   // tuning: the in-loop tile schedule
      const int pair_hyp = p.hyp_place == HYP_PAIR_WAVES ? 2 : p.hyp_place == HYP_PAIR_EPI ? 1 : 0;
      // the stamp build has the 5-slot gather only: shapes past it run unstamped (never a partial gather)
      const bool stamp = want_stamp && d.Tp <= 512 && FCH * d.O <= 256 * 5;
      launch_fwd_pair(s, d, rp, P0, P1, L, w, pair_hyp, stamp, hsched);
      if (stamp) {
        std::vector<uint32_t> st((size_t)8 * PST);
        MQ_HIP(hipMemcpyAsync(st.data(), w.slab_rnn, st.size() * 4, hipMemcpyDeviceToHost, s));
        MQ_HIP(hipStreamSynchronize(s));
        if (FILE* f = fopen(stamp_path.c_str(), "ab")) { fwrite(st.data(), 4, st.size(), f); fclose(f); }
      }
    } else {
      launch_fwd_fused(dim3(d.R, 2), s, d, rp, P0, P1, L, w);
    }
    MQ_HIP(hipGetLastError());
  } else {
    pt.begin(PH_FC1);
    {
      // the dense agent-input copy (XIN) is dW1's operand, fused or not
      Fc1Prob p{d, rp, h->on, h->tg, h->off[MQ_P_FC1_W], h->off[MQ_P_FC1_B], w.X1, w.XIN, RT};
      MQ_HIP(launch_gemm(p, (int)RT, 2 * mq::H, 1, s));
    }
    pt.begin(PH_GI);
    {
      GiProb p{w.X1, h->on, h->tg, h->off[MQ_P_RNN_W_IH], h->off[MQ_P_RNN_B_IH], w.GI, RT};
      MQ_HIP(launch_gemm(p, (int)RT, mq::G3, 2, s));
    }
    pt.begin(PH_GRUF);
    {
      const int rw_fwd = p.rw_fwd;
      hipError_t e = rw_fwd == 1 ? launch_gru_fwd<1>(d, h, L, w, s)
                   : rw_fwd == 2 ? launch_gru_fwd<2>(d, h, L, w, s)
                   : rw_fwd == 4 ? launch_gru_fwd<4>(d, h, L, w, s)
                                 : launch_gru_fwd<8>(d, h, L, w, s);
      MQ_HIP(e);
    }
    pt.begin(PH_FC2);
    {
      Fc2Prob p{w.Hs, h->on, h->tg, h->off[MQ_P_FC2_W], h->off[MQ_P_FC2_B], w.Q, RT, d.A};
      MQ_HIP(launch_gemm(p, (int)RT, d.A, 2, s));
    }
  }
  return MQ_OK;
}

// The QMIX hypernet as a launch of its own (no forward carried it).
int Step::hypernet(const StepPlan& p) {
  if (p.hyp_place != HYP_OWN_LAUNCH) return MQ_OK;
  pt.begin(PH_HYP);
  if (p.hyper2) {
    // layer 1 (pre-activations A1, and S0), then layer 2 into HYP: both nets each (hyper2_kernels.hpp)
    const Hyp2Lay& y = h->y2;
    Hyp1Prob p1{d, rp, y, h->on, h->tg, h->A1, w.S0};
    MQ_HIP(launch_gemm(p1, d.M, y.N1, 2, s));
    Hyp2FwdProb p2{y, h->on, h->tg, h->A1, w.HYP, d.M, d.NH};
    MQ_HIP(launch_gemm(p2, d.M, d.NH, 2, s));
    return MQ_OK;
  }
  if (p.hyper == MQ_HYP_WS) {
    // wave-specialised weight streaming (hyper_kernel.hpp)
    MQ_LDS(hyper_ws_kernel<0>, hyper_ws_lds_bytes(d.S));
    hipLaunchKernelGGL(hyper_ws_kernel<0>, dim3((d.M + HYR - 1) / HYR, 2), dim3(HYWS_THREADS),
                       hyper_ws_lds_bytes(d.S), s, d, rp, (const float*)h->on, (const float*)h->tg, L, w.HYP,
                       w.S0);
    MQ_HIP(hipGetLastError());
  } else if (p.hyper == MQ_HYP_LDS) {
    const size_t dyn = HyperGeom(d.S, d.NH).lds_bytes();
    MQ_LDS(hyper_kernel<0>, dyn);
    hipLaunchKernelGGL(hyper_kernel<0>, dim3((d.M + HYR - 1) / HYR, 2), dim3(256), dyn, s, d, rp,
                       (const float*)h->on, (const float*)h->tg, L, w.HYP, w.S0);
    MQ_HIP(hipGetLastError());
  } else {
    HypProb p{d, rp, L, h->on, h->tg, w.HYP, w.S0};
    MQ_HIP(launch_gemm(p, d.M, d.NH, 2, s));
  }
  return MQ_OK;
}

int Step::mixer_tail(const StepPlan& p) {
  const mq_config& c = h->cfg;
  pt.begin(PH_MIX);
  if (rnorm) {   // the batch's rewards into the running statistics, and RS: the rewards every launch below reads
    hipLaunchKernelGGL(reward_norm_kernel, dim3(1), dim3(RN_THREADS), 0, s, d, rp, h->rew_state, h->RS);
    MQ_HIP(hipGetLastError());
  }
  if (!p.lambda) {
    if (rnorm && p.per)
      launch_mix_rs<MIX_ONE_STEP | MIX_PER | MIX_RS>(p.mix, p.nblk_mix, h, d, rp, L, w, curmax, s, h->per.weights,
                                                     h->TDA);
    else if (rnorm) launch_mix_rs<MIX_ONE_STEP | MIX_RS>(p.mix, p.nblk_mix, h, d, rp, L, w, curmax, s);
    else if (p.per) launch_mix_per<MIX_ONE_STEP>(p.mix, p.nblk_mix, h, d, rp, L, w, curmax, s);
    else launch_mix<MIX_ONE_STEP>(p.mix, p.nblk_mix, h, d, rp, L, w, curmax, s);
    MQ_HIP(hipGetLastError());
  } else {
    // TD(lambda): y' of every (t, b), the backward scan over t per episode, then the loss against its targets
    const int k = c.mixer == MQ_MIXER_NONE ? d.n : 1;
    const size_t dyn = td_lambda_lds_bytes(d.T, k);
    MQ_LDS(td_lambda_kernel, dyn);
    launch_mix<MIX_LAMBDA_TARGETS>(p.mix, p.nblk_mix, h, d, rp, L, w, curmax, s);
    MQ_HIP(hipGetLastError());
    const float lg = (float)((double)c.td_lambda * (double)c.gamma);
    const float og = (float)((1.0 - (double)c.td_lambda) * (double)c.gamma);
    if (rnorm) {
      MQ_LDS(td_lambda_rs_kernel, dyn);
      hipLaunchKernelGGL(td_lambda_rs_kernel, dim3(d.B), dim3(256), dyn, s, d, rp, (const float*)h->YT, h->G, k, lg, og,
                         (const float*)h->RS);
    } else {
      hipLaunchKernelGGL(td_lambda_kernel, dim3(d.B), dim3(256), dyn, s, d, rp, (const float*)h->YT, h->G, k, lg, og);
    }
    MQ_HIP(hipGetLastError());
    if (p.per) launch_mix_per<MIX_LAMBDA_LOSS>(p.mix, p.nblk_mix, h, d, rp, L, w, curmax, s);
    else launch_mix<MIX_LAMBDA_LOSS>(p.mix, p.nblk_mix, h, d, rp, L, w, curmax, s);
    MQ_HIP(hipGetLastError());
  }
  if (p.per) {   // the new priorities of the batch's episodes, from the tail's |td m| record
    hipLaunchKernelGGL(per_priority_kernel, dim3((d.B + 3) / 4), dim3(256), 0, s, d, rp, (const float*)h->TDA,
                       h->per.prio, h->per.prio_max, h->per.n_prio, h->per.eps);
    MQ_HIP(hipGetLastError());
  }
  return MQ_OK;
}

// The two-layer hypernet behind the mixer tail's dHYP: layer 2's backward into dA1, then every hypernet weight and
// bias gradient as p.ns m-slices of slab_mix (reduce() sums them).
int Step::hypernet2_backward(const StepPlan& p) {
  if (!p.hyper2) return MQ_OK;
  pt.begin(PH_DWH);
  const Hyp2Lay& y = h->y2;
  Hyp2BwdProb pb{y, h->on, h->A1, w.dHYP, h->dA1, d.M, d.NH};
  MQ_HIP(launch_gemm(pb, d.M, y.N1, 1, s));
  const int t0 = (y.nE + GBM - 1) / GBM, t1 = (y.E + GBM - 1) / GBM, t2 = (y.N1 + GBM - 1) / GBM;
  Hyp2DwProb pw{y, h->A1, h->dA1, w.dHYP, w.S0, w.slab_mix, h->len_mix, h->off[MQ_P_HW1_W], d.M, d.NH, d.S, p.ns, t0, t1};
  MQ_HIP(launch_gemm(pw, (t0 + t1 + t2) * GBM, std::max(y.He, d.S), p.ns, s));
  return MQ_OK;
}

// BPTT, with dX1 / dW1 as GEMMs behind the unfused recurrence.
int Step::bptt(const StepPlan& p) {
  pt.begin(PH_GRUB);
  const float* P0 = h->on;
  const int64_t l1 = (int64_t)mq::H * d.I + mq::H;
  const size_t dyn = ((size_t)2 * d.A * mq::H + d.A) * sizeof(float);   // the one-row kernels' fc2 staging
  if (p.ffn) {
    // dP2 (in dGI's buffer, as [RT][H]) and the fc2-gradient slabs, then dP1, [dWr | dbr] and dW1 as GEMMs
    const size_t dyn2 = ffn_dp2_lds_bytes(d.A);
    MQ_LDS(ffn_dp2_kernel, dyn2);
    hipLaunchKernelGGL(ffn_dp2_kernel, dim3(p.ffn_nblk2), dim3(256), dyn2, s, d, rp, P0 + h->off[MQ_P_FC2_W],
                       (const float*)w.dch, (const float*)w.Hs, w.dGI, w.slab_rnn + ffn_w2_slabs(p), p.ffn_rpb);
    MQ_HIP(hipGetLastError());
    pt.begin(PH_DX1);
    {
      FfnDx1Prob px{w.dGI, P0 + h->off[MQ_P_FFN_W], w.X1, w.dP1, RT};
      MQ_HIP(launch_gemm(px, (int)RT, mq::H, 1, s));
    }
    pt.begin(PH_DW1);
    {
      FfnDwrProb pr{w.dGI, w.X1, w.slab_rnn, RT, p.ffn_wr_ns};
      MQ_HIP(launch_gemm(pr, mq::H, mq::H, p.ffn_wr_ns, s));
      Dw1Prob p1{d.I, w.dP1, w.XIN, w.slab_fc1, RT, p.dw1_ns};
      MQ_HIP(launch_gemm(p1, mq::H, d.I, p.dw1_ns, s));
    }
    return MQ_OK;
  }
  if (p.fwd == FWD_TILES) {
    // the two-role (chain / weight-gradient waves) BPTT, 512 threads
    dispatch_kq1(p.kq1, [&](auto K) {
      hipLaunchKernelGGL(gru_bwd_split_kernel<decltype(K)::value>, dim3(p.nblk_bwd), dim3(512), 0, s, d, rp, P0, L, w,
                         h->len_rnn, l1);
    });
    MQ_HIP(hipGetLastError());
  } else if (p.fused_bwd) {
    // one row per workgroup: dW_hh / dW_ih / dX1 / dW1 on the chain's idle matrix cores (gru_bwd_fused.hpp)
    if (p.dwh_in_bwd) {   // dW_hyper's tiles in this grid: the reduction's dW_hyper blocks, same geometry
      w.dwh_tj = p.tj;
      w.dwh_ns = p.ns;
      w.dwh_n = p.ndwh;
      w.dwh_len = h->len_mix;
    }
    // diagnostic (MQ_DIAG bwd_stamp=<file>): step stamps of the first 8 workgroups
    std::string bstamp_path;
    const bool bstamp = !p.dwh_in_bwd && env_item("MQ_DIAG", "bwd_stamp", &bstamp_path) && !bstamp_path.empty() &&
                        d.Tp <= BSTN - BSTH;
    if (p.lean) {
      if (p.dwh_in_bwd) MQ_LDS((gru_bwd_fused_kernel<1, false, kBwdLean>), dyn);
      else MQ_LDS((gru_bwd_fused_kernel<0, true, kBwdLean>), dyn);   // the larger of the two builds
    } else {
      if (p.dwh_in_bwd) MQ_LDS(gru_bwd_fused_kernel<1>, dyn);
      else MQ_LDS((gru_bwd_fused_kernel<0, true>), dyn);
    }
    if (p.dwh_in_bwd) launch_bwd_fused_dwh(dyn, s, d, rp, P0, L, w, h->pitch_rnn, l1, p.lean);
    else launch_bwd_fused(dim3(d.R), dyn, s, d, rp, P0, L, w, h->pitch_rnn, l1, p.lean, bstamp);
    if (bstamp) {
      std::vector<uint32_t> st((size_t)8 * BSTN);
      MQ_HIP(hipMemcpyAsync(st.data(), w.GI, st.size() * 4, hipMemcpyDeviceToHost, s));
      MQ_HIP(hipStreamSynchronize(s));
      if (FILE* f = fopen(bstamp_path.c_str(), "ab")) { fwrite(st.data(), 4, st.size(), f); fclose(f); }
    }
    MQ_HIP(hipGetLastError());
  } else {
    {
      const int rw_bwd = p.rw_bwd, nblk = p.nblk_bwd;
      if (rw_bwd == 1) MQ_LDS(gru_bwd_kernel<1>, dyn);
      else if (rw_bwd == 2) MQ_LDS(gru_bwd_kernel<2>, dyn);
      else MQ_LDS(gru_bwd_kernel<4>, dyn);
      hipError_t e = rw_bwd == 1 ? launch_gru_bwd<1>(d, rp, h, L, w, s, nblk, dyn)
                   : rw_bwd == 2 ? launch_gru_bwd<2>(d, rp, h, L, w, s, nblk, dyn)
                                 : launch_gru_bwd<4>(d, rp, h, L, w, s, nblk, dyn);
      MQ_HIP(e);
    }
    pt.begin(PH_DX1);
    {
      Dx1Prob p{w.dGI, h->on + h->off[MQ_P_RNN_W_IH], w.X1, w.dP1, RT};
      MQ_HIP(launch_gemm(p, (int)RT, mq::H, 1, s));
    }
    pt.begin(PH_DW1);
    {
      const int ns = p.dw1_ns;
      Dw1Prob p{d.I, w.dP1, w.XIN, w.slab_fc1, RT, ns};
      MQ_HIP(launch_gemm(p, mq::H, d.I, ns, s));
    }
  }
  return MQ_OK;
}

// The slab reductions into the flat gradient buffer; pass 1 shares its launch with dW_hyper (dwh_red1_kernel) unless
// dW_hyper's tiles rode in the BPTT's grid.
int Step::reduce(const StepPlan& p) {
  const bool qmix = h->cfg.mixer == MQ_MIXER_QMIX;
  RedBuilder rb(w.red_tmp);
  rb.add(w.slab_fc1, p.nsplit_fc1, (int64_t)mq::H * d.I + mq::H, h->grad + h->off[MQ_P_FC1_W], true);
  if (p.ffn) {   // [rnn.w | rnn.b] from the split-K slabs, [fc2.w | fc2.b] from ffn_dp2_kernel's
    rb.add(w.slab_rnn, p.ffn_wr_ns, FfnDwrProb::LEN, h->grad + h->off[MQ_P_FFN_W], true);
    rb.add(w.slab_rnn + ffn_w2_slabs(p), p.ffn_nblk2, (int64_t)d.A * mq::H + d.A, h->grad + h->off[MQ_P_FC2_W], true);
  } else if (p.fused_bwd) {   // [W_ih | W_hh] in the BPTT's C-tile order (red_dst), then the biases and fc2
    const int64_t lm = 2LL * mq::G3 * mq::H;
    rb.add(w.slab_rnn, p.nblk_bwd, lm, h->grad + h->off[MQ_P_RNN_W_IH], true, h->pitch_rnn, false, 1);
    rb.add(w.slab_rnn + lm, p.nblk_bwd, h->len_rnn - lm, h->grad + h->off[MQ_P_RNN_W_IH] + lm, true, h->pitch_rnn);
  } else {
    rb.add(w.slab_rnn, p.nblk_bwd, h->len_rnn, h->grad + h->off[MQ_P_RNN_W_IH], true);
  }
  if (qmix) {
    // dW_hyper's few m-slice slabs go straight to pass 2 (they are written in the same launch as pass 1)
    const bool direct = rb.add(w.slab_mix, p.nsplit_mix, h->len_mix, h->grad + h->off[MQ_P_HW1_W], true, 0, true);
    if (p.dwh_in_red1 && !direct)   // pass-1 blocks would read slabs the dW_hyper blocks of the same grid still write
      return set_err(MQ_ERR_STATE, "dW_hyper fused with reduction pass 1 needs a direct slab region");
    rb.add(w.slab_v2, p.nblk_mix, d.E + 1, h->grad + h->off[MQ_P_V2_W], true);
  }
  rb.add(w.loss_part, p.nblk_mix, MQ_NSUMS, h->grad + h->P, false);
  if (p.dwh_in_red1) {
    pt.begin(PH_DWH);
    const int ndwh_pad = (p.ndwh + 15) / 16 * 16;
    hipLaunchKernelGGL(dwh_red1_kernel<4>, dim3(ndwh_pad + rb.b1), dim3(256), 0, s, d, L, (const float*)w.dHYP,
                       (const float*)w.S0, w.slab_mix, h->len_mix, p.ns, p.tj, p.ndwh, ndwh_pad, rb.pl);
    MQ_HIP(hipGetLastError());
    pt.begin(PH_RED);
  } else {
    pt.begin(PH_RED);
    if (rb.b1 > 0) {
      hipLaunchKernelGGL(red_pass1_kernel, dim3(rb.b1), dim3(256), 0, s, rb.pl);
      MQ_HIP(hipGetLastError());
    }
  }
  hipLaunchKernelGGL(red_pass2_kernel, dim3(rb.b2), dim3(256), 0, s, rb.pl, w.norm_part);
  MQ_HIP(hipGetLastError());
  h->n_norm_part = rb.b2;
  pt.end();
  return MQ_OK;
}

// One acting step of the feed-forward agent (mq_mac_forward / mq_agent_forward on an MQ_AGENT_FFN handle): the three
// layers in one launch, h = relu(rnn(x1)) to h_out; the incoming hidden state is not read.
int ffn_step(const mq_handle* h, const Dims& d, const Rep& rp, int32_t which, int t, const float* xin_dense, int rows,
             float* h_out, float* q_out, hipStream_t s) {
  const size_t smem = ffn_step_lds_bytes(d.I);
  MQ_LDS(ffn_step_kernel, smem);
  hipLaunchKernelGGL(ffn_step_kernel, dim3(rows), dim3(256), smem, s, d, rp, (const float*)(which ? h->tg : h->on),
                     h->off[MQ_P_FC1_W], h->off[MQ_P_FC1_B], h->off[MQ_P_FFN_W], h->off[MQ_P_FFN_B],
                     h->off[MQ_P_FC2_W], h->off[MQ_P_FC2_B], t, xin_dense, h_out, q_out);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

}  // namespace

extern "C" {

const char* mq_last_error(void) {
  std::lock_guard<std::mutex> lk(g_err_mu);
  return g_err.c_str();
}

const char* mq_phase_names(void) { return kPhaseNames; }

int mq_create(const mq_config* cfg, mq_handle** out) {
  if (!cfg || !out) return set_err(MQ_ERR_ARG, "NULL argument");
  const mq_config& c = *cfg;
  if (c.mixer != MQ_MIXER_NONE && c.mixer != MQ_MIXER_VDN && c.mixer != MQ_MIXER_QMIX)
    return set_err(MQ_ERR_ARG, "Mixer " + std::to_string(c.mixer) + " not recognised.");
  if (c.rnn_hidden_dim != mq::H) return set_err(MQ_ERR_ARG, "rnn_hidden_dim must be 64");
  if (c.n_agents < 1 || c.n_agents > 64) return set_err(MQ_ERR_ARG, "n_agents must be in [1, 64]");
  if (c.n_actions < 1 || c.n_actions > 64) return set_err(MQ_ERR_ARG, "n_actions must be in [1, 64]");
  if (c.obs_dim < 1 || c.state_dim < 1) return set_err(MQ_ERR_ARG, "obs_dim / state_dim must be positive");
  if (c.mixer == MQ_MIXER_QMIX && (c.mixing_embed_dim < 1 || c.mixing_embed_dim > 64))
    return set_err(MQ_ERR_ARG, "mixing_embed_dim must be in [1, 64]");
  if (c.mixer == MQ_MIXER_QMIX && (c.hypernet_layers < 0 || c.hypernet_layers > 2))
    return set_err(MQ_ERR_ARG, "hypernet_layers must be 1 or 2 (0: 1)");
  if (c.agent != MQ_AGENT_GRU && c.agent != MQ_AGENT_FFN)
    return set_err(MQ_ERR_ARG, "agent must be MQ_AGENT_GRU (0) or MQ_AGENT_FFN (1)");
  const bool hyper2 = c.mixer == MQ_MIXER_QMIX && c.hypernet_layers == 2;
  if (hyper2 && (c.hypernet_embed < 1 || c.hypernet_embed > MQ_HYPERNET_EMBED_MAX))
    return set_err(MQ_ERR_ARG, "hypernet_embed must be in [1, " + std::to_string((int)MQ_HYPERNET_EMBED_MAX) + "]");
  if (c.max_batch < 1 || c.max_seq < 2) return set_err(MQ_ERR_ARG, "max_batch >= 1 and max_seq >= 2 required");
  if (!(c.huber_delta >= 0.0f)) return set_err(MQ_ERR_ARG, "huber_delta must be >= 0 (0: the reference's L2 loss)");
  if (!(c.td_lambda >= 0.0f && c.td_lambda <= 1.0f))
    return set_err(MQ_ERR_ARG, "td_lambda must be in [0, 1] (0: the reference's one-step target)");
  // the scan stages an episode's inputs in dynamic LDS (td_lambda_kernel.hpp): kept within what a launch may ask for
  // without raising the kernel's dynamic-LDS attribute
  const PlanOverrides ov = read_plan_overrides();
  if ((c.td_lambda > 0.0f || ov.lambda_path) &&
      td_lambda_lds_bytes(c.max_seq - 1, c.mixer == MQ_MIXER_NONE ? c.n_agents : 1) > kLambdaLdsMax)
    return set_err(MQ_ERR_ARG, "td_lambda: max_seq " + std::to_string(c.max_seq) + " needs more than " +
                                   std::to_string(kLambdaLdsMax) + " B of LDS for the TD(lambda) scan");

  mq_handle* h = new mq_handle();
  h->cfg = c;
  h->ov = ov;
  h->hyper2 = hyper2;
  h->ffn = c.agent == MQ_AGENT_FFN;
  const Dims dmax = mq::make_dims(c, c.max_batch, c.max_seq, c.max_seq);   // E, I, NH as every step derives them
  h->E = dmax.E; h->I = dmax.I; h->NH = dmax.NH;
  compute_layout(h);

  const int64_t n = c.n_agents, A = c.n_actions, Hd = mq::H;
  const int64_t RT = (int64_t)c.max_seq * c.max_batch * n;
  const int64_t Mm = (int64_t)(c.max_seq - 1) * c.max_batch;
  const int64_t Rm = (int64_t)c.max_batch * n;
  const int64_t nmix = (Mm + 3) / 4;
  const int64_t NH = h->NH;
  auto ng = [](int64_t ns) { return std::min<int64_t>(ns, kRedZ); };
  const int64_t nfc1 = std::max<int64_t>(kNsplitMax, Rm);   // fc1 slabs: split-K GEMM, or one per fused-BPTT row
  // the feed-forward agent's slab_rnn, from the largest batch: its [dWr | dbr] slabs, then its [dW2 | db2] slabs
  const int64_t ffn_ns = ffn_wr_ns_max(RT), ffn_nb = ffn_nblk2_max(RT);
  const int64_t ffn_slabs = h->ffn ? ffn_ns * FfnDwrProb::LEN + ffn_nb * (A * Hd + A) : 0;
  const int64_t red_tmp = (h->ffn ? ng(ffn_ns) * FfnDwrProb::LEN + ng(ffn_nb) * (A * Hd + A) : 0) + ng(Rm) * h->len_rnn + ng(nfc1) * (Hd * h->I + Hd) + ng(kNsplitMax) * h->len_mix +
                          ng(nmix) * (h->E + 1) + ng(nmix) * 8;
  const int64_t norm_parts = (Hd * h->I + Hd + 255) / 256 + (h->len_rnn + 255) / 256 + (h->len_mix + 255) / 256 +
                             (h->E + 1 + 255) / 256 + 1 + 8;
  int64_t sizes[20] = {
      2 * RT * Hd,                                   // X1
      2 * RT * 3 * Hd,                               // GI
      2 * RT * Hd,                                   // Hs (both nets)
      RT * 5 * Hd,                                   // Gates (four gate planes, or five coefficient planes)
      2 * RT * A,                                    // Q
      2 * Mm * NH,                                   // HYP
      Mm * NH,                                       // dHYP
      Mm * n,                                        // dch
      RT * 3 * Hd,                                   // dGI
      RT * Hd,                                       // dP1
      nfc1 * (Hd * h->I + Hd),                       // slab_fc1
      std::max(Rm * h->pitch_rnn, ffn_slabs),        // slab_rnn (RW = 1 worst case)
      (int64_t)kNsplitMax * h->len_mix,              // slab_mix
      nmix * (h->E + 1),                             // slab_v2
      nmix * 8,                                      // loss_part
      std::max<int64_t>(norm_parts, 256),            // norm_part
      Mm * n,                                        // curmax (int32)
      red_tmp,                                       // two-pass reduction partials
      RT * h->I,                                     // XIN (dense agent inputs)
      Mm * c.state_dim,                              // S0 (gathered state[:, :-1] rows)
  };
  int64_t total = 0, offs[20];
  for (int i = 0; i < 20; ++i) { offs[i] = total; total += align_up(std::max<int64_t>(sizes[i], 1)); }
  hipError_t e = hipMalloc(&h->ws, total * sizeof(float));
  if (e != hipSuccess) {
    delete h;
    return set_err(MQ_ERR_HIP, std::string("workspace hipMalloc(") + std::to_string(total * 4) + " B): " +
                                   hipGetErrorString(e));
  }
  float* base = (float*)h->ws;
  Work& w = h->w;
  w.X1 = base + offs[0]; w.GI = base + offs[1]; w.Hs = base + offs[2]; w.Gates = base + offs[3];
  w.Q = base + offs[4]; w.HYP = base + offs[5]; w.dHYP = base + offs[6]; w.dch = base + offs[7];
  w.dGI = base + offs[8]; w.dP1 = base + offs[9]; w.slab_fc1 = base + offs[10]; w.slab_rnn = base + offs[11];
  w.slab_mix = base + offs[12]; w.slab_v2 = base + offs[13]; w.loss_part = base + offs[14];
  w.norm_part = base + offs[15];
  h->curmax_ws = (int32_t*)(base + offs[16]);
  w.red_tmp = base + offs[17];
  w.XIN = base + offs[18];
  w.S0 = base + offs[19];
  w.curmax = h->curmax_ws;
  if (c.td_lambda > 0.0f || ov.lambda_path) {
    const int64_t len = align_up((int64_t)c.max_seq * c.max_batch * (c.mixer == MQ_MIXER_NONE ? n : 1));
    e = hipMalloc((void**)&h->YT, 2 * len * sizeof(float));
    if (e != hipSuccess) {
      (void)hipFree(h->ws);
      delete h;
      return set_err(MQ_ERR_HIP, std::string("TD(lambda) workspace hipMalloc: ") + hipGetErrorString(e));
    }
    h->G = h->YT + len;
  }
  if (hyper2) {
    const int64_t len = align_up(Mm * h->y2.N1);
    e = hipMalloc((void**)&h->A1, 3 * len * sizeof(float));
    if (e != hipSuccess) {
      (void)hipFree(h->ws);
      if (h->YT) (void)hipFree(h->YT);
      delete h;
      return set_err(MQ_ERR_HIP, std::string("two-layer hypernet workspace hipMalloc: ") + hipGetErrorString(e));
    }
    h->dA1 = h->A1 + 2 * len;
  }
  *out = h;
  return MQ_OK;
}

int mq_destroy(mq_handle* h) {
  if (!h) return MQ_OK;
  for (auto e : h->ev0) (void)hipEventDestroy(e);
  for (auto e : h->ev1) (void)hipEventDestroy(e);
  if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
  if (h->ev_join) (void)hipEventDestroy(h->ev_join);
  if (h->side) (void)hipStreamDestroy(h->side);
  if (h->ws) (void)hipFree(h->ws);
  if (h->YT) (void)hipFree(h->YT);
  if (h->TDA) (void)hipFree(h->TDA);
  if (h->RS) (void)hipFree(h->RS);
  if (h->A1) (void)hipFree(h->A1);
  if (h->comm && h->comm_owned) (void)ncclCommDestroy(h->comm);
  delete h;
  return MQ_OK;
}

int mq_param_offsets(const mq_handle* h, int64_t* offsets) {
  if (!h || !offsets) return set_err(MQ_ERR_ARG, "NULL argument");
  for (int i = 0; i <= MQ_P_COUNT; ++i) offsets[i] = h->off[i];
  return MQ_OK;
}

int mq_bind(mq_handle* h, float* online, float* target, float* grad, float* sq_avg, float* stats,
            int32_t* cur_max) {
  // target/grad/sq_avg/stats may be NULL for an inference-only handle (mq_mac_forward / mq_agent_forward)
  if (!h || !online) return set_err(MQ_ERR_ARG, "NULL handle or online parameters in mq_bind");
  h->on = online; h->tg = target; h->grad = grad; h->sq = sq_avg; h->stats = stats; h->curmax_user = cur_max;
  return MQ_OK;
}

static int fb_impl(mq_handle* h, const mq_replay* batch, hipStream_t s);

int mq_forward_backward(mq_handle* h, const mq_replay* batch, void* stream) {
  return fb_impl(h, batch, (hipStream_t)stream);
}

int mq_train_step(mq_handle* h, const mq_replay* batch, void* stream) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  const int rc = fb_impl(h, batch, (hipStream_t)stream);
  if (rc) return rc;
  return mq_apply(h, stream);
}

static int fb_impl(mq_handle* h, const mq_replay* batch, hipStream_t s) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  if (!h->on || !h->tg || !h->grad || !h->sq || !h->stats)
    return set_err(MQ_ERR_STATE, "training needs online, target, grad, sq_avg and stats bound (mq_bind)");
  const bool per = h->per_armed;
  h->per_armed = false;   // armed for one step, whatever becomes of it
  int rc = check_batch(h, batch);
  if (rc) return rc;
  if (per) {
    if (h->comm || h->dp)
      return set_err(MQ_ERR_ARG, "prioritized replay does not support data parallelism (a communicator is attached "
                                 "or mq_set_data_parallel is on)");
    if (!batch->ep_ids || batch->ep_ids_host)
      return set_err(MQ_ERR_ARG, "a prioritized-replay step needs device episode ids (mq_replay.ep_ids, ep_ids_host "
                                 "NULL): they are the priority slots it writes");
    if (batch->n_episodes > h->per.n_prio)
      return set_err(MQ_ERR_ARG, "mq_per.n_prio is smaller than the replay's n_episodes");
  }
  const bool rnorm = h->rew_state != nullptr;
  if (rnorm && (h->comm || h->dp))
    return set_err(MQ_ERR_ARG, "reward standardisation does not support data parallelism (a communicator is attached "
                               "or mq_set_data_parallel is on): each rank would see only its shard's rewards");
  Step st{h, make_dims(h, batch), make_rep(batch), make_lay(h), h->w, h->curmax_user ? h->curmax_user : h->curmax_ws,
          s, PhaseTimer{h, s}, rnorm};
  // a handle with the TD(lambda) workspace runs the lambda passes: cfg.td_lambda > 0 or MQ_PLAN lambda_path=1
  const StepPlan p = plan_step(h->cfg, h->ov, st.d, st.rp.nids > 0, h->YT != nullptr, device_cus(h), per,
                                 h->hyper2 ? 2 : 1, h->cfg.agent);
  st.w.rec_coef = p.rec_coef;
  if ((rc = st.forward(p)) || (rc = st.hypernet(p)) || (rc = st.mixer_tail(p)) || (rc = st.hypernet2_backward(p)) ||
      (rc = st.bptt(p)) ||
      (rc = st.reduce(p)))
    return rc;
  if (h->comm) {   // native data parallelism: the whole [grads | sums] buffer, summed over the ranks in stream order
    const ncclResult_t r = ncclAllReduce(h->grad, h->grad, (size_t)(h->P + MQ_NSUMS), ncclFloat, ncclSum, h->comm, s);
    if (r != ncclSuccess) return set_err(MQ_ERR_HIP, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
  }
  h->last = st.d;
  h->plan = p.report;
  h->have_fb = true;
  h->have_lambda = p.lambda;
  h->have_per = p.per;
  h->have_h2 = p.hyper2;
  h->have_rs = rnorm;
  h->hyper_layers = p.hyper_layers;
  h->last_agent = p.agent_report;
  return MQ_OK;
}

int mq_apply(mq_handle* h, void* stream) {
  if (!h || !h->on) return set_err(MQ_ERR_STATE, "mq_apply before mq_bind");
  if (!h->have_fb) return set_err(MQ_ERR_STATE, "mq_apply before mq_forward_backward");
  hipStream_t s = (hipStream_t)stream;
  PhaseTimer pt{h, s};
  pt.begin(PH_APPLY);
  if (h->dp || h->comm) {   // the gradient was all-reduced after the reduce pass: its norm partials are stale
    h->n_norm_part = 256;
    hipLaunchKernelGGL(sumsq_kernel, dim3(h->n_norm_part), dim3(256), 0, s, (const float*)h->grad, h->P,
                       h->w.norm_part);
    MQ_HIP(hipGetLastError());
  }
  if (h->adam) {
    const AdamHP hp = make_adam_hp(h->cfg.lr, h->ad.beta1, h->ad.beta2, h->ad.eps, h->ad.weight_decay,
                                   h->adam_step + 1, h->cfg.grad_norm_clip, h->cfg.n_agents);
    hipLaunchKernelGGL(apply_adam_kernel, dim3(adam_blocks(h->on, h->grad, h->ad.exp_avg, h->sq, h->P)), dim3(256), 0,
                       s, h->on, h->grad, h->ad.exp_avg, h->sq, h->P, (const float*)h->w.norm_part, h->n_norm_part, hp,
                       h->stats, (const int*)nullptr);
    MQ_HIP(hipGetLastError());
    ++h->adam_step;
  } else {
    OptHP hp{h->cfg.lr, h->cfg.optim_alpha, h->cfg.optim_eps, h->cfg.grad_norm_clip, h->cfg.n_agents};
    int blocks = (int)std::min<int64_t>((h->P + 255) / 256, 1024);
    hipLaunchKernelGGL(apply_kernel, dim3(blocks), dim3(256), 0, s, h->on, h->grad, h->sq, h->P,
                       (const float*)h->w.norm_part, h->n_norm_part, hp, h->stats, (const int*)nullptr);
    MQ_HIP(hipGetLastError());
  }
  if (h->soft) {   // the step's last launch: the targets follow the parameters the apply just wrote
    hipLaunchKernelGGL(soft_update_kernel, dim3(soft_blocks(h->tg, h->on, h->P)), dim3(256), 0, s, h->tg,
                       (const float*)h->on, h->P, h->soft_omt, h->soft_tau, (const int*)nullptr);
    MQ_HIP(hipGetLastError());
  }
  h->last_soft = h->soft ? 1 : 0;
  pt.end();
  ++h->tstep;
  return MQ_OK;
}

int mq_set_soft_target(mq_handle* h, double tau) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  if (tau == 0.0) {
    h->soft = false;
    h->soft_omt = h->soft_tau = 0.0f;
    return MQ_OK;
  }
  if (!(tau > 0.0 && tau <= 1.0)) return set_err(MQ_ERR_ARG, "mq_set_soft_target: tau must be in (0, 1] (0: off)");
  h->soft_omt = (float)(1.0 - tau);
  h->soft_tau = (float)tau;
  h->soft = true;
  return MQ_OK;
}

int32_t mq_last_soft_target(const mq_handle* h) { return h ? h->last_soft : -1; }

int mq_soft_update(float* target, const float* online, int64_t n, float one_minus_tau, float tau, void* stream) {
  if (!target || !online) return set_err(MQ_ERR_ARG, "NULL pointer in mq_soft_update");
  if (((uintptr_t)target | (uintptr_t)online) & 3)
    return set_err(MQ_ERR_ARG, "mq_soft_update: a pointer is not aligned to a float");
  if (n < 0) return set_err(MQ_ERR_ARG, "mq_soft_update: n must be >= 0");
  if (!(tau > 0.0f && tau <= 1.0f)) return set_err(MQ_ERR_ARG, "mq_soft_update: tau must be in (0, 1]");
  if (n == 0) return MQ_OK;
  hipLaunchKernelGGL(soft_update_kernel, dim3(soft_blocks(target, online, n)), dim3(256), 0, (hipStream_t)stream,
                     target, online, n, one_minus_tau, tau, (const int*)nullptr);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mq_set_reward_norm(mq_handle* h, double* state) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  if (!state) {
    h->rew_state = nullptr;
    return MQ_OK;
  }
  if ((uintptr_t)state & 7) return set_err(MQ_ERR_ARG, "mq_set_reward_norm: state is not aligned to a double");
  if (!h->RS) {
    const int64_t len = align_up((int64_t)h->cfg.max_seq * h->cfg.max_batch);
    const hipError_t e = hipMalloc((void**)&h->RS, len * sizeof(float));
    if (e != hipSuccess) {
      h->RS = nullptr;
      return set_err(MQ_ERR_HIP, std::string("reward-standardisation workspace hipMalloc: ") + hipGetErrorString(e));
    }
  }
  h->rew_state = state;
  return MQ_OK;
}

int32_t mq_last_reward_norm(const mq_handle* h) { return h && h->have_fb ? (h->have_rs ? 1 : 0) : -1; }

int mq_set_adam(mq_handle* h, const mq_adam* a) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  if (!a) {   // back to RMSprop
    h->adam = false;
    h->ad = mq_adam{};
    h->adam_step = 0;
    return MQ_OK;
  }
  if (!a->exp_avg) return set_err(MQ_ERR_ARG, "mq_set_adam: exp_avg is NULL");
  if ((uintptr_t)a->exp_avg & 3) return set_err(MQ_ERR_ARG, "mq_set_adam: exp_avg is not aligned to a float");
  const int rc = check_adam("mq_set_adam", a->beta1, a->beta2, a->eps, a->weight_decay);
  if (rc) return rc;
  if (a->step < 0) return set_err(MQ_ERR_ARG, "mq_set_adam: step must be >= 0");
  h->ad = *a;
  h->adam_step = a->step;
  h->adam = true;
  return MQ_OK;
}

int64_t mq_opt_step(const mq_handle* h) { return h ? h->adam_step : -1; }

int mq_adam_update(float* p, float* g, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int64_t step, void* stream) {
  if (!p || !g || !exp_avg || !exp_avg_sq) return set_err(MQ_ERR_ARG, "NULL pointer in mq_adam_update");
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 3)
    return set_err(MQ_ERR_ARG, "mq_adam_update: a pointer is not aligned to a float");
  if (n < 0) return set_err(MQ_ERR_ARG, "mq_adam_update: n must be >= 0");
  if (step < 1) return set_err(MQ_ERR_ARG, "mq_adam_update: step is the 1-based step number (>= 1)");
  if (!(lr >= 0.0f)) return set_err(MQ_ERR_ARG, "mq_adam_update: lr must be >= 0");
  const int rc = check_adam("mq_adam_update", beta1, beta2, eps, weight_decay);
  if (rc) return rc;
  if (n == 0) return MQ_OK;
  const AdamHP hp = make_adam_hp(lr, beta1, beta2, eps, weight_decay, step, 0.0f, 1);
  hipLaunchKernelGGL(apply_adam_kernel, dim3(adam_blocks(p, g, exp_avg, exp_avg_sq, n)), dim3(256), 0,
                     (hipStream_t)stream, p, g, exp_avg, exp_avg_sq, n, (const float*)nullptr, 0, hp, (float*)nullptr,
                     (const int*)nullptr);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mq_last_plan(const mq_handle* h, mq_plan* out) {
  if (!h || !out) return set_err(MQ_ERR_ARG, "NULL argument");
  if (!h->have_fb) return set_err(MQ_ERR_STATE, "no forward/backward has run");
  *out = h->plan;
  return MQ_OK;
}

int32_t mq_last_hyper_layers(const mq_handle* h) { return h && h->have_fb ? h->hyper_layers : -1; }

int32_t mq_last_agent(const mq_handle* h) { return h && h->have_fb ? h->last_agent : -1; }

int mq_set_data_parallel(mq_handle* h, int32_t on) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  h->dp = on != 0;
  return MQ_OK;
}

int mq_comm_unique_id(uint8_t* id) {
  if (!id) return set_err(MQ_ERR_ARG, "NULL id");
  ncclUniqueId u;
  const ncclResult_t r = ncclGetUniqueId(&u);
  if (r != ncclSuccess) return set_err(MQ_ERR_HIP, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
  static_assert(sizeof(u) == MQ_COMM_ID_BYTES, "ncclUniqueId size");
  std::memcpy(id, &u, sizeof(u));
  return MQ_OK;
}

// One RCCL communicator over `world` ranks (the calling process's current HIP device).
static int comm_init(ncclComm_t* out, const uint8_t* id, int32_t rank, int32_t world) {
  if (!id || world < 1 || rank < 0 || rank >= world) return set_err(MQ_ERR_ARG, "mq_comm_attach: bad id, rank or world");
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  const ncclResult_t r = ncclCommInitRank(out, world, u, rank);
  if (r != ncclSuccess) return set_err(MQ_ERR_HIP, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
  return MQ_OK;
}

int mq_comm_attach(mq_handle* h, const uint8_t* id, int32_t rank, int32_t world) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  if (h->comm) return set_err(MQ_ERR_STATE, "a communicator is already attached (mq_comm_detach first)");
  const int rc = comm_init(&h->comm, id, rank, world);
  if (rc) return rc;
  h->comm_world = world;
  h->comm_owned = true;
  return MQ_OK;
}

int mq_comm_create(const uint8_t* id, int32_t rank, int32_t world, void** comm) {
  if (!comm) return set_err(MQ_ERR_ARG, "NULL comm");
  ncclComm_t c = nullptr;
  const int rc = comm_init(&c, id, rank, world);
  if (rc) return rc;
  *comm = (void*)c;
  return MQ_OK;
}

int mq_comm_free(void* comm) {
  if (comm) (void)ncclCommDestroy((ncclComm_t)comm);
  return MQ_OK;
}

int mq_comm_use(mq_handle* h, void* comm) {
  if (!h || !comm) return set_err(MQ_ERR_ARG, "NULL handle or communicator");
  if (h->comm) return set_err(MQ_ERR_STATE, "a communicator is already attached (mq_comm_detach first)");
  int world = 0;
  const ncclResult_t r = ncclCommCount((ncclComm_t)comm, &world);
  if (r != ncclSuccess) return set_err(MQ_ERR_ARG, std::string("ncclCommCount: ") + ncclGetErrorString(r));
  h->comm = (ncclComm_t)comm;
  h->comm_world = world;
  h->comm_owned = false;
  return MQ_OK;
}

int32_t mq_comm_world(const mq_handle* h) { return h ? h->comm_world : 0; }

int mq_comm_detach(mq_handle* h) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  if (h->comm && h->comm_owned) (void)ncclCommDestroy(h->comm);
  h->comm = nullptr;
  h->comm_world = 0;
  h->comm_owned = false;
  return MQ_OK;
}

int mq_per_sample(const float* prio, int32_t n_live, const float* u, int32_t batch, float alpha, float beta,
                  int64_t* ids, float* weights, void* stream) {
  if (!prio || !u || !ids || !weights) return set_err(MQ_ERR_ARG, "NULL pointer in mq_per_sample");
  if (!(alpha >= 0.0f)) return set_err(MQ_ERR_ARG, "per alpha must be >= 0");
  if (!(beta >= 0.0f && beta <= 1.0f)) return set_err(MQ_ERR_ARG, "per beta must be in [0, 1]");
  if (n_live < 1 || n_live > PER_NMAX)
    return set_err(MQ_ERR_ARG, "mq_per_sample: n_live " + std::to_string(n_live) + " outside [1, " +
                                   std::to_string(PER_NMAX) + "]");
  if (batch < 1) return set_err(MQ_ERR_ARG, "mq_per_sample: batch must be >= 1");
  static_assert(PER_NMAX == MQ_PER_MAX_LIVE && PER_THREADS == 1 << PER_SCAN_DEPTH, "per_kernels.hpp constants");
  hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(PER_THREADS), 0, (hipStream_t)stream, prio, (int)n_live, u,
                     (int)batch, alpha, beta, ids, weights);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mq_set_per(mq_handle* h, const mq_per* per) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  h->per_armed = false;
  if (!per) return MQ_OK;
  if (!per->weights || !per->prio || !per->prio_max) return set_err(MQ_ERR_ARG, "NULL pointer in mq_per");
  if (!(per->eps > 0.0f)) return set_err(MQ_ERR_ARG, "per eps must be > 0");
  if (per->n_prio < 1) return set_err(MQ_ERR_ARG, "mq_per.n_prio must be >= 1");
  if (!h->TDA) {
    const int64_t len = align_up((int64_t)h->cfg.max_seq * h->cfg.max_batch);
    const hipError_t e = hipMalloc((void**)&h->TDA, len * sizeof(float));
    if (e != hipSuccess) {
      h->TDA = nullptr;
      return set_err(MQ_ERR_HIP, std::string("prioritized-replay workspace hipMalloc: ") + hipGetErrorString(e));
    }
  }
  h->per = *per;
  h->per_armed = true;
  return MQ_OK;
}

int mq_update_targets(mq_handle* h, void* stream) {
  if (!h || !h->on || !h->tg) return set_err(MQ_ERR_STATE, "mq_update_targets needs online and target bound");
  MQ_HIP(hipMemcpyAsync(h->tg, h->on, h->P * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MQ_OK;
}

int mq_copy_intermediate(mq_handle* h, int which, float* dst, int64_t* count, void* stream) {
  if (!h || !h->have_fb) return set_err(MQ_ERR_STATE, "no forward/backward has run");
  const Dims& d = h->last;
  const int64_t RT = (int64_t)d.Tp * d.R;
  const float* src;
  int64_t cnt;
  switch (which) {
    case 0: src = h->w.Q; cnt = RT * d.A; break;
    case 1: src = h->w.Q + RT * d.A; cnt = RT * d.A; break;
    case 2: src = h->w.dch; cnt = (int64_t)d.T * d.R; break;
    case 3: src = h->w.X1; cnt = RT * mq::H; break;
    case 4:
    case 5:
      if (!h->have_lambda) return set_err(MQ_ERR_STATE, "the last step did not run the TD(lambda) passes");
      src = which == 4 ? h->YT : h->G;
      cnt = (int64_t)d.T * d.B * (d.mixer == MQ_MIXER_NONE ? d.n : 1);
      break;
    case 6:
      if (!h->have_per) return set_err(MQ_ERR_STATE, "the last step was not a prioritized-replay step");
      src = h->TDA;
      cnt = (int64_t)d.T * d.B;
      break;
    case 8:
      if (!h->have_rs) return set_err(MQ_ERR_STATE, "the last step did not standardise the rewards");
      src = h->RS;
      cnt = (int64_t)d.T * d.B;
      break;
    case 9:
      if (!(h->last_agent & 1)) return set_err(MQ_ERR_STATE, "the last step did not run the feed-forward agent");
      src = h->w.Hs;
      cnt = RT * mq::H;
      break;
    case 7: {   // the online net's first 2 He columns of A1's rows (row pitch N1)
      if (!h->have_h2) return set_err(MQ_ERR_STATE, "the last step did not run the two-layer hypernet");
      const int64_t wd = 2 * h->y2.He;
      if (count) *count = (int64_t)d.M * wd;
      if (dst)
        MQ_HIP(hipMemcpy2DAsync(dst, wd * sizeof(float), h->A1, h->y2.N1 * sizeof(float), wd * sizeof(float), d.M,
                                hipMemcpyDeviceToDevice, (hipStream_t)stream));
      return MQ_OK;
    }
    default: return set_err(MQ_ERR_ARG, "unknown intermediate id");
  }
  if (count) *count = cnt;
  if (dst) MQ_HIP(hipMemcpyAsync(dst, src, cnt * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return MQ_OK;
}

int mq_mac_forward(mq_handle* h, const mq_replay* batch, int32_t t, const float* h_in, float* h_out, float* q_out,
                   int32_t which, void* stream) {
  if (!h || !h->on) return set_err(MQ_ERR_STATE, "mq_mac_forward before mq_bind");
  if (which && !h->tg) return set_err(MQ_ERR_STATE, "target parameters not bound");
  if (!batch || !batch->obs || !batch->actions || !batch->filled || (!h_in && !h->ffn) || !h_out || !q_out)
    return set_err(MQ_ERR_ARG, "NULL pointer in mq_mac_forward");
  if (t < 0 || t >= batch->t_stride) return set_err(MQ_ERR_ARG, "t outside the stored episode");
  if (batch->batch_size < 1) return set_err(MQ_ERR_ARG, "empty batch");
  if (const int rc = check_ids(batch)) return rc;
  mq_replay b = *batch;
  b.t_len = std::max(2, std::min(b.t_stride, 2));
  const Dims d = make_dims(h, &b);
  const Rep rp = make_rep(batch);
  const Lay L = make_lay(h);
  if (h->ffn) return ffn_step(h, d, rp, which, (int)t, nullptr, d.R, h_out, q_out, (hipStream_t)stream);
  const size_t smem = (size_t)(((d.I + 3) & ~3) + mq::H * 3 + mq::G3 * 2) * sizeof(float);
  hipLaunchKernelGGL(mac_step_kernel, dim3(d.R), dim3(256), smem, (hipStream_t)stream, d, rp,
                     (const float*)(which ? h->tg : h->on), L, (int)t, (const float*)nullptr, h_in, h_out, q_out);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mq_agent_forward(mq_handle* h, const float* inputs, int32_t rows, const float* h_in, float* h_out, float* q_out,
                     int32_t which, void* stream) {
  if (!h || !h->on) return set_err(MQ_ERR_STATE, "mq_agent_forward before mq_bind");
  if (which && !h->tg) return set_err(MQ_ERR_STATE, "target parameters not bound");
  if (!inputs || (!h_in && !h->ffn) || !h_out || !q_out || rows < 0)
    return set_err(MQ_ERR_ARG, "bad mq_agent_forward args");
  if (rows == 0) return MQ_OK;
  mq_replay b;
  std::memset(&b, 0, sizeof(b));
  b.batch_size = 1; b.t_len = 2; b.t_stride = 2;
  Dims d = make_dims(h, &b);
  d.n = 1;   // rows are independent here: block -> row, agent id unused
  const Rep rp = make_rep(&b);
  const Lay L = make_lay(h);
  if (h->ffn) return ffn_step(h, d, rp, which, 0, inputs, rows, h_out, q_out, (hipStream_t)stream);
  const size_t smem = (size_t)(((d.I + 3) & ~3) + mq::H * 3 + mq::G3 * 2) * sizeof(float);
  hipLaunchKernelGGL(mac_step_kernel, dim3(rows), dim3(256), smem, (hipStream_t)stream, d, rp,
                     (const float*)(which ? h->tg : h->on), L, 0, inputs, h_in, h_out, q_out);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mq_greedy_actions(const float* q, const int32_t* avail, int64_t* out, int32_t rows, int32_t n_actions,
                      void* stream) {
  if (!q || !avail || !out || rows < 0 || n_actions < 1) return set_err(MQ_ERR_ARG, "bad mq_greedy_actions args");
  if (rows == 0) return MQ_OK;
  hipLaunchKernelGGL(greedy_kernel, dim3((rows + 255) / 256), dim3(256), 0, (hipStream_t)stream, q, avail, out,
                     (int)rows, (int)n_actions);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mq_qmix_forward(const float* mixer, int32_t n_agents, int32_t state_dim, int32_t embed_dim,
                    const float* agent_qs, const float* states, float* q_tot, int32_t rows, void* stream) {
  if (!mixer || !agent_qs || !states || !q_tot || rows < 0) return set_err(MQ_ERR_ARG, "bad mq_qmix_forward args");
  if (n_agents < 1 || n_agents > 64 || embed_dim < 1 || embed_dim > 64 || state_dim < 1)
    return set_err(MQ_ERR_ARG, "mq_qmix_forward: n_agents / embed_dim in [1, 64], state_dim >= 1");
  if (rows == 0) return MQ_OK;
  const size_t lds = qmix_forward_lds(n_agents, state_dim, embed_dim);
  if (lds > 160 * 1024) return set_err(MQ_ERR_ARG, "mq_qmix_forward: state_dim too large for the LDS staging");
  MQ_LDS(qmix_forward_kernel, lds);
  if (lds > 64 * 1024)   // past the default dynamic LDS of a launch (n_agents = embed_dim = 64: 68.6 KB at least)
    MQ_HIP(hipFuncSetAttribute((const void*)qmix_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
  hipLaunchKernelGGL(qmix_forward_kernel, dim3((rows + QMF_ROWS - 1) / QMF_ROWS), dim3(256), lds,
                     (hipStream_t)stream, mixer, (int)n_agents, (int)state_dim, (int)embed_dim, agent_qs, states,
                     q_tot, (int)rows);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mq_qmix_forward2(const float* mixer, int32_t n_agents, int32_t state_dim, int32_t embed_dim,
                     int32_t hypernet_embed, const float* agent_qs, const float* states, float* q_tot, int32_t rows,
                     void* stream) {
  if (!mixer || !agent_qs || !states || !q_tot || rows < 0) return set_err(MQ_ERR_ARG, "bad mq_qmix_forward2 args");
  if (n_agents < 1 || n_agents > 64 || embed_dim < 1 || embed_dim > 64 || state_dim < 1)
    return set_err(MQ_ERR_ARG, "mq_qmix_forward2: n_agents / embed_dim in [1, 64], state_dim >= 1");
  if (hypernet_embed < 1 || hypernet_embed > MQ_HYPERNET_EMBED_MAX)
    return set_err(MQ_ERR_ARG, "mq_qmix_forward2: hypernet_embed must be in [1, " +
                                   std::to_string((int)MQ_HYPERNET_EMBED_MAX) + "]");
  if (rows == 0) return MQ_OK;
  const size_t lds = qmix_forward2_lds(n_agents, state_dim, embed_dim, hypernet_embed);
  if (lds > 64 * 1024) return set_err(MQ_ERR_ARG, "mq_qmix_forward2: state_dim too large for the LDS staging");
  const int64_t S = state_dim, E = embed_dim, He = hypernet_embed, nE = (int64_t)n_agents * E;
  Qmix2Off o;
  Hyp2Lay& y = o.Y;   // parameters() order, relative to hyper_w_1.0.weight
  y.w1a = 0; y.b1a = He * S; y.w12 = y.b1a + He; y.b12 = y.w12 + nE * He;
  y.wfa = y.b12 + nE; y.bfa = y.wfa + He * S; y.wf2 = y.bfa + He; y.bf2 = y.wf2 + E * He;
  y.hbw = y.bf2 + E; y.hbb = y.hbw + E * S; y.v0w = y.hbb + E; y.v0b = y.v0w + E * S;
  o.v2w = y.v0b + E; o.v2b = o.v2w + E;
  y.He = (int)He; y.E = (int)E; y.nE = (int)nE; y.N1 = (int)(2 * He + 2 * E);
  hipLaunchKernelGGL(qmix_forward2_kernel, dim3((rows + QMF2_ROWS - 1) / QMF2_ROWS), dim3(256), lds,
                     (hipStream_t)stream, mixer, o, (int)n_agents, (int)state_dim, agent_qs, states, q_tot,
                     (int)rows);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mq_set_timing(mq_handle* h, int32_t slots, uint32_t phase_mask) {
  if (!h || slots < 0 || slots > 4096) return set_err(MQ_ERR_ARG, "bad mq_set_timing args");
  for (auto e : h->ev0) (void)hipEventDestroy(e);
  for (auto e : h->ev1) (void)hipEventDestroy(e);
  h->ev0.clear(); h->ev1.clear(); h->ev_used.clear();
  h->slots = slots;
  h->mask = phase_mask;
  h->tstep = 0;
  const size_t n = (size_t)slots * PH_N;
  h->ev0.resize(n); h->ev1.resize(n); h->ev_used.assign(n, 0);
  for (size_t i = 0; i < n; ++i) {
    MQ_HIP(hipEventCreate(&h->ev0[i]));
    MQ_HIP(hipEventCreate(&h->ev1[i]));
  }
  return MQ_OK;
}

int mq_phase_times(mq_handle* h, float* ms, int32_t cap, int32_t* n) {
  if (!h || !ms) return set_err(MQ_ERR_ARG, "NULL argument");
  if (n) *n = PH_N;
  for (int p = 0; p < PH_N && p < cap; ++p) {
    double sum = 0.0;
    int cnt = 0;
    for (int sl = 0; sl < h->slots; ++sl) {
      const size_t i = (size_t)sl * PH_N + p;
      if (!h->ev_used[i]) continue;
      float t = 0.0f;
      MQ_HIP(hipEventSynchronize(h->ev1[i]));
      MQ_HIP(hipEventElapsedTime(&t, h->ev0[i], h->ev1[i]));
      sum += t;
      ++cnt;
    }
    ms[p] = cnt ? (float)(sum / cnt) : 0.0f;
  }
  return MQ_OK;
}

}  // extern "C"
#include "coma_host.hpp"
