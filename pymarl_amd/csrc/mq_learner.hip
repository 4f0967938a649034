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
//
// The host side by file: host_util.hpp (errors, HIP / LDS checks, device-buffer owner, workspace table),
// learner_layout.hpp (parameter layout and workspace sizes from the config), step_plan.hpp and reduce_plan.hpp (what a
// step launches, decided without a HIP call), learner_handle.hpp (mq_handle, batch checks), step_launch.hpp (the
// launches), optim_host.hpp (Adam's host side, and launch_reduce: the two-pass reduction's launcher outside Step),
// actor_plan.hpp (what the policy-gradient actor launches, for the three learners below), coma_plan.hpp (what a COMA
// step launches, decided without a HIP call) and coma_host.hpp (the COMA learner: its handle, the shared actor, the
// step's phases), a2c_host.hpp (the actor-critic learner, with a2c_plan.hpp and a2c_kernels.hpp), ppo_host.hpp (its
// PPO step). This file holds the C ABI.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>

#include "step_launch.hpp"
#include "module_fwd.hpp"
#include "optim_host.hpp"
#include "coma_host.hpp"
#include "a2c_host.hpp"
#include "ppo_host.hpp"

namespace {

// One acting step (mq_mac_forward / mq_agent_forward), a workgroup per row: mac_step_kernel or, for the feed-forward
// agent, ffn_step_kernel (the three layers, h = relu(rnn(x1)) to h_out; the incoming hidden state is not read).
int agent_step(const mq_handle* h, const Dims& d, const Rep& rp, int32_t which, int t, const float* xin_dense, int rows,
               const float* h_in, float* h_out, float* q_out, hipStream_t s) {
  const float* P = which ? h->tg : h->on;
  if (h->ffn) {
    const size_t smem = ffn_step_lds_bytes(d.I);
    MQ_LDS(ffn_step_kernel, smem);
    hipLaunchKernelGGL(ffn_step_kernel, dim3(rows), dim3(256), smem, s, d, rp, P, h->off[MQ_P_FC1_W],
                       h->off[MQ_P_FC1_B], h->off[MQ_P_FFN_W], h->off[MQ_P_FFN_B], h->off[MQ_P_FC2_W],
                       h->off[MQ_P_FC2_B], t, xin_dense, h_out, q_out);
  } else {
    hipLaunchKernelGGL(mac_step_kernel, dim3(rows), dim3(256), mac_step_lds_bytes(d.I), s, d, rp, P, make_lay(h), t,
                       xin_dense, h_in, h_out, q_out);
  }
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

  std::unique_ptr<mq_handle> h(new mq_handle(c));   // a failure below frees whatever it had allocated
  h->ov = ov;
  const WsTable ws = mq_ws_table(c, *h, h->w);
  int rc = ws_carve(h->ws, ws, "workspace hipMalloc(" + std::to_string(ws_assign(ws, nullptr) * 4) + " B)");
  if (rc) return rc;
  if (c.td_lambda > 0.0f || ov.lambda_path) {
    const int64_t len = align_up((int64_t)c.max_seq * c.max_batch * (c.mixer == MQ_MIXER_NONE ? c.n_agents : 1));
    if ((rc = h->YT.alloc(2 * len, "TD(lambda) workspace hipMalloc"))) return rc;
    h->G = h->YT.p + len;
  }
  if (hyper2) {
    const int64_t len = align_up((int64_t)(c.max_seq - 1) * c.max_batch * h->y2.N1);
    if ((rc = h->A1.alloc(3 * len, "two-layer hypernet workspace hipMalloc"))) return rc;
    h->dA1 = h->A1.p + 2 * len;
  }
  *out = h.release();
  return MQ_OK;
}

int mq_destroy(mq_handle* h) {
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

int mq_forward_backward(mq_handle* h, const mq_replay* batch, void* stream) {
  if (!h) return set_err(MQ_ERR_ARG, "NULL handle");
  hipStream_t s = (hipStream_t)stream;
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
  Step st{h, mq::make_dims(h->cfg, batch->batch_size, batch->t_len, batch->t_stride), make_rep(batch), make_lay(h),
          h->w, h->curmax_user ? h->curmax_user : h->w.curmax, s, PhaseTimer{h, s}, rnorm};
  // a handle with the TD(lambda) workspace runs the lambda passes: cfg.td_lambda > 0 or MQ_PLAN lambda_path=1
  const StepPlan p = plan_step(h->cfg, h->ov, st.d, st.rp.nids > 0, h->YT.p != nullptr, device_cus(h), per,
                                 h->hyper2 ? 2 : 1, h->cfg.agent);
  st.w.rec_coef = p.rec_coef;
  if ((rc = st.forward(p)) || (rc = st.hypernet(p)) || (rc = st.mixer_tail(p)) || (rc = st.hypernet2_backward(p)) ||
      (rc = st.bptt(p)) || (rc = st.reduce(p)))
    return rc;
  if (h->comm) {   // native data parallelism: the whole [grads | sums] buffer, summed over the ranks in stream order
    const ncclResult_t r = ncclAllReduce(h->grad, h->grad, (size_t)(h->P + MQ_NSUMS), ncclFloat, ncclSum, h->comm, s);
    if (r != ncclSuccess) return set_err(MQ_ERR_HIP, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
  }
  h->last = LastStep{true, st.d, p.report, st.n_norm_part, p.lambda, p.per, p.hyper2, rnorm, p.hyper_layers,
                     p.agent_report, h->last.soft};
  return MQ_OK;
}

int mq_train_step(mq_handle* h, const mq_replay* batch, void* stream) {
  const int rc = mq_forward_backward(h, batch, stream);
  return rc ? rc : mq_apply(h, stream);
}

int mq_apply(mq_handle* h, void* stream) {
  if (!h || !h->on) return set_err(MQ_ERR_STATE, "mq_apply before mq_bind");
  if (!h->last.ran) return set_err(MQ_ERR_STATE, "mq_apply before mq_forward_backward");
  hipStream_t s = (hipStream_t)stream;
  PhaseTimer pt{h, s};
  pt.begin(PH_APPLY);
  int n_norm_part = h->last.n_norm_part;
  if (h->dp || h->comm) {   // the gradient was all-reduced after the reduce pass: its norm partials are stale
    n_norm_part = 256;
    hipLaunchKernelGGL(sumsq_kernel, dim3(n_norm_part), dim3(256), 0, s, (const float*)h->grad, h->P,
                       h->w.norm_part);
    MQ_HIP(hipGetLastError());
  }
  if (h->adam) {
    const AdamHP hp = make_adam_hp(h->cfg.lr, h->ad.beta1, h->ad.beta2, h->ad.eps, h->ad.weight_decay,
                                   h->adam_step + 1, h->cfg.grad_norm_clip, h->cfg.n_agents);
    hipLaunchKernelGGL(apply_adam_kernel, dim3(vec4_blocks({h->on, h->grad, h->ad.exp_avg, h->sq}, h->P)), dim3(256), 0,
                       s, h->on, h->grad, h->ad.exp_avg, h->sq, h->P, (const float*)h->w.norm_part, n_norm_part, hp,
                       h->stats, (const int*)nullptr);
    MQ_HIP(hipGetLastError());
    ++h->adam_step;
  } else {
    OptHP hp{h->cfg.lr, h->cfg.optim_alpha, h->cfg.optim_eps, h->cfg.grad_norm_clip, h->cfg.n_agents};
    int blocks = (int)std::min<int64_t>((h->P + 255) / 256, 1024);
    hipLaunchKernelGGL(apply_kernel, dim3(blocks), dim3(256), 0, s, h->on, h->grad, h->sq, h->P,
                       (const float*)h->w.norm_part, n_norm_part, hp, h->stats, (const int*)nullptr);
    MQ_HIP(hipGetLastError());
  }
  if (h->soft) {   // the step's last launch: the targets follow the parameters the apply just wrote
    hipLaunchKernelGGL(soft_update_kernel, dim3(vec4_blocks({h->tg, h->on}, h->P)), dim3(256), 0, s, h->tg,
                       (const float*)h->on, h->P, h->soft_omt, h->soft_tau, (const int*)nullptr);
    MQ_HIP(hipGetLastError());
  }
  h->last.soft = h->soft ? 1 : 0;
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

int32_t mq_last_soft_target(const mq_handle* h) { return h ? h->last.soft : -1; }

int mq_soft_update(float* target, const float* online, int64_t n, float one_minus_tau, float tau, void* stream) {
  if (!target || !online) return set_err(MQ_ERR_ARG, "NULL pointer in mq_soft_update");
  if (((uintptr_t)target | (uintptr_t)online) & 3)
    return set_err(MQ_ERR_ARG, "mq_soft_update: a pointer is not aligned to a float");
  if (n < 0) return set_err(MQ_ERR_ARG, "mq_soft_update: n must be >= 0");
  if (!(tau > 0.0f && tau <= 1.0f)) return set_err(MQ_ERR_ARG, "mq_soft_update: tau must be in (0, 1]");
  if (n == 0) return MQ_OK;
  hipLaunchKernelGGL(soft_update_kernel, dim3(vec4_blocks({target, online}, n)), dim3(256), 0, (hipStream_t)stream,
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
  const int rc = h->RS.alloc(align_up((int64_t)h->cfg.max_seq * h->cfg.max_batch),
                             "reward-standardisation workspace hipMalloc");
  if (rc) return rc;
  h->rew_state = state;
  return MQ_OK;
}

int32_t mq_last_reward_norm(const mq_handle* h) { return h && h->last.ran ? (h->last.rs ? 1 : 0) : -1; }

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
  hipLaunchKernelGGL(apply_adam_kernel, dim3(vec4_blocks({p, g, exp_avg, exp_avg_sq}, n)), dim3(256), 0,
                     (hipStream_t)stream, p, g, exp_avg, exp_avg_sq, n, (const float*)nullptr, 0, hp, (float*)nullptr,
                     (const int*)nullptr);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mq_last_plan(const mq_handle* h, mq_plan* out) {
  if (!h || !out) return set_err(MQ_ERR_ARG, "NULL argument");
  if (!h->last.ran) return set_err(MQ_ERR_STATE, "no forward/backward has run");
  *out = h->last.plan;
  return MQ_OK;
}

int32_t mq_last_hyper_layers(const mq_handle* h) { return h && h->last.ran ? h->last.hyper_layers : -1; }

int32_t mq_last_agent(const mq_handle* h) { return h && h->last.ran ? h->last.agent : -1; }

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
  const int rc = h->TDA.alloc(align_up((int64_t)h->cfg.max_seq * h->cfg.max_batch),
                              "prioritized-replay workspace hipMalloc");
  if (rc) return rc;
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
  if (!h || !h->last.ran) return set_err(MQ_ERR_STATE, "no forward/backward has run");
  const LastStep& last = h->last;
  const Dims& d = last.d;
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
      if (!last.lambda) return set_err(MQ_ERR_STATE, "the last step did not run the TD(lambda) passes");
      src = which == 4 ? h->YT.p : h->G;
      cnt = (int64_t)d.T * d.B * (d.mixer == MQ_MIXER_NONE ? d.n : 1);
      break;
    case 6:
      if (!last.per) return set_err(MQ_ERR_STATE, "the last step was not a prioritized-replay step");
      src = h->TDA;
      cnt = (int64_t)d.T * d.B;
      break;
    case 8:
      if (!last.rs) return set_err(MQ_ERR_STATE, "the last step did not standardise the rewards");
      src = h->RS;
      cnt = (int64_t)d.T * d.B;
      break;
    case 9:
      if (!(last.agent & 1)) return set_err(MQ_ERR_STATE, "the last step did not run the feed-forward agent");
      src = h->w.Hs;
      cnt = RT * mq::H;
      break;
    case 7: {   // the online net's first 2 He columns of A1's rows (row pitch N1)
      if (!last.hyper2) return set_err(MQ_ERR_STATE, "the last step did not run the two-layer hypernet");
      const int64_t wd = 2 * h->y2.He;
      if (count) *count = (int64_t)d.M * wd;
      if (dst)
        MQ_HIP(hipMemcpy2DAsync(dst, wd * sizeof(float), h->A1.p, h->y2.N1 * sizeof(float), wd * sizeof(float), d.M,
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
  const Dims d = mq::make_dims(h->cfg, b.batch_size, b.t_len, b.t_stride);
  return agent_step(h, d, make_rep(batch), which, (int)t, nullptr, d.R, h_in, h_out, q_out, (hipStream_t)stream);
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
  Dims d = mq::make_dims(h->cfg, b.batch_size, b.t_len, b.t_stride);
  d.n = 1;   // rows are independent here: block -> row, agent id unused
  return agent_step(h, d, make_rep(&b), which, 0, inputs, rows, h_in, h_out, q_out, (hipStream_t)stream);
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
