// The QMIX / VDN / IQL learner's handle (include/mq_learner.h): its config and layout, what the caller bound, the
// device buffers it owns, the opt-ins' settings, and the record of the last step. Beside it, the batch checks and the
// replay / layout argument blocks every entry point builds from it.
#pragma once
#include <vector>

#include <rccl/rccl.h>
#include "learner_layout.hpp"

using namespace mq;

namespace {

constexpr size_t kLambdaLdsMax = 64 * 1024;   // dynamic LDS of td_lambda_kernel (checked in mq_create)
enum Phase { PH_FC1, PH_GI, PH_GRUF, PH_FC2, PH_HYP, PH_MIX, PH_GRUB, PH_DX1, PH_DW1, PH_DWH, PH_RED, PH_APPLY,
             PH_N };
const char* kPhaseNames = "fc1;gi;gru_fwd;fc2;hyper;mix;gru_bwd;dx1;dw1;dwh;reduce;apply";

// What the last step was: mq_forward_backward assigns it whole when it succeeds (mq_apply adds `soft`), and
// mq_copy_intermediate and the mq_last_* getters read it.
struct LastStep {
  bool ran = false;   // a forward/backward has run
  Dims d{};
  mq_plan plan{};
  int n_norm_part = 0;    // reduction pass 2's blocks: the norm partials mq_apply sums
  bool lambda = false;    // it ran the TD(lambda) passes (mq_copy_intermediate 4 / 5)
  bool per = false;       // it was a prioritized-replay step (6)
  bool hyper2 = false;    // it ran the two-layer hypernet (7)
  bool rs = false;        // it standardised the rewards (8, mq_last_reward_norm)
  int hyper_layers = 0;   // mq_last_hyper_layers
  int agent = 0;          // mq_last_agent
  int soft = -1;          // of the last mq_apply (mq_last_soft_target); a forward/backward carries it over
};

}  // namespace

struct mq_handle : Layout {   // the layout is make_layout(cfg)
  mq_config cfg;
  // bound (caller-owned)
  float *on = nullptr, *tg = nullptr, *grad = nullptr, *sq = nullptr, *stats = nullptr;
  int32_t* curmax_user = nullptr;
  // workspace (handle-owned): one allocation, carved by mq_ws_table
  DevBuf<float> ws;
  Work w;
  LastStep last;
  PlanOverrides ov;   // MQ_PLAN, read once in mq_create (step_plan.hpp)
  bool dp = false;   // gradient buffer is summed across ranks between mq_forward_backward and mq_apply
  ncclComm_t comm = nullptr;   // mq_comm_attach / mq_comm_use: the library all-reduces the grad buffer itself
  int comm_world = 0;
  bool comm_owned = false;     // mq_comm_attach created it (freed on detach); mq_comm_use borrows the caller's
  hipStream_t side = nullptr;   // COMA: the actor's side stream (coma_host.hpp)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // the TD(lambda) passes' workspace, allocated only for a handle that runs them: y' and, behind it in the same
  // allocation, the lambda targets G; [max_seq * max_batch] (no mixer: x n_agents) floats each
  DevBuf<float> YT;
  float* G = nullptr;
  // prioritized replay (mq_set_per): armed for the next step only; TDA [max_seq * max_batch] is the tail's |td m|
  // record, allocated by the first mq_set_per
  mq_per per{};
  bool per_armed = false;
  DevBuf<float> TDA;
  // the two-layer hypernet (hyper2): the layer-1 tensors A1 [2][max M][N1] and, behind them, dA1 [max M][N1],
  // allocated only for such a handle
  DevBuf<float> A1;
  float* dA1 = nullptr;
  // Adam (mq_set_adam): mq_apply launches apply_adam_kernel with ad.exp_avg beside sq; adam_step counts the steps applied
  bool adam = false;
  mq_adam ad{};
  int64_t adam_step = 0;
  // soft target updates (mq_set_soft_target): soft_update_kernel behind the apply, target = target omt + online tau
  bool soft = false;
  float soft_omt = 0.0f, soft_tau = 0.0f;
  // reward standardisation (mq_set_reward_norm): the caller's [mean, var, count] doubles, and RS [max_seq * max_batch],
  // the step's standardised rewards, allocated by the first mq_set_reward_norm
  double* rew_state = nullptr;
  DevBuf<float> RS;
  int num_cu = 0;
  // timing: a ring of `slots` steps x PH_N (start, stop) event pairs; phases outside `mask` are not recorded
  int slots = 0;
  uint32_t mask = 0;
  int64_t tstep = 0;
  std::vector<hipEvent_t> ev0, ev1;
  std::vector<uint8_t> ev_used;

  explicit mq_handle(const mq_config& c) : Layout(make_layout(c)), cfg(c) {}
  ~mq_handle() {   // the buffers free themselves
    for (auto e : ev0) (void)hipEventDestroy(e);
    for (auto e : ev1) (void)hipEventDestroy(e);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (side) (void)hipStreamDestroy(side);
    if (comm && comm_owned) (void)ncclCommDestroy(comm);
  }
};

namespace {
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

// One RCCL communicator over `world` ranks (the calling process's current HIP device).
int comm_init(ncclComm_t* out, const uint8_t* id, int32_t rank, int32_t world) {
  if (!id || world < 1 || rank < 0 || rank >= world) return set_err(MQ_ERR_ARG, "mq_comm_attach: bad id, rank or world");
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof(u));
  const ncclResult_t r = ncclCommInitRank(out, world, u, rank);
  if (r != ncclSuccess) return set_err(MQ_ERR_HIP, std::string("ncclCommInitRank: ") + ncclGetErrorString(r));
  return MQ_OK;
}

}  // namespace
