/* C ABI of the MI355X-native QMIX/VDN learner hot path (libmq_learner.so, gfx950).
 *
 * This is the drop-in boundary behind pymarl's learner plugin API: the host shim
 * pymarl_amd/learners/q_learner.py (registered as learners.REGISTRY["q_learner"]) binds these symbols with
 * ctypes. Every pointer passed in is a DEVICE pointer owned by the caller (borrowed for the call or, for
 * mq_bind, until the next mq_bind / mq_destroy); the handle owns only its activation workspace. All calls
 * are asynchronous on the given HIP stream (passed as void*; NULL = the null stream) unless stated otherwise.
 * Every function returns MQ_OK (0) or an error code; mq_last_error() gives the text. No C++ exception crosses
 * this boundary.
 *
 * Reference interfaces replaced (nicholasburden/pymarl, /root/reference):
 *   mq_train_step        QLearner.train(batch, t_env, episode_num)      src/learners/q_learner.py:37-116
 *   mq_forward_backward  q_learner.py:39-101 (loss + backward, before clip/step)
 *   mq_apply             q_learner.py:102-103 (clip_grad_norm_ + RMSprop.step) and the stats of :109-116
 *   mq_set_adam          (opt-in, not in the reference) torch.optim.Adam in RMSprop's place at q_learner.py:30,103;
 *                        mq_adam_update is the same step on caller-owned buffers, mq_opt_step its step count
 *   mq_update_targets    QLearner._update_targets                       src/learners/q_learner.py:118-122
 *   mq_set_soft_target   (opt-in, not in the reference) epymarl's soft target update behind every mq_apply;
 *                        mq_soft_update is the same update on caller-owned buffers
 *   mq_set_reward_norm   (opt-in, not in the reference) epymarl's standardise_rewards in front of q_learner.py:86
 *   mq_mac_forward       BasicMAC.forward(ep_batch, t)                   src/controllers/basic_controller.py:40-75
 *   mq_agent_forward     RNNAgent.forward(inputs, hidden_state)          src/modules/agents/rnn_agent.py:27-36
 *   mq_greedy_actions    EpsilonGreedyActionSelector greedy branch      src/components/action_selectors.py:44-62
 *   mq_qmix_forward      QMixer.forward(agent_qs, states)                src/modules/mixers/qmix.py:28-47
 *   mq_replay.ep_ids     ReplayBuffer.sample -> EpisodeBatch.__getitem__ gather, episode_buffer.py:165-217,291-298
 *                        (ids drawn on the host exactly as the reference does; the gather is fused into kernels)
 */
#ifndef MQ_LEARNER_H
#define MQ_LEARNER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { MQ_MIXER_NONE = 0, MQ_MIXER_VDN = 1, MQ_MIXER_QMIX = 2 };
enum { MQ_OK = 0, MQ_ERR_ARG = 1, MQ_ERR_HIP = 2, MQ_ERR_STATE = 3 };
enum { MQ_NSUMS = 8 };   /* tail of the gradient buffer: sum (td*m)^2 (Huber: sum huber(td*m)), sum m, sum |td*m|, sum Q_tot*m, sum y*m */
enum { MQ_NSTATS = 8 };  /* loss, grad_norm, td_error_abs, q_taken_mean, target_mean, mask_sum, clip coefficient,
                           0 (reserved) */

/* Parameter tensors: RNNAgent (rnn_agent.py:19-21) then QMixer (qmix.py:14-23). mq_param_offsets fills
 * offsets[MQ_P_COUNT + 1] (last = total) with each tensor's place in the flat buffer, which follows the modules'
 * parameters() / state_dict order.
 *
 * With one hypernet layer (mq_config.hypernet_layers 0 or 1) that order is the enum's order up to MQ_P_V2_B, and
 * MQ_P_HW1_W .. MQ_P_HWF_B are hyper_w_1.weight / .bias and hyper_w_final.weight / .bias. The four second-layer
 * entries are absent: each reports offset = total (a tensor of zero floats at the end of the buffer).
 *
 * With two layers (hypernet_layers = 2) MQ_P_HW1_W / _B and MQ_P_HWF_W / _B name the state-fed FIRST layers
 * (hyper_w_1.0, hyper_w_final.0: [hypernet_embed][state_dim] and [hypernet_embed]) and MQ_P_HW1_W2 / _B2,
 * MQ_P_HWF_W2 / _B2 the second layers (hyper_w_1.2: [embed * n_agents][hypernet_embed]; hyper_w_final.2:
 * [embed][hypernet_embed]). The buffer's order is upstream PyMARL's parameters() order
 *   ... fc2.bias, hyper_w_1.0.weight, hyper_w_1.0.bias, hyper_w_1.2.weight, hyper_w_1.2.bias, hyper_w_final.0.weight,
 *   hyper_w_final.0.bias, hyper_w_final.2.weight, hyper_w_final.2.bias, hyper_b_1.weight, ... V.2.bias
 * so the offsets are NOT monotone in the enum index: never derive a tensor's size from the next enum entry's
 * offset. The new entries sit after MQ_P_V2_B so that every earlier entry keeps its number. */
enum {
  MQ_P_FC1_W, MQ_P_FC1_B, MQ_P_RNN_W_IH, MQ_P_RNN_W_HH, MQ_P_RNN_B_IH, MQ_P_RNN_B_HH, MQ_P_FC2_W, MQ_P_FC2_B,
  MQ_P_HW1_W, MQ_P_HW1_B, MQ_P_HWF_W, MQ_P_HWF_B, MQ_P_HB1_W, MQ_P_HB1_B, MQ_P_V0_W, MQ_P_V0_B, MQ_P_V2_W,
  MQ_P_V2_B, MQ_P_HW1_W2, MQ_P_HW1_B2, MQ_P_HWF_W2, MQ_P_HWF_B2, MQ_P_FFN_W, MQ_P_FFN_B, MQ_P_COUNT
};

/* The agent's middle layer (mq_config.agent). MQ_AGENT_GRU: the reference's GRUCell (rnn_agent.py:20), the default and
 * what a zeroed field selects. MQ_AGENT_FFN: epymarl's use_rnn: False, rnn = Linear(64, 64) followed by a ReLU,
 *   x1 = relu(fc1(xin));  h = relu(rnn(x1));  q = fc2(h)
 * with the incoming hidden state ignored. MQ_P_FFN_W / MQ_P_FFN_B are then rnn.weight [64][64] / rnn.bias [64], the
 * buffer's order is fc1.weight, fc1.bias, rnn.weight, rnn.bias, fc2.weight, fc2.bias, <mixer>, and the four GRU
 * entries MQ_P_RNN_* report offset = total (tensors of zero floats), as the absent hypernet entries do. With the GRU
 * the two FFN entries report offset = total. They sit after MQ_P_HWF_B2 so that every earlier entry keeps its
 * number. */
enum { MQ_AGENT_GRU = 0, MQ_AGENT_FFN = 1 };

typedef struct mq_config {
  int32_t n_agents, n_actions, obs_dim, state_dim;
  int32_t rnn_hidden_dim;    /* 64 (the reference default; the kernels are built for it) */
  int32_t mixing_embed_dim;  /* QMIX embed dim, <= 64 */
  int32_t mixer;             /* MQ_MIXER_*; unknown -> MQ_ERR_ARG (reference: ValueError, q_learner.py:26) */
  int32_t double_q, obs_last_action, obs_agent_id;
  float gamma, lr, optim_alpha, optim_eps, grad_norm_clip;
  int32_t max_batch;         /* most episodes one call may train on (workspace bound) */
  int32_t max_seq;           /* most stored steps per episode (episode_limit + 1) */
  float huber_delta;         /* TD loss: 0 = masked L2 (q_learner.py:96-97, default); > 0 = masked Huber with this
                                delta, an opt-in the reference lacks (not pinned by its goldens) */
  float td_lambda;           /* TD target: 0 = the one-step target r + gamma (1 - term) Q'_tot(t+1) (q_learner.py:86,
                                default; the kernels of that path run as they always did); in (0, 1] = TD(lambda)
                                returns, build_td_lambda_targets (rl_utils.py:4-14) over the target network's mixed
                                values with the learner's mask, as COMALearner applies it: an opt-in the reference's
                                Q learner lacks. The mixer tail then runs as three launches (targets, the backward
                                scan over t, loss + mixer backward). Outside [0, 1] or NaN: MQ_ERR_ARG; so is a
                                max_seq whose scan inputs, (max_seq - 1) * (k + 3) floats with k = 1 (no mixer:
                                n_agents), pass 64 KB of LDS. */
  int32_t hypernet_layers;   /* QMIX: 0 or 1 = hyper_w_1 / hyper_w_final are one Linear each (the reference; every
                                kernel of that path runs as it always did); 2 = Linear(S, hypernet_embed) -> ReLU ->
                                Linear(hypernet_embed, .), upstream PyMARL's two-layer hypernetwork. Anything else:
                                MQ_ERR_ARG. Ignored without a QMIX mixer. */
  int32_t hypernet_embed;    /* width of the two-layer hypernet's hidden layer, 1 .. MQ_HYPERNET_EMBED_MAX (two layers
                                only; outside: MQ_ERR_ARG) */
  int32_t agent;             /* MQ_AGENT_*: 0 = the GRU agent (the reference; every kernel of that path runs as it
                                always did), 1 = the feed-forward agent (epymarl's use_rnn: False). Anything else:
                                MQ_ERR_ARG. */
} mq_config;
enum { MQ_HYPERNET_EMBED_MAX = 64 };

/* A batch of episodes as the learner reads it: the replay storage (reference scheme dtypes, episode-major
 * [episode][t][...], run.py:122-135) plus the sampled episode ids. t_len = max_t_filled() of the batch
 * (run.py:211-212), t_stride = the storage's max_seq_length. */
typedef struct mq_replay {
  const float* obs;            /* [N][t_stride][n_agents][obs_dim] */
  const float* state;          /* [N][t_stride][state_dim] */
  const int64_t* actions;      /* [N][t_stride][n_agents][1] */
  const int32_t* avail_actions;/* [N][t_stride][n_agents][n_actions] */
  const float* reward;         /* [N][t_stride][1] */
  const uint8_t* terminated;   /* [N][t_stride][1] */
  const int64_t* filled;       /* [N][t_stride][1] */
  const int64_t* ep_ids;       /* [batch_size] episode ids (device); NULL = 0..batch_size-1 */
  int64_t n_episodes;
  int32_t batch_size, t_len, t_stride;
  /* Optional HOST copy of the ids, read during the call: when set and batch_size <= MQ_INLINE_IDS the ids travel
   * in the kernel arguments and ep_ids is not read (no host-to-device copy per step). */
  const int64_t* ep_ids_host;
  /* Optional [N][t_stride][n_agents] bitmask view of avail_actions (bit a set iff avail_actions[..][a] != 0), kept
   * by the replay buffer as episodes are inserted. When set, the mixer's double-Q selection reads these 8 bytes per
   * agent row instead of 4 n_actions (configs[2], 27m: 82 of the mixer's 262 MB); NULL reads avail_actions. */
  const uint64_t* avail_bits;
} mq_replay;

#define MQ_INLINE_IDS 256

typedef struct mq_handle mq_handle;

const char* mq_last_error(void);
int mq_create(const mq_config* cfg, mq_handle** out);
int mq_destroy(mq_handle* h);
int mq_param_offsets(const mq_handle* h, int64_t* offsets /* [MQ_P_COUNT + 1] */);

/* online/target/sq_avg: [P] floats (only `online` is required for an inference-only handle); grad: [P + MQ_NSUMS] floats (clipped grads land here after mq_apply,
 * as .grad does after clip_grad_norm_); stats: [MQ_NSTATS] floats; cur_max: optional [max_seq*max_batch*n]
 * int32 double-Q greedy actions of the last step ([t][b][agent], t < t_len-1), may be NULL. */
int mq_bind(mq_handle* h, float* online, float* target, float* grad, float* sq_avg, float* stats,
            int32_t* cur_max);

/* Loss + backward of QLearner.train on `batch`: writes UNNORMALISED gradients d(sum (td*m)^2)/dtheta and the
 * MQ_NSUMS partial sums into grad. Data-parallel callers all-reduce grad (whole buffer) between the two calls. */
int mq_forward_backward(mq_handle* h, const mq_replay* batch, void* stream);
/* Normalise by sum(m), clip_grad_norm_(grad_norm_clip), RMSprop(lr, alpha, eps) step (Adam's after mq_set_adam),
 * write stats. */
int mq_apply(mq_handle* h, void* stream);
/* mq_forward_backward + mq_apply in one call (with a communicator attached, the all-reduce between them too). */
int mq_train_step(mq_handle* h, const mq_replay* batch, void* stream);
/* Declare that the caller sums the gradient buffer across ranks between mq_forward_backward and mq_apply
 * (mq_apply then recomputes the global gradient norm from the reduced buffer). */
int mq_set_data_parallel(mq_handle* h, int32_t on);
/* Native RCCL data parallelism (SURVEY.md §8b's mq_allreduce_attach): rank 0 calls mq_comm_unique_id and ships
 * the MQ_COMM_ID_BYTES bytes to every rank over any channel; every rank (one process per GPU) then calls
 * mq_comm_attach(h, id, rank, world) once. From then on mq_forward_backward ends with one RCCL all-reduce (sum) of
 * the whole grad buffer [P + MQ_NSUMS] on `stream`, and mq_apply recomputes the norm from the sum: one call of
 * mq_train_step is a full data-parallel QLearner.train step, with no host collective in between. world = 1 is
 * allowed (the all-reduce is the identity). mq_comm_world reports the attached world size (0: none);
 * mq_comm_detach frees the communicator (mq_destroy does too). */
enum { MQ_COMM_ID_BYTES = 128 };
int mq_comm_unique_id(uint8_t* id /* [MQ_COMM_ID_BYTES] */);
int mq_comm_attach(mq_handle* h, const uint8_t* id, int32_t rank, int32_t world);
int32_t mq_comm_world(const mq_handle* h);
int mq_comm_detach(mq_handle* h);
/* SURVEY.md §8b's mq_allreduce_attach(handle, ncclComm_t): attach a communicator the CALLER owns (an ncclComm_t,
 * passed as void* so this header needs no RCCL include). The handle borrows it: detach / destroy leave it alive,
 * and one communicator may serve several handles (QMIX and COMA learners of one process). mq_comm_create /
 * mq_comm_free make and release one from a unique id for hosts without their own RCCL setup. */
int mq_comm_use(mq_handle* h, void* nccl_comm);
int mq_comm_create(const uint8_t* id, int32_t rank, int32_t world, void** nccl_comm);
int mq_comm_free(void* nccl_comm);
int mq_update_targets(mq_handle* h, void* stream);

/* Adam, an opt-in (the reference's learner has RMSprop only; pymarl2 / epymarl configs say optimizer: adam).
 * mq_set_adam makes mq_apply (and so mq_train_step) take torch.optim.Adam's step instead of RMSprop's, until
 * mq_set_adam(h, NULL) goes back (sticky). Everything in front of the apply is untouched, and so are the
 * normalisation by sum(m), clip_grad_norm_ and the stats; per element, in fp32 and torch's operand order
 * (non-amsgrad, non-maximize):
 *   gi = (g / sum(m)) * coef;  g = gi             (the clipped gradient, WITHOUT the decay term)
 *   gd = weight_decay != 0 ? gi + weight_decay * p : gi          (L2 decay: after the clip, not in grad_norm)
 *   m += (1 - beta1) * (gd - m);  v = v * beta2 + (1 - beta2) * gd * gd
 *   p += -(lr / (1 - beta1^t)) * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps))
 * with t = step + 1 the 1-based number of this step; lr / (1 - beta1^t), sqrt(1 - beta2^t), 1 - beta1 and 1 - beta2
 * are formed in double on the host and cast to float once; lr and the betas enter that arithmetic as the shortest
 * decimal that rounds to the given float (0.999f stands for 0.999, the Python float torch would be given: 1 - beta2
 * from the widened float would be off by 1.3e-5 of itself). exp_avg (m): [P] device floats, borrowed like mq_bind's
 * pointers; mq_bind's sq_avg serves as exp_avg_sq (v). step: the steps already applied (0: a fresh optimiser);
 * every mq_apply uses step + 1 and then increments the count, which mq_opt_step reports (-1: NULL handle; 0 while
 * RMSprop is selected). mq_config.optim_alpha / optim_eps are ignored while Adam is set. Data parallelism
 * (mq_set_data_parallel, an attached communicator), PER, TD(lambda), Huber and both hypernet depths work as before:
 * none of them touches the apply. MQ_ERR_ARG: exp_avg NULL, a beta outside [0, 1) or NaN, eps <= 0 or NaN,
 * weight_decay < 0 or NaN, step < 0. */
typedef struct mq_adam { float* exp_avg; float beta1, beta2, eps, weight_decay; int64_t step; } mq_adam;
int mq_set_adam(mq_handle* h, const mq_adam* a);
int64_t mq_opt_step(const mq_handle* h);
/* One Adam step (the arithmetic above with gi = g: no normalisation, no clip, no stats) on caller-owned device
 * buffers of n floats each, one launch on `stream`; step: the 1-based number of this step. The buffers need no
 * alignment beyond a float's. MQ_ERR_ARG: step < 1, a NULL pointer, n < 0, lr < 0 or NaN, and mq_set_adam's range
 * checks. */
int mq_adam_update(float* p, float* g, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                   float beta2, float eps, float weight_decay, int64_t step, void* stream);

/* Soft (Polyak) target updates, an opt-in (epymarl's target_update_interval_or_tau <= 1; the reference has the hard
 * copy of mq_update_targets only). mq_set_soft_target(h, tau) makes every mq_apply (and so mq_train_step) end with one
 * more launch, after the optimiser's, over the flat online / target buffers bound with mq_bind:
 *   target = target * (1 - tau) + online * tau
 * in fp32 with both products and the sum rounded separately (no FMA): bitwise what torch gives on the CPU for
 * t * (1.0 - tau) + p * tau. The host forms (float)(1.0 - tau) and (float)tau, each cast once from double. Sticky
 * until mq_set_soft_target(h, 0), which turns it off. Everything in front of it is untouched; data parallelism works
 * unchanged (every rank holds the same parameters). MQ_ERR_ARG: NULL handle, tau outside [0, 1] or NaN.
 * mq_last_soft_target: 1 / 0 whether the last mq_apply ran it; -1 for a NULL handle or when no step has been applied. */
int mq_set_soft_target(mq_handle* h, double tau);
int32_t mq_last_soft_target(const mq_handle* h);
/* The same update on caller-owned device buffers of n floats each, one launch on `stream`; the caller passes both
 * factors as it wants them rounded. The buffers need no alignment beyond a float's. MQ_ERR_ARG: a NULL pointer,
 * n < 0, tau outside (0, 1] or NaN. */
int mq_soft_update(float* target, const float* online, int64_t n, float one_minus_tau, float tau, void* stream);

/* Reward standardisation with running statistics, an opt-in (epymarl's standardise_rewards). state: three device
 * doubles [mean, var, count], initialised by the caller (epymarl: 0, 1, 1e-4), borrowed like mq_bind's pointers;
 * sticky until mq_set_reward_norm(h, NULL) turns it off. Every mq_forward_backward / mq_train_step then begins its
 * mixer tail with one launch of one workgroup over x = reward[:, :-1] of the batch (M = batch_size * (t_len - 1) values
 * gathered by episode id, UNMASKED: padded steps count with the storage's zeros, duplicate ids count twice):
 *   bm = mean(x);  bv = sum (x - bm)^2 / (M - 1)   (M = 1: 0, where torch's unbiased variance is NaN)
 *   delta = bm - mean;  tot = count + M
 *   mean = mean + delta * M / tot;  var = (var * count + bv * M + delta^2 * count * M / tot) / tot;  count = tot
 * all in fp64, fixed summation order; then, with the UPDATED statistics each rounded to fp32 once,
 *   r_std = (r - mean) / sqrtf(var)                 (fp32, no epsilon)
 * which the step reads wherever it read the reward: the one-step target, the TD(lambda) scan, their PER and Huber
 * forms. stats[4] (target_mean) is then on the standardised scale. Nothing is read back to the host.
 * MQ_ERR_ARG: NULL handle, a state pointer not aligned to a double; at the step: a communicator attached or data
 * parallelism set (each rank would standardise with its own shard's rewards).
 * mq_last_reward_norm: 1 / 0 whether the last mq_forward_backward standardised; -1 for a NULL handle or when none
 * has run. Like mq_last_hyper_layers these are entries of their own: mq_plan keeps its size. */
int mq_set_reward_norm(mq_handle* h, double* state /* device, [mean, var, count] */);
int32_t mq_last_reward_norm(const mq_handle* h);

/* Prioritized episode replay (PER), an opt-in the reference lacks. Priorities live on the device and never reach the
 * host: mq_per_sample draws, the next train step weights its loss and writes the new priorities back.
 *
 * mq_per_sample: stratified draw of `batch` episodes (duplicates allowed) from slots [0, n_live) of prio (raw
 * priorities, > 0), u[batch] uniform in [0, 1), all fp32:
 *   q_i = prio_i^alpha (alpha == 1: prio_i), cum = inclusive scan of q, total = cum[n_live - 1]
 *   tau_b = ((float)b + u[b]) * (total / (float)batch);  ids[b] = the first i with cum[i] > tau_b, at most n_live - 1
 *   weights[b] = (n_live * q_ids[b] / total)^(-beta), divided by their maximum (beta == 0: exactly 1)
 * One launch on `stream`; ids int64 [batch] and weights [batch] are device outputs. MQ_ERR_ARG: alpha < 0 or NaN,
 * beta outside [0, 1], n_live < 1 or > MQ_PER_MAX_LIVE, batch < 1, a NULL pointer. */
enum { MQ_PER_MAX_LIVE = 32768 };
int mq_per_sample(const float* prio, int32_t n_live, const float* u, int32_t batch, float alpha, float beta,
                  int64_t* ids, float* weights, void* stream);
/* Arm the NEXT mq_forward_backward / mq_train_step as a PER step; that step disarms it again, and so does a NULL
 * `per` (never sticky). The step's batch must carry device episode ids (mq_replay.ep_ids, ep_ids_host NULL): they
 * are the slots of prio it writes. The PER step:
 *   loss = sum_b weights[b] sum_t loss(td * mask) / sum mask (stats[0]; the other stats stay unweighted), dy of every
 *   row times its weights[b];
 *   afterwards prio[ids[b]] = sum_t |td * mask| / max(sum_t mask, 1) + eps (no mixer: the agents' sum over
 *   n_agents * sum_t mask), and *prio_max = max(*prio_max, those).
 * weights [batch_size], prio [n_prio], prio_max [1]: device pointers, borrowed until that step has been queued.
 * MQ_ERR_ARG: eps <= 0 or NaN, n_prio < 1, a NULL pointer; at the step: a communicator attached or data parallelism
 * set (not supported), or a batch without device ids. */
typedef struct mq_per { const float* weights; float* prio; float* prio_max; int64_t n_prio; float eps; } mq_per;
int mq_set_per(mq_handle* h, const mq_per* per);

/* Copy an intermediate of the last mq_forward_backward into dst (device): 0 = online mac_out [t][b*n+a][A],
 * 1 = target mac_out (same layout), 2 = dQ/dchosen [t][b*n+a] (unnormalised), 3 = online relu(fc1) activations
 * [t][b*n+a][64]. Returns element count in *count.
 * After a step that ran the TD(lambda) passes (mq_plan.td_lambda = 1; MQ_ERR_STATE otherwise): 4 = y', the target
 * network's mixed value at step t + 1, as [t][b] (no mixer: [t][b*n+a], one value per agent), t < t_len - 1;
 * 5 = the lambda targets in the same layout.
 * After a prioritized-replay step (mq_plan.per = 1; MQ_ERR_STATE otherwise): 6 = |td * mask| of every transition,
 * unweighted, as [t][b] (no mixer: summed over the agents), t < t_len - 1: what the priority write-back summed.
 * After a step of the two-layer hypernet (mq_last_hyper_layers = 2; MQ_ERR_STATE otherwise): 7 = the online net's
 * first-layer pre-activations [hyper_w_1.0 | hyper_w_final.0] as [t][b][2 * hypernet_embed], t < t_len - 1.
 * After a step that standardised its rewards (mq_last_reward_norm = 1; MQ_ERR_STATE otherwise): 8 = the standardised
 * rewards the step read, as [t][b], t < t_len - 1.
 * After a step of the feed-forward agent (mq_last_agent bit 0; MQ_ERR_STATE otherwise): 9 = the online net's
 * h = relu(rnn(x1)) as [t][b*n+a][64]. */
int mq_copy_intermediate(mq_handle* h, int which, float* dst, int64_t* count, void* stream);

/* BasicMAC.forward(ep_batch, t) for every episode of `batch`: h_in/h_out [batch*n][64] (h_in may equal
 * h_out), q_out [batch*n][n_actions]; which = 0 online params, 1 target params (MQ_ERR_STATE when none are bound).
 * MQ_ERR_ARG as mq_train_step gives it: a host id (ep_ids_host) outside [0, n_episodes), or a batch without ids
 * whose batch_size exceeds n_episodes.
 * On a feed-forward handle (MQ_AGENT_FFN) this and mq_agent_forward run the three layers in one launch, write
 * h = relu(rnn(x1)) to h_out and never read h_in, which may be NULL. */
int mq_mac_forward(mq_handle* h, const mq_replay* batch, int32_t t, const float* h_in, float* h_out,
                   float* q_out, int32_t which, void* stream);
/* RNNAgent.forward(inputs, hidden) (rnn_agent.py:27-36) on given inputs [rows][input_dim]. */
int mq_agent_forward(mq_handle* h, const float* inputs, int32_t rows, const float* h_in, float* h_out,
                     float* q_out, int32_t which, void* stream);
/* argmax over available actions (avail != 0; unavailable = -inf, first index on ties) of q [rows][n_actions], as
 * torch's max(dim) takes it: a NaN at an available action is the maximum (the first such index); a NaN at an
 * unavailable action is masked; a row with no available action gives 0. */
int mq_greedy_actions(const float* q, const int32_t* avail, int64_t* out, int32_t rows, int32_t n_actions,
                      void* stream);

/* QMixer.forward(agent_qs, states) outside train(): mixer = the mixer's parameters in QMixer.parameters() order
 * (hyper_w_1.weight .. V.2.bias, the MQ_P_HW1_W .. MQ_P_V2_B block), agent_qs [rows][n_agents], states
 * [rows][state_dim], q_tot [rows]. n_agents and embed_dim in [1, 64]; MQ_ERR_ARG when the LDS staging of four rows,
 * 16 (state_dim + embed_dim (n_agents + 3)) bytes, passes the 160 KB of a CU. */
int mq_qmix_forward(const float* mixer, int32_t n_agents, int32_t state_dim, int32_t embed_dim,
                    const float* agent_qs, const float* states, float* q_tot, int32_t rows, void* stream);
/* The same for a two-layer QMixer (hypernet_layers = 2): mixer = its parameters in parameters() order
 * (hyper_w_1.0.weight .. V.2.bias, see MQ_P_*), hypernet_embed in 1 .. MQ_HYPERNET_EMBED_MAX. */
int mq_qmix_forward2(const float* mixer, int32_t n_agents, int32_t state_dim, int32_t embed_dim,
                     int32_t hypernet_embed, const float* agent_qs, const float* states, float* q_tot, int32_t rows,
                     void* stream);

/* Which kernel variants the last mq_forward_backward launched (test / profiling introspection; no device sync).
 * rw_fwd / rw_bwd: rows per workgroup of the unfused recurrences (0 when the fused kernel ran). */
enum { MQ_HYP_NONE = 0, MQ_HYP_WS = 1, MQ_HYP_LDS = 2, MQ_HYP_GEMM = 3 };
enum { MQ_MIX_FAST16 = 0, MQ_MIX_FAST32 = 1, MQ_MIX_GENERIC = 2, MQ_MIX_STREAM = 3 };
typedef struct mq_plan {
  int32_t rows;          /* R = batch_size * n_agents */
  int32_t fused_fwd;     /* gru_fwd_fused_kernel (1), gru_fwd_pair_kernel (2) or fc1 / gi / gru_fwd<rw_fwd> / fc2 (0) */
  int32_t rw_fwd;
  int32_t fused_bwd;     /* gru_bwd_fused_kernel (1) or gru_bwd<rw_bwd> / dx1 / dw1 (0) */
  int32_t rw_bwd;
  int32_t inline_ids;    /* episode ids in the kernel arguments (1) or read from mq_replay.ep_ids (0) */
  int32_t hyper;         /* MQ_HYP_* */
  int32_t mix;           /* MQ_MIX_* */
  int32_t tiles;         /* 1: the row-tile MFMA forward / BPTT of large batches (gru_fwd_tile / gru_bwd_tile);
                            fused_fwd / fused_bwd / rw_* are then 0 */
  int32_t dwh;           /* QMIX dW_hyper: beside reduction pass 1 (0) or appended to the fused BPTT's grid (1) */
  int32_t td_lambda;     /* 1: the mixer tail ran as the TD(lambda) passes (mq_config.td_lambda > 0, or MQ_PLAN
                            lambda_path=1, which runs them at td_lambda = 0 too: the one-step target through the scan,
                            for A/B runs and tests); `mix` names the variant of both mixer passes */
  int32_t bwd_lean;      /* 1: the fused BPTT ran its lean per-step path (walked chain addresses, per-chunk fc2-gradient
                            inputs, dW2 / db2 in registers): the default behind the row-pair forward (fused_fwd = 2,
                            fused_bwd = 1); MQ_PLAN bwd_lean=0 keeps the classic step (bitwise the same results) */
  int32_t per;           /* 1: a prioritized-replay step (mq_set_per): the loss-bearing mixer pass ran in its PER form
                            and the priority write-back followed it */
} mq_plan;
int mq_last_plan(const mq_handle* h, mq_plan* out);
/* The hypernet of the last mq_forward_backward, the plan item `hyper_layers`. mq_plan itself keeps its size and `per`
 * as its last field (hosts built against it stay valid), so the item has an entry of its own. 2: the two-layer QMIX
 * hypernet ran, as launches of its own around the mixer tail (layer 1, layer 2 forward; layer 2 backward, weight
 * gradients); mq_plan.hyper then names layer 1's kernel and mq_plan.dwh is 0. 1: the one-layer hypernet. 0: no QMIX
 * mixer. -1: NULL handle, or no forward/backward has run. */
int32_t mq_last_hyper_layers(const mq_handle* h);
/* The agent of the last mq_forward_backward, an entry of its own like mq_last_hyper_layers (mq_plan keeps its size).
 * -1: NULL handle, or no forward/backward has run. 0: the GRU agent ran. Otherwise a bit set: bit 0 = the feed-forward
 * agent ran (fc1 / rnn / fc2 as GEMMs forward; dP2 and the fc2 gradients, then dP1, [dW_rnn | db_rnn] and dW1 as GEMMs
 * backward: ffn_kernels.hpp); bits 1 and 2 are reserved for a fused forward / backward kernel (never set by this
 * library). After such a step mq_plan.fused_fwd, rw_fwd, fused_bwd, rw_bwd, tiles, bwd_lean and dwh are all 0. */
int32_t mq_last_agent(const mq_handle* h);

/* Optional per-kernel HIP-event timing of train steps (bench / profiling): events bracket every phase whose bit
 * is set in phase_mask (bit i = phase i of mq_phase_names), in a ring of `slots` steps; slots = 0 turns it off. */
int mq_set_timing(mq_handle* h, int32_t slots, uint32_t phase_mask);
/* Mean ms per phase over the recorded steps (synchronises on the events); *n = number of phases. */
int mq_phase_times(mq_handle* h, float* ms, int32_t cap, int32_t* n);
const char* mq_phase_names(void);

#ifdef __cplusplus
}
#endif
#endif /* MQ_LEARNER_H */
