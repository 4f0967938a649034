/* C ABI of the MI355X-native actor-critic learner step (libmq_learner.so, gfx950): epymarl's actor_critic_learner
 * (configs maa2c.yaml / ia2c.yaml) as DESIGN.md §3k specifies it.
 *
 * The boundary behind learners.REGISTRY["actor_critic_learner"]: pymarl_amd/learners/actor_critic_learner.py binds
 * these symbols with ctypes. Conventions as include/mc_coma.h: DEVICE pointers owned by the caller, asynchronous on
 * the given HIP stream, int status + mq_last_error().
 *
 * The critic is a V network, fc1 (K -> Hc) relu fc2 (Hc -> Hc) relu fc3 (Hc -> 1), trained in ONE optimiser step over
 * every t of the batch against n-step returns of the target critic; the actor is the GRU agent with a softmax policy
 * (no epsilon floor), trained with the advantage td = (return - V) mask and an entropy bonus. Both optimisers are
 * RMSprop (the reference's) or, after ma_set_adam, torch.optim.Adam.
 */
#ifndef MA_A2C_H
#define MA_A2C_H

#include "mq_learner.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-row critic input. CV (cv_critic): state | last joint one-hot actions of all agents (obs_last_action only; zero
 * at t = 0 and behind unfilled slots) | one-hot agent id. AC (ac_critic): the row's own obs | one-hot agent id. */
enum { MA_CRITIC_CV = 0, MA_CRITIC_AC = 1 };
/* Critic parameter tensors in parameters() order. */
enum { MA_P_FC1_W, MA_P_FC1_B, MA_P_FC2_W, MA_P_FC2_B, MA_P_FC3_W, MA_P_FC3_B, MA_P_COUNT };
enum { MA_NTAIL = 8 };   /* tail of the critic gradient buffer: the step's loss sums ([1] = mask elements M) */
/* stats[MA_NSTATS]: [0] critic_loss, [1] critic_grad_norm, [2] td_error_abs, [3] q_taken_mean, [4] target_mean,
 * [5] mask elements M = n_agents * sum(mask) (0: the batch was empty and nothing was applied), [6] critic clip
 * coefficient; [8] pg_loss, [9] agent_grad_norm, [10] advantage_mean, [11] pi_max, [12] entropy mean, [13] M,
 * [14] agent clip coefficient. */
enum { MA_NSTATS = 16 };

typedef struct ma_config {
  int32_t n_agents, n_actions, obs_dim, state_dim;
  int32_t rnn_hidden_dim;          /* 64 */
  int32_t critic_hidden;           /* 64 or 128 */
  int32_t critic_type;             /* MA_CRITIC_* */
  int32_t obs_last_action, obs_agent_id;
  int32_t mask_before_softmax;
  int32_t q_nstep;                 /* >= 1 */
  int32_t add_value_last_step;
  float entropy_coef;              /* >= 0 */
  float lr, optim_alpha, optim_eps, grad_norm_clip;   /* one lr for both optimisers */
  const float* gamma_pow;          /* HOST pointer, q_nstep + 2 floats: g[k] = float32(gamma ** k); ma_create copies it */
  int32_t max_batch, max_seq;
} ma_config;

/* Adam in RMSprop's place for both optimisers: the first-moment buffers [Pa] / [Pc] (the second moments live where
 * RMSprop's square_avg does: agent_sq / critic_sq of ma_bind). NULL switches back to RMSprop. */
typedef struct ma_adam {
  float* agent_exp_avg;
  float* critic_exp_avg;
  float beta1, beta2, eps, weight_decay;
} ma_adam;

/* PPO (epymarl's ppo_learner) in the one-step actor-critic's place: ma_train_step runs `epochs`
 * optimisation epochs over the batch, each one critic step and one actor step on the clipped surrogate
 * min(ratio adv, clamp(ratio, lo, hi) adv), ratio = exp(log pi_u - old), old = epoch 0's own log pi_u,
 * lo = (float)(1.0 - (double)eps_clip), hi = (float)(1.0 + (double)eps_clip). The returns, the standardised rewards
 * and the running reward statistics are formed once per step. epoch_stats: DEVICE memory [epochs][MA_NSTATS], row k
 * = stats as epoch k's applies left it, with the number of live rows whose surrogate gradient was cut at [15]. */
typedef struct ma_ppo {
  int32_t epochs;       /* >= 1 */
  float eps_clip;       /* 0 < eps_clip < 1 */
  float* epoch_stats;
} ma_ppo;

/* What the last ma_train_step launched (host tests read the edges off it). */
typedef struct ma_plan {
  int32_t rows;           /* T * B * n: the online critic's and the actor's rows */
  int32_t rows_target;    /* (T + 1) * B * n: the target critic's rows */
  int32_t k, kp;          /* critic input width and its padded pitch (multiple of 4) */
  int32_t hidden;         /* critic hidden width */
  int32_t vec16;          /* 1: the critic GEMMs read X and W1 with 16-byte loads (k % 4 == 0 for W1's part) */
  int32_t fwd_tiles;      /* 64-row tiles of the two-net forward GEMMs (grid.x) */
  int32_t vhead_blocks;   /* a2c_vhead_kernel: 4 rows (waves) per block over rows_target + rows */
  int32_t nstep_lds;      /* a2c_nstep_kernel's dynamic LDS, bytes */
  int32_t dv_blocks;      /* a2c_dv_kernel's workgroups = fc3 gradient slabs */
  int32_t ns_cw2, ns_cw1; /* split-K slices of the critic's [dW2 | db2] and [dW1 | db1] */
  int32_t policy_blocks;  /* a2c_policy_kernel: 4 rows (waves) per block */
  int32_t policy_tail;    /* rows % 4: live waves of its last block (0: full) */
  int32_t policy_lanes;   /* n_actions: the live lanes of each of its waves (of 64) */
  int32_t ap;             /* dlogits' row pitch: n_actions rounded up to 4 (pad columns written as zeros) */
  int32_t ns_aw1, ns_aw2; /* split-K slices of the agent's dW1 and dW2 */
  int32_t bwd_blocks;     /* the BPTT's workgroups */
  int32_t reward_norm;    /* 1: the step standardised its rewards */
  int32_t adam;           /* 1: Adam applied, 0: RMSprop */
  int32_t epochs;         /* optimisation epochs the step ran: 1, or ma_ppo.epochs */
  int32_t hoisted;        /* PPO: launches and copies made once per step, not once per epoch (0: not a PPO step) */
} ma_plan;

typedef struct ma_handle ma_handle;

int ma_create(const ma_config* cfg, ma_handle** out);
int ma_destroy(ma_handle* h);
/* agent_offsets[MQ_P_COUNT + 1] (RNNAgent layout, mixer entries empty), critic_offsets[MA_P_COUNT + 1]. */
int ma_param_offsets(const ma_handle* h, int64_t* agent_offsets, int64_t* critic_offsets);
/* agent / agent_sq: [Pa]; agent_grad: [Pa + MQ_NSUMS]; critic / target_critic / critic_sq: [Pc];
 * critic_grad: [Pc + MA_NTAIL]; stats: [MA_NSTATS]. Both clipped gradients are left in the grad buffers. */
int ma_bind(ma_handle* h, float* agent, float* agent_grad, float* agent_sq, float* critic, float* target_critic,
            float* critic_grad, float* critic_sq, float* stats);
int ma_set_adam(ma_handle* h, const ma_adam* a);
/* Running reward statistics [mean, var, count] (three device doubles, mq_set_reward_norm's semantics); NULL: off. */
int ma_set_reward_norm(ma_handle* h, double* state);
/* NULL switches back to the one-step actor-critic. Arguments are checked before any HIP call (MQ_ERR_ARG). */
int ma_set_ppo(ma_handle* h, const ma_ppo* p);
/* One train() on `batch` (t_len = max_t_filled). adam_step: the 1-based number of the Adam step this call applies
 * (ignored under RMSprop); the caller counts it, because a batch whose mask is empty applies nothing: it leaves every
 * bound buffer but stats untouched and writes stats[5] = 0, which the caller reads. After ma_set_ppo the call applies
 * `epochs` steps numbered adam_step, adam_step + 1, ..; an empty batch applies none of them and every row of
 * epoch_stats is zero. */
int ma_train_step(ma_handle* h, const mq_replay* batch, int64_t adam_step, void* stream);
/* target_critic <- critic (tau = 0 or tau >= 1 ... a hard copy), or target = target (1 - tau) + critic tau for
 * 0 < tau < 1 (soft_update_kernel). */
int ma_update_targets(ma_handle* h, double tau, void* stream);
/* The critic module's forward(batch, t) outside train(): critic = fc1.weight .. fc3.bias; t < 0: every stored step,
 * else step t. v_out [batch_size][Tq][n_agents][1], Tq = t_len or 1; workspace:
 * ma_critic_forward_workspace(cfg, batch_size, Tq) floats of device memory. cfg->gamma_pow is not read. */
int64_t ma_critic_forward_workspace(const ma_config* cfg, int32_t batch_size, int32_t t_count);
int ma_critic_forward(const float* critic, const ma_config* cfg, const mq_replay* batch, int32_t t, float* v_out,
                      float* workspace, void* stream);
/* 0 = V' (target critic) [T + 1][B*n]; 1 = V [T][B*n]; 2 = n-step returns [T][B*n]; 3 = pi [T][B*n][A];
 * 4 = dLoss/dlogits before the 1 / M scale [T * B*n][Ap], Ap = n_actions rounded up to 4 (pad columns zero).
 * After a PPO step 1, 3 and 4 hold the last epoch's values, and 5 = old, epoch 0's log pi_u [T][B*n];
 * 6 = the last epoch's ratio [T][B*n]. */
int ma_copy_intermediate(ma_handle* h, int which, float* dst, int64_t* count, void* stream);
int ma_last_plan(const ma_handle* h, ma_plan* out);

#ifdef __cplusplus
}
#endif
#endif /* MA_A2C_H */
