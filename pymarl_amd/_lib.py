"""ctypes binding of libmq_learner.so (the C ABI declared in include/mq_learner.h).

The product path has no fallback: if the library is missing, or the device is not a HIP GPU, the learner fails
loudly here. Build it with `python __graft_entry__.py build` (or `make -C pymarl_amd/csrc`).
"""
from __future__ import annotations

import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MQ_LEARNER_LIB", os.path.join(HERE, "lib", "libmq_learner.so"))

MIXER_NONE, MIXER_VDN, MIXER_QMIX = 0, 1, 2
AGENT_GRU, AGENT_FFN = 0, 1   # MQ_AGENT_*
NSUMS = 8
NSTATS = 8
PARAM_NAMES = [
    "fc1.weight", "fc1.bias", "rnn.weight_ih", "rnn.weight_hh", "rnn.bias_ih", "rnn.bias_hh", "fc2.weight",
    "fc2.bias", "hyper_w_1.weight", "hyper_w_1.bias", "hyper_w_final.weight", "hyper_w_final.bias",
    "hyper_b_1.weight", "hyper_b_1.bias", "V.0.weight", "V.0.bias", "V.2.weight", "V.2.bias",
    # two-layer hypernet only (hypernet_layers: 2): the entries above then name hyper_w_1.0 / hyper_w_final.0
    "hyper_w_1.2.weight", "hyper_w_1.2.bias", "hyper_w_final.2.weight", "hyper_w_final.2.bias",
    # feed-forward agent only (use_rnn: False): the four rnn.* entries above are then empty
    "rnn.weight", "rnn.bias",
]
P_COUNT = len(PARAM_NAMES)

# Every symbol include/mq_learner.h declares (checked by tests/test_boundary.py).
EXPORTS = [
    "mq_last_error", "mq_create", "mq_destroy", "mq_param_offsets", "mq_bind", "mq_forward_backward", "mq_apply",
    "mq_train_step", "mq_update_targets", "mq_copy_intermediate", "mq_mac_forward", "mq_agent_forward",
    "mq_greedy_actions", "mq_set_timing", "mq_phase_times", "mq_phase_names", "mq_set_data_parallel",
    "mq_last_plan", "mq_qmix_forward", "mq_qmix_forward2", "mq_last_hyper_layers", "mq_per_sample", "mq_set_per",
    "mq_set_adam", "mq_opt_step", "mq_adam_update", "mq_set_soft_target", "mq_last_soft_target", "mq_soft_update",
    "mq_set_reward_norm", "mq_last_reward_norm", "mq_last_agent",
    # include/mc_coma.h
    "mc_create", "mc_destroy", "mc_param_offsets", "mc_bind", "mc_train_step", "mc_update_targets", "mc_policy",
    "mc_copy_intermediate", "mc_set_timing", "mc_phase_times", "mc_last_critic_path", "mq_comm_unique_id", "mq_comm_attach",
    "mq_comm_world", "mq_comm_detach", "mc_comm_attach", "mc_set_data_parallel", "mc_critic_forward",
    "mc_critic_forward_workspace", "mc_set_actor_shard", "mq_comm_use", "mq_comm_create", "mq_comm_free",
    "mc_comm_use", "mc_comm_detach",
]

# Every symbol include/ma_a2c.h declares (the actor-critic learner; __graft_entry__.build() checks them too).
MA_EXPORTS = [
    "ma_create", "ma_destroy", "ma_param_offsets", "ma_bind", "ma_set_adam", "ma_set_reward_norm", "ma_train_step",
    "ma_update_targets", "ma_critic_forward_workspace", "ma_critic_forward", "ma_copy_intermediate", "ma_last_plan",
    "ma_set_ppo",
]

# mc_allreduce_fn (include/mc_coma.h): int (*)(float* buf, int64_t count, void* stream, void* ctx)
MC_ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p)

MC_P_COUNT = 6
MC_NTAIL = 8
MC_NSTATS = 16
COMA_STATS = ["critic_loss", "critic_grad_norm", "td_error_abs", "q_taken_mean", "target_mean", "advantage_mean",
              "coma_loss", "agent_grad_norm", "pi_max", "critic_steps", "mask_sum"]


class MQConfig(ctypes.Structure):
    _fields_ = [
        ("n_agents", ctypes.c_int32), ("n_actions", ctypes.c_int32), ("obs_dim", ctypes.c_int32),
        ("state_dim", ctypes.c_int32), ("rnn_hidden_dim", ctypes.c_int32), ("mixing_embed_dim", ctypes.c_int32),
        ("mixer", ctypes.c_int32), ("double_q", ctypes.c_int32), ("obs_last_action", ctypes.c_int32),
        ("obs_agent_id", ctypes.c_int32), ("gamma", ctypes.c_float), ("lr", ctypes.c_float),
        ("optim_alpha", ctypes.c_float), ("optim_eps", ctypes.c_float), ("grad_norm_clip", ctypes.c_float),
        ("max_batch", ctypes.c_int32), ("max_seq", ctypes.c_int32), ("huber_delta", ctypes.c_float),
        ("td_lambda", ctypes.c_float), ("hypernet_layers", ctypes.c_int32), ("hypernet_embed", ctypes.c_int32),
        ("agent", ctypes.c_int32),
    ]


HYPERNET_EMBED_MAX = 64   # MQ_HYPERNET_EMBED_MAX


class MQReplay(ctypes.Structure):
    _fields_ = [
        ("obs", ctypes.c_void_p), ("state", ctypes.c_void_p), ("actions", ctypes.c_void_p),
        ("avail_actions", ctypes.c_void_p), ("reward", ctypes.c_void_p), ("terminated", ctypes.c_void_p),
        ("filled", ctypes.c_void_p), ("ep_ids", ctypes.c_void_p), ("n_episodes", ctypes.c_int64),
        ("batch_size", ctypes.c_int32), ("t_len", ctypes.c_int32), ("t_stride", ctypes.c_int32),
        ("ep_ids_host", ctypes.c_void_p), ("avail_bits", ctypes.c_void_p),
    ]


class MCConfig(ctypes.Structure):
    _fields_ = [
        ("n_agents", ctypes.c_int32), ("n_actions", ctypes.c_int32), ("obs_dim", ctypes.c_int32),
        ("state_dim", ctypes.c_int32), ("rnn_hidden_dim", ctypes.c_int32), ("obs_last_action", ctypes.c_int32),
        ("obs_agent_id", ctypes.c_int32), ("mask_before_softmax", ctypes.c_int32), ("gamma", ctypes.c_float),
        ("td_lambda", ctypes.c_float), ("lr", ctypes.c_float), ("critic_lr", ctypes.c_float),
        ("optim_alpha", ctypes.c_float), ("optim_eps", ctypes.c_float), ("grad_norm_clip", ctypes.c_float),
        ("max_batch", ctypes.c_int32), ("max_seq", ctypes.c_int32),
    ]


MA_CRITIC_CV, MA_CRITIC_AC = 0, 1   # MA_CRITIC_*
MA_P_COUNT = 6
MA_NTAIL = 8
MA_NSTATS = 16
MA_CRITIC_PARAMS = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias"]
# where ma_train_step leaves each logged stat in stats[MA_NSTATS] (include/ma_a2c.h)
A2C_STATS = {"critic_loss": 0, "critic_grad_norm": 1, "td_error_abs": 2, "q_taken_mean": 3, "target_mean": 4,
             "advantage_mean": 10, "pg_loss": 8, "agent_grad_norm": 9, "pi_max": 11}
A2C_MASK_ELEMS = 5   # stats[5]: M = n_agents * sum(mask); 0 after a batch whose mask was empty


class MAConfig(ctypes.Structure):
    _fields_ = [
        ("n_agents", ctypes.c_int32), ("n_actions", ctypes.c_int32), ("obs_dim", ctypes.c_int32),
        ("state_dim", ctypes.c_int32), ("rnn_hidden_dim", ctypes.c_int32), ("critic_hidden", ctypes.c_int32),
        ("critic_type", ctypes.c_int32), ("obs_last_action", ctypes.c_int32), ("obs_agent_id", ctypes.c_int32),
        ("mask_before_softmax", ctypes.c_int32), ("q_nstep", ctypes.c_int32), ("add_value_last_step", ctypes.c_int32),
        ("entropy_coef", ctypes.c_float), ("lr", ctypes.c_float), ("optim_alpha", ctypes.c_float),
        ("optim_eps", ctypes.c_float), ("grad_norm_clip", ctypes.c_float), ("gamma_pow", ctypes.c_void_p),
        ("max_batch", ctypes.c_int32), ("max_seq", ctypes.c_int32),
    ]


class MAAdam(ctypes.Structure):
    """ma_adam: both optimisers' first-moment buffers (device pointers) and Adam's hyper-parameters."""
    _fields_ = [("agent_exp_avg", ctypes.c_void_p), ("critic_exp_avg", ctypes.c_void_p), ("beta1", ctypes.c_float),
                ("beta2", ctypes.c_float), ("eps", ctypes.c_float), ("weight_decay", ctypes.c_float)]


class MAPpo(ctypes.Structure):
    """ma_ppo: the PPO step's epochs and clip range, and the device buffer [epochs][MA_NSTATS] of per-epoch stats."""
    _fields_ = [("epochs", ctypes.c_int32), ("eps_clip", ctypes.c_float), ("epoch_stats", ctypes.c_void_p)]


PPO_STAT_CLIPPED = 15   # epoch_stats[k][15]: live rows whose surrogate gradient epoch k cut


class MAPlan(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in (
        "rows", "rows_target", "k", "kp", "hidden", "vec16", "fwd_tiles", "vhead_blocks", "nstep_lds", "dv_blocks",
        "ns_cw2", "ns_cw1", "policy_blocks", "policy_tail", "policy_lanes", "ap", "ns_aw1", "ns_aw2", "bwd_blocks", "reward_norm", "adam",
        "epochs", "hoisted")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class MQPlan(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("rows", "fused_fwd", "rw_fwd", "fused_bwd", "rw_bwd", "inline_ids",
                                               "hyper", "mix", "tiles", "dwh", "td_lambda", "bwd_lean", "per")]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class MQPer(ctypes.Structure):
    """mq_per: one prioritized-replay step's weights and the priority storage it writes (device pointers)."""
    _fields_ = [("weights", ctypes.c_void_p), ("prio", ctypes.c_void_p), ("prio_max", ctypes.c_void_p),
                ("n_prio", ctypes.c_int64), ("eps", ctypes.c_float)]


class MQAdam(ctypes.Structure):
    """mq_adam: the Adam opt-in's first-moment buffer (device pointer), hyper-parameters and steps already applied."""
    _fields_ = [("exp_avg", ctypes.c_void_p), ("beta1", ctypes.c_float), ("beta2", ctypes.c_float),
                ("eps", ctypes.c_float), ("weight_decay", ctypes.c_float), ("step", ctypes.c_int64)]


PER_MAX_LIVE = 32768   # MQ_PER_MAX_LIVE: live episodes one mq_per_sample draw supports


HYP_NAMES = {0: "none", 1: "ws", 2: "lds", 3: "gemm"}
MIX_NAMES = {0: "fast16", 1: "fast32", 2: "generic", 3: "stream"}

INLINE_IDS = 256   # MQ_INLINE_IDS: batches up to this size pass their episode ids in the kernel arguments
COMM_ID_BYTES = 128   # MQ_COMM_ID_BYTES (ncclUniqueId)


_LIB = None


class MQError(RuntimeError):
    pass


def load(required=True):
    """Load the shared library once; raise MQError (no fallback) if it cannot be loaded."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        if not required:
            return None
        raise MQError(f"libmq_learner.so not found at {LIB_PATH}; build it with `python __graft_entry__.py build`")
    import torch  # noqa: F401  (loads torch's HIP runtime first so the library binds to the same one)
    lib = ctypes.CDLL(LIB_PATH)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    sig = {
        "mq_last_error": ([], ctypes.c_char_p),
        "mq_phase_names": ([], ctypes.c_char_p),
        "mq_create": ([ctypes.POINTER(MQConfig), ctypes.POINTER(vp)], ctypes.c_int),
        "mq_destroy": ([vp], ctypes.c_int),
        "mq_param_offsets": ([vp, ctypes.POINTER(i64)], ctypes.c_int),
        "mq_bind": ([vp, vp, vp, vp, vp, vp, vp], ctypes.c_int),
        "mq_forward_backward": ([vp, ctypes.POINTER(MQReplay), vp], ctypes.c_int),
        "mq_apply": ([vp, vp], ctypes.c_int),
        "mq_train_step": ([vp, ctypes.POINTER(MQReplay), vp], ctypes.c_int),
        "mq_update_targets": ([vp, vp], ctypes.c_int),
        "mq_copy_intermediate": ([vp, ctypes.c_int, vp, ctypes.POINTER(i64), vp], ctypes.c_int),
        "mq_mac_forward": ([vp, ctypes.POINTER(MQReplay), i32, vp, vp, vp, i32, vp], ctypes.c_int),
        "mq_agent_forward": ([vp, vp, i32, vp, vp, vp, i32, vp], ctypes.c_int),
        "mq_greedy_actions": ([vp, vp, vp, i32, i32, vp], ctypes.c_int),
        "mq_set_timing": ([vp, i32, ctypes.c_uint32], ctypes.c_int),
        "mq_set_data_parallel": ([vp, i32], ctypes.c_int),
        "mq_last_plan": ([vp, ctypes.POINTER(MQPlan)], ctypes.c_int),
        "mq_qmix_forward": ([vp, i32, i32, i32, vp, vp, vp, i32, vp], ctypes.c_int),
        "mq_last_hyper_layers": ([vp], i32),
        "mq_qmix_forward2": ([vp, i32, i32, i32, i32, vp, vp, vp, i32, vp], ctypes.c_int),
        "mq_per_sample": ([vp, i32, vp, i32, ctypes.c_float, ctypes.c_float, vp, vp, vp], ctypes.c_int),
        "mq_set_per": ([vp, ctypes.POINTER(MQPer)], ctypes.c_int),
        "mq_set_adam": ([vp, ctypes.POINTER(MQAdam)], ctypes.c_int),
        "mq_opt_step": ([vp], i64),
        "mq_adam_update": ([vp, vp, vp, vp, i64] + [ctypes.c_float] * 5 + [i64, vp], ctypes.c_int),
        "mq_set_soft_target": ([vp, ctypes.c_double], ctypes.c_int),
        "mq_last_soft_target": ([vp], i32),
        "mq_soft_update": ([vp, vp, i64, ctypes.c_float, ctypes.c_float, vp], ctypes.c_int),
        "mq_set_reward_norm": ([vp, vp], ctypes.c_int),
        "mq_last_reward_norm": ([vp], i32),
        "mq_last_agent": ([vp], i32),
        "mc_critic_forward_workspace": ([ctypes.POINTER(MCConfig), i32, i32], i64),
        "mc_critic_forward": ([vp, ctypes.POINTER(MCConfig), ctypes.POINTER(MQReplay), i32, vp, vp, vp], ctypes.c_int),
        "mq_phase_times": ([vp, ctypes.POINTER(ctypes.c_float), i32, ctypes.POINTER(i32)], ctypes.c_int),
        "mc_create": ([ctypes.POINTER(MCConfig), ctypes.POINTER(vp)], ctypes.c_int),
        "mc_destroy": ([vp], ctypes.c_int),
        "mc_param_offsets": ([vp, ctypes.POINTER(i64), ctypes.POINTER(i64)], ctypes.c_int),
        "mc_bind": ([vp, vp, vp, vp, vp, vp, vp, vp, vp], ctypes.c_int),
        "mc_train_step": ([vp, ctypes.POINTER(MQReplay), ctypes.c_float, vp], ctypes.c_int),
        "mc_update_targets": ([vp, vp], ctypes.c_int),
        "mc_policy": ([vp, vp, i32, i32, ctypes.c_float, i32, i32, vp], ctypes.c_int),
        "mc_copy_intermediate": ([vp, ctypes.c_int, vp, ctypes.POINTER(i64), vp], ctypes.c_int),
        "mc_set_timing": ([vp, i32], ctypes.c_int),
        "mc_phase_times": ([vp, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
        "mc_last_critic_path": ([vp], i32),
        "mq_comm_unique_id": ([vp], ctypes.c_int),
        "mq_comm_attach": ([vp, vp, i32, i32], ctypes.c_int),
        "mq_comm_world": ([vp], i32),
        "mq_comm_detach": ([vp], ctypes.c_int),
        "mc_comm_attach": ([vp, vp, i32, i32], ctypes.c_int),
        "mc_set_data_parallel": ([vp, MC_ALLREDUCE_FN, vp, i32, vp, i64], ctypes.c_int),
        "mc_set_actor_shard": ([vp, i32, i32], ctypes.c_int),
        "mq_comm_use": ([vp, vp], ctypes.c_int),
        "mq_comm_create": ([vp, i32, i32, ctypes.POINTER(vp)], ctypes.c_int),
        "mq_comm_free": ([vp], ctypes.c_int),
        "mc_comm_use": ([vp, vp], ctypes.c_int),
        "mc_comm_detach": ([vp], ctypes.c_int),
        "ma_create": ([ctypes.POINTER(MAConfig), ctypes.POINTER(vp)], ctypes.c_int),
        "ma_destroy": ([vp], ctypes.c_int),
        "ma_param_offsets": ([vp, ctypes.POINTER(i64), ctypes.POINTER(i64)], ctypes.c_int),
        "ma_bind": ([vp, vp, vp, vp, vp, vp, vp, vp, vp], ctypes.c_int),
        "ma_set_adam": ([vp, ctypes.POINTER(MAAdam)], ctypes.c_int),
        "ma_set_reward_norm": ([vp, vp], ctypes.c_int),
        "ma_train_step": ([vp, ctypes.POINTER(MQReplay), i64, vp], ctypes.c_int),
        "ma_update_targets": ([vp, ctypes.c_double, vp], ctypes.c_int),
        "ma_critic_forward_workspace": ([ctypes.POINTER(MAConfig), i32, i32], i64),
        "ma_critic_forward": ([vp, ctypes.POINTER(MAConfig), ctypes.POINTER(MQReplay), i32, vp, vp, vp], ctypes.c_int),
        "ma_copy_intermediate": ([vp, ctypes.c_int, vp, ctypes.POINTER(i64), vp], ctypes.c_int),
        "ma_last_plan": ([vp, ctypes.POINTER(MAPlan)], ctypes.c_int),
        "ma_set_ppo": ([vp, ctypes.POINTER(MAPpo)], ctypes.c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    _LIB = lib
    return lib


def check(rc):
    if rc != 0:
        msg = _LIB.mq_last_error().decode() if _LIB is not None else "library not loaded"
        if "not recognised" in msg:
            raise ValueError(msg)
        raise MQError(f"libmq_learner error {rc}: {msg}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def require_gpu(tensor_or_device):
    import torch
    dev = getattr(tensor_or_device, "device", tensor_or_device)
    dev = torch.device(dev)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise MQError(f"the MI355X learner path needs HIP device tensors (got device {dev}); there is no CPU "
                      "fallback — call .cuda() on the learner/MAC and keep the replay on the GPU")


class _Owner:
    """RAII owner of a library handle: <PREFIX>_create on construction, <PREFIX>_destroy on collection, and one list
    of parameter offsets per entry of OFFSETS (attribute name, parameter count), read with <PREFIX>_param_offsets."""
    PREFIX, OFFSETS = None, ()

    def __init__(self, cfg):
        self.lib = load()
        h = ctypes.c_void_p()
        check(self._fn("create")(ctypes.byref(cfg), ctypes.byref(h)))
        self.h = h
        self.cfg = cfg
        offs = [(ctypes.c_int64 * (count + 1))() for _, count in self.OFFSETS]
        check(self._fn("param_offsets")(self.h, *offs))
        for (name, _), o in zip(self.OFFSETS, offs):
            setattr(self, name, list(o))

    def _fn(self, name):
        return getattr(self.lib, "{}_{}".format(self.PREFIX, name))

    def __del__(self):
        try:
            if getattr(self, "h", None) and self.h.value:
                self._fn("destroy")(self.h)
                self.h = ctypes.c_void_p()
        except Exception:
            pass

    def copy_intermediate(self, which, device):
        """<PREFIX>_copy_intermediate's two calls (the size, then the copy on the current stream): array `which` of
        the last step as a flat float32 tensor on `device`."""
        import torch
        cnt = ctypes.c_int64()
        check(self._fn("copy_intermediate")(self.h, which, None, ctypes.byref(cnt), None))
        out = torch.empty(cnt.value, dtype=torch.float32, device=device)
        check(self._fn("copy_intermediate")(self.h, which, ptr(out), ctypes.byref(cnt), stream_ptr()))
        return out


class Handle(_Owner):
    """Owner of an mq_handle (include/mq_learner.h)."""
    PREFIX, OFFSETS = "mq", (("offsets", P_COUNT),)

    @property
    def n_params(self):
        return self.offsets[-1]


class ComaHandle(_Owner):
    """Owner of an mc_handle (include/mc_coma.h)."""
    PREFIX, OFFSETS = "mc", (("agent_offsets", P_COUNT), ("critic_offsets", MC_P_COUNT))


class A2CHandle(_Owner):
    """Owner of an ma_handle (include/ma_a2c.h)."""
    PREFIX, OFFSETS = "ma", (("agent_offsets", P_COUNT), ("critic_offsets", MA_P_COUNT))
