"""ctypes binding of the estimator side of libgoldsrl.so (C ABI: include/goldsrl_net.h)."""
import ctypes as C

import numpy as np

from . import _ffi, _ffi_paac

_P, _I, _F, _SZ = C.c_void_p, C.c_int32, C.c_float, C.c_size_t


class GrlNetConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("kind", C.c_int32), ("max_chunk_samples", C.c_int32), ("reserved", C.c_int32),
                ("scale", C.c_float), ("entropy_beta", C.c_float), ("clip_norm", C.c_float), ("gamma", C.c_float),
                ("num_actions", C.c_int32), ("reserved2", C.c_int32)]


NET_SIGNATURES = {
    "grl_net_config_default": (C.c_int, [_I, C.POINTER(GrlNetConfig)]),
    "grl_net_create": (C.c_int, [_P, C.POINTER(GrlNetConfig), C.POINTER(_P)]),
    "grl_net_destroy": (C.c_int, [_P]),
    "grl_net_last_error": (C.c_char_p, [_P]),
    "grl_net_num_params": (C.c_int64, [_P]),
    "grl_net_set_params": (C.c_int, [_P, _P, C.c_int64]),
    "grl_net_get_params": (C.c_int, [_P, _P, C.c_int64]),
    "grl_net_get_grads": (C.c_int, [_P, _P, C.c_int64]),
    "grl_net_get_action_counter": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "grl_net_set_action_counter": (C.c_int, [_P, C.c_uint64]),
    "grl_net_get_optimizer_state": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "grl_net_set_optimizer_state": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64]),
    "grl_net_predict": (C.c_int, [_P, _P, _P, _P]),
    "grl_net_predict_obs": (C.c_int, [_P, _I, _P, _P, _P, _P, _P, _P]),
    "grl_net_rollout": (C.c_int, [_P, _I, _I]),
    "grl_net_train_rollout": (C.c_int, [_P, _F, _P]),
    "grl_net_train_rollout_grads": (C.c_int, [_P, _P]),
    "grl_net_set_grads": (C.c_int, [_P, _P, C.c_int64]),
    "grl_net_apply_grads": (C.c_int, [_P, _F, _F, _P]),
    "grl_net_train_obs": (C.c_int, [_P, _I, _P, _P, _P, _P, _P, _P, _F, _I, _P]),
    "grl_net_read_rollout": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
    "grl_net_read_activation": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
    "grl_comm_unique_id_bytes": (C.c_size_t, []),
    "grl_comm_unique_id": (C.c_int, [_P, _SZ]),
    "grl_net_comm_init": (C.c_int, [_P, _P, _SZ, _I, _I]),
    "grl_net_comm_broadcast_params": (C.c_int, [_P, _I]),
    "grl_net_comm_destroy": (C.c_int, [_P]),
    "grl_net_comm_info": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "grl_net_debug_obs_index": (C.c_int, [_P, _I, _P, _P, _P, _P, _SZ]),
    "grl_net_range_info": (C.c_int, [_P, _P, _P, _P]),
    "grl_net_host_times": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "grl_net_keep_info": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "grl_net_set_gemm_f32": (C.c_int, [_P, C.c_int32]),
    "grl_net_range_return_info": (C.c_int, [_P, _P, _P, _P, _P]),
    "grl_net_set_range_return": (C.c_int, [_P, C.c_int32]),
    "grl_net_profile_enable": (C.c_int, [_P, _I]),
    "grl_net_profile_read": (C.c_int, [_P, C.POINTER(_I), C.POINTER(C.c_float), C.POINTER(C.c_double)]),
    "grl_net_profile_read_tags": (C.c_int, [_P, _I, _P, _P, _P]),
}

# include/goldsrl_neteval.h
NET_EVAL_SIGNATURES = {
    "grl_net_eval": (C.c_int, [_P, _I, _I, _P, _I, _I]),
    "grl_net_read_eval": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}

# grl_net_read_eval: the traced env's outputs, name -> shape behind (max_steps,); all float32
_EVAL_TRACE = {"trace_mu": (10, 2), "trace_sigma": (10, 2), "trace_raw": (10, 2), "trace_value": (10,)}

NET_CONV_SINGLE_AGENT = 0

# (name, shape) in flat-vector order == tf.trainable_variables() creation order
# (reference fed_gym/agents/paac/policy_v_network.py:14-59)
def conv_param_shapes(num_actions=2):
    A = int(num_actions)
    return [
        ("conv1_w", (8, 8, 3, 32)), ("conv1_b", (32,)), ("conv2_w", (4, 4, 32, 64)), ("conv2_b", (64,)),
        ("conv3_w", (3, 3, 64, 64)), ("conv3_b", (64,)), ("dense1_w", (3136, 512)), ("dense1_b", (512,)),
        ("dense2_w", (512, 256)), ("dense2_b", (256,)), ("pol1_w", (256, 512)), ("pol1_b", (512,)),
        ("mu_w", (512, A)), ("mu_b", (A,)), ("sigma_w", (512, A)), ("sigma_b", (A,)),
        ("v1_w", (256, 512)), ("v1_b", (512,)), ("v2_w", (512, 256)), ("v2_b", (256,)), ("v3_w", (256, 1)), ("v3_b", (1,)),
    ]


CONV_PARAM_SHAPES = conv_param_shapes(2)      # train_paac_conv.py: SwarmEnvironmentCreator.num_actions = 2


def glorot_uniform_flat(seed=3, num_actions=2):
    """tf.layers defaults: glorot-uniform kernels, zero biases -> flat float32 vector."""
    return _ffi_paac.glorot_uniform_flat(conv_param_shapes(num_actions), seed)


class ConvNet(_ffi_paac.PaacTrainerNet):
    """ConvSingleAgentPolicyNetwork on the device of a Swarm Engine."""

    PREFIX = "grl_net_"

    def __init__(self, engine, **kw):
        self._create(engine, dict(NET_SIGNATURES, **NET_EVAL_SIGNATURES), GrlNetConfig(), kw, NET_CONV_SINGLE_AGENT)

    def predict(self):
        B, A = self.eng.E * 10, int(self.cfg.num_actions)
        mu, sg, vs = np.empty((B, A), np.float32), np.empty((B, A), np.float32), np.empty(B, np.float32)
        self._check(self.lib.grl_net_predict(self.n, _ffi._ptr(mu), _ffi._ptr(sg), _ffi._ptr(vs)))
        return {"mu": mu, "sigma": sg, "vs": vs}

    def predict_obs(self, locust_bins, agent_bins, positions):
        lb = np.ascontiguousarray(locust_bins, np.uint8); ab = np.ascontiguousarray(agent_bins, np.uint8)
        ps = np.ascontiguousarray(positions, np.uint8)
        ne = lb.shape[0]
        B, A = ne * 10, int(self.cfg.num_actions)
        mu, sg, vs = np.empty((B, A), np.float32), np.empty((B, A), np.float32), np.empty(B, np.float32)
        self._check(self.lib.grl_net_predict_obs(self.n, ne, _ffi._ptr(lb), _ffi._ptr(ab), _ffi._ptr(ps), _ffi._ptr(mu),
                                                 _ffi._ptr(sg), _ffi._ptr(vs)))
        return {"mu": mu, "sigma": sg, "vs": vs}

    def debug_obs_index(self, locust_bins, agent_bins, positions):
        """The device's observation index records (obs_index_kernel) of host observations: (n_envs, 288) uint32."""
        lb = np.ascontiguousarray(locust_bins, np.uint8); ab = np.ascontiguousarray(agent_bins, np.uint8)
        ps = np.ascontiguousarray(positions, np.uint8)
        rec = np.empty((lb.shape[0], 288), np.uint32)
        self._check(self.lib.grl_net_debug_obs_index(self.n, lb.shape[0], _ffi._ptr(lb), _ffi._ptr(ab), _ffi._ptr(ps), _ffi._ptr(rec),
                                                     rec.nbytes))
        return rec

    def train_obs(self, locust_bins, agent_bins, positions, actions, advantages, critic_target, lr, apply_update=True):
        lb = np.ascontiguousarray(locust_bins, np.uint8); ab = np.ascontiguousarray(agent_bins, np.uint8)
        ps = np.ascontiguousarray(positions, np.uint8)
        a = np.ascontiguousarray(actions, np.float32); adv = np.ascontiguousarray(advantages, np.float32)
        y = np.ascontiguousarray(critic_target, np.float32)
        if a.shape != (lb.shape[0] * 10, int(self.cfg.num_actions)):
            raise ValueError("train_obs: actions must be (%d, %d), got %s" % (lb.shape[0] * 10, self.cfg.num_actions, a.shape))
        return self._stats4("train_obs", lb.shape[0], _ffi._ptr(lb), _ffi._ptr(ab), _ffi._ptr(ps), _ffi._ptr(a), _ffi._ptr(adv), _ffi._ptr(y), lr,
                            1 if apply_update else 0)

    def rollout(self, T, reward_layout=0):
        self._check(self.lib.grl_net_rollout(self.n, T, reward_layout))

    def read_rollout(self, which, shape, dtype=np.float32):
        a = np.empty(shape, dtype)
        self._check(self.lib.grl_net_read_rollout(self.n, which.encode(), _ffi._ptr(a), a.nbytes))
        return a

    # -- whole evaluation episodes on the engine, nothing read back per step (include/goldsrl_neteval.h)
    def read_eval(self, which, max_steps):
        """An output of the last eval of max_steps steps by name.  The first read after an eval raises E_RANGE when a forward pass of
        it left the fp16 range: the net is on the fp32 form then (unless the fallback is off); reset the env and eval again."""
        E, S = self.eng.E, int(max_steps)
        if which in _EVAL_TRACE:
            a = np.empty((S,) + _EVAL_TRACE[which], np.float32)
        else:
            shape, dtype = {"rewards": ((E, S), np.float64), "length": ((E,), np.int32), "finished": ((E,), np.uint8),
                            "actions": ((E, S, 10, 2), np.float32)}.get(which, ((0,), np.uint8))      # an unknown name is the library's to refuse
            a = np.empty(shape, dtype)
        self._check(self.lib.grl_net_read_eval(self.n, which.encode(), _ffi._ptr(a), a.nbytes))
        return a

    def eval(self, max_steps, greedy=False, normals=None, keep_actions=False, trace_env=-1):
        """Every env of the engine plays one episode from its CURRENT state (reset first), at most max_steps steps, enqueued as
        one pipeline (per step and chunk: forward, action, env step, accounting) and read back once.  The engine's env state
        advances as a host loop's would; the net's parameters, optimizer state, action counter and last rollout stay as they were.
        greedy: the action is the norm-clipped mu; else mu + sigma z with z = normals[env, t] -- (E, max_steps, 10, 2) float64, e.g.
        a seeded generator's draws -- or, without normals, the rollout's keyed noise at the net's action counter (which stays).
        The env steps with the float32 row.  Returns rewards (E,S) float64, length (E), finished (E), total_reward (E) -- the
        float64 sum in step order -- plus actions (E,S,10,2) float32 with keep_actions and the trace_* outputs of env trace_env."""
        S = int(max_steps)
        z = None
        if normals is not None:
            z = np.ascontiguousarray(normals, np.float64)
            if z.shape != (self.eng.E, S, 10, 2):
                raise ValueError("eval: normals must be %s, got %s" % ((self.eng.E, S, 10, 2), z.shape))
        self._check(self.lib.grl_net_eval(self.n, S, 1 if greedy else 0, None if z is None else _ffi._ptr(z), 1 if keep_actions else 0, int(trace_env)))
        self.eng.wait()      # the join, as behind rollout(); the reads below find the streams drained
        names = ["rewards", "length", "finished"] + (["actions"] if keep_actions else []) + (sorted(_EVAL_TRACE) if trace_env >= 0 else [])
        out = {k: self.read_eval(k, S) for k in names}
        total = np.zeros(self.eng.E, np.float64)
        for t in range(S):      # step order; rewards past an env's length are zero
            total = total + out["rewards"][:, t]
        out["total_reward"] = total
        return out

    def read_activation(self, which, shape):
        a = np.empty(shape, np.float32)
        self._check(self.lib.grl_net_read_activation(self.n, which.encode(), _ffi._ptr(a), a.nbytes))
        return a

    def host_times(self):
        """Wall-clock ms this thread spent enqueueing rollouts / gradient steps and waiting for the device (grl_net_host_times)."""
        ro, up = C.c_int64(0), C.c_int64(0)
        a, b, c = C.c_double(0), C.c_double(0), C.c_double(0)
        self._check(self.lib.grl_net_host_times(self.n, C.byref(ro), C.byref(up), C.byref(a), C.byref(b), C.byref(c)))
        return {"rollouts": int(ro.value), "updates": int(up.value), "rollout_enqueue_ms": a.value, "train_enqueue_ms": b.value,
                "train_wait_ms": c.value}

    def keep_info(self):
        """Which form of the gradient step over a rollout this net runs (grl_net_keep_info): 'level' 0..3 and 'slots' of the resident
        buffer (0, 0 before the first rollout), 'slot_bytes' {1, 2, 3: bytes per slot at that level}, 'headroom_bytes' and
        'free_bytes' the choice was made with, 'resident' = the last train_rollout* call read the rollout's resident activations."""
        lv, res, slots, hr, fr = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        sb = (C.c_int64 * 3)()
        self._check(self.lib.grl_net_keep_info(self.n, C.byref(lv), C.byref(slots), sb, C.byref(hr), C.byref(fr), C.byref(res)))
        return {"level": lv.value, "slots": int(slots.value), "slot_bytes": {1: int(sb[0]), 2: int(sb[1]), 3: int(sb[2])},
                "headroom_bytes": int(hr.value), "free_bytes": int(fr.value), "resident": bool(res.value)}

    def range_info(self):
        """Arithmetic form of the GEMMs: 'gemm_f32' once a range violation (or set_gemm_f32) moved the net to the fp32 form,
        'fallbacks' = how often that happened, 'update_skipped' = the last train_rollout* call gave its update up."""
        f32, fb, sk = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.grl_net_range_info(self.n, C.byref(f32), C.byref(fb), C.byref(sk)))
        return {"gemm_f32": bool(f32.value), "fallbacks": fb.value, "update_skipped": bool(sk.value)}

    def set_gemm_f32(self, on=True):
        self._check(self.lib.grl_net_set_gemm_f32(self.n, 1 if on else 0))

    def range_return_info(self):
        """The way back from a range fallback: 'returns' = how often the net went back to the fp16 form, 'clean_passes' = clean updates
        counted so far on the fp32 form, 'needed' = how many in a row it takes (0: never), 'absmax_last' = the largest |GEMM output|
        the last decision saw."""
        r, c, k, a = C.c_int32(), C.c_int32(), C.c_int32(), C.c_float()
        self._check(self.lib.grl_net_range_return_info(self.n, C.byref(r), C.byref(c), C.byref(k), C.byref(a)))
        return {"returns": r.value, "clean_passes": c.value, "needed": k.value, "absmax_last": a.value}

    def set_range_return(self, clean_passes):
        self._check(self.lib.grl_net_set_range_return(self.n, int(clean_passes)))

    def profile_enable(self, on=True):
        self._check(self.lib.grl_net_profile_enable(self.n, 1 if on else 0))

    PROFILE_TAGS = ("other", "dense_small_fwd", "dense_small_dgrad", "dense_small_wgrad", "dense1_patch_fwd", "dense1_patch_dgrad",
                    "dense1_patch_wgrad", "per_env_fwd", "per_env_dgrad", "per_env_wgrad", "slot_products_fwd", "slot_dgrad", "slot_wgrad",
                    "conv2_class_corrections", "per_agent_mode", "-")

    def profile_read_tags(self):
        """{family: (launches, ms, flops)} of the bracketed GEMM launches since profile_enable(True)."""
        k = len(self.PROFILE_TAGS)
        n, ms, fl = np.zeros(k, np.int32), np.zeros(k, np.float32), np.zeros(k, np.float64)
        self._check(self.lib.grl_net_profile_read_tags(self.n, k, _ffi._ptr(n), _ffi._ptr(ms), _ffi._ptr(fl)))
        return {name: (int(n[i]), float(ms[i]), float(fl[i])) for i, name in enumerate(self.PROFILE_TAGS) if n[i]}

    def profile_read(self):
        n, ms, fl = C.c_int32(), C.c_float(), C.c_double()
        self._check(self.lib.grl_net_profile_read(self.n, C.byref(n), C.byref(ms), C.byref(fl)))
        return n.value, ms.value, fl.value
