"""ctypes binding of ConvPolicyVFieldNetwork on the device (C ABI: include/goldsrl_fieldnet.h, and include/goldsrl_fieldrollout.h
for acting and learning on a Swarm handle)."""
import ctypes as C

import numpy as np

from . import _ffi, _ffi_paac

_P, _I, _F, _SZ = C.c_void_p, C.c_int32, C.c_float, C.c_size_t


class GrlFieldnetConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("channels", C.c_int32), ("filters", C.c_int32),
                ("conv_layers", C.c_int32), ("num_actions", C.c_int32), ("max_samples", C.c_int32), ("scale", C.c_float),
                ("entropy_beta", C.c_float), ("clip_norm", C.c_float)]


FIELD_SIGNATURES = {
    "grl_fieldnet_config_default": (C.c_int, [C.POINTER(GrlFieldnetConfig)]),
    "grl_fieldnet_create": (C.c_int, [_P, C.POINTER(GrlFieldnetConfig), C.POINTER(_P)]),
    "grl_fieldnet_destroy": (C.c_int, [_P]),
    "grl_fieldnet_last_error": (C.c_char_p, [_P]),
    "grl_fieldnet_num_params": (C.c_int64, [_P]),
    "grl_fieldnet_set_params": (C.c_int, [_P, _P, C.c_int64]),
    "grl_fieldnet_get_params": (C.c_int, [_P, _P, C.c_int64]),
    "grl_fieldnet_get_grads": (C.c_int, [_P, _P, C.c_int64]),
    "grl_fieldnet_predict": (C.c_int, [_P, _I, _P, _P, _P, _P, _P]),
    "grl_fieldnet_train": (C.c_int, [_P, _I, _P, _P, _P, _P, _P, _F, _I, _P]),
}

# include/goldsrl_fieldrollout.h
FIELD_ROLLOUT_SIGNATURES = {
    "grl_fieldnet_rollout_bind": (C.c_int, [_P, _F]),
    "grl_fieldnet_predict_swarm": (C.c_int, [_P, _P, _P, _P]),
    "grl_fieldnet_debug_grid": (C.c_int, [_P, _I, _P, _P, _P, _SZ]),
    "grl_fieldnet_rollout": (C.c_int, [_P, _I, _I]),
    "grl_fieldnet_train_rollout": (C.c_int, [_P, _F, _P]),
    "grl_fieldnet_train_rollout_grads": (C.c_int, [_P, _P]),
    "grl_fieldnet_read_rollout": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
    "grl_fieldnet_get_optimizer_state": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "grl_fieldnet_set_optimizer_state": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64]),
    "grl_fieldnet_get_action_counter": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "grl_fieldnet_set_action_counter": (C.c_int, [_P, C.c_uint64]),
}

# include/goldsrl_fieldeval.h
FIELD_EVAL_SIGNATURES = {
    "grl_fieldnet_eval": (C.c_int, [_P, _I, _I, _I, _I, _I]),
    "grl_fieldnet_read_eval": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}

# grl_fieldnet_read_eval: the traced env's outputs, name -> (shape behind (max_steps,), dtype)
_EVAL_TRACE = {"trace_mu": ((10, 2), np.float32), "trace_sigma": ((10, 2), np.float32), "trace_value": ((), np.float32),
               "trace_raw": ((10, 2), np.float32), "trace_locust_bins": ((80, 2), np.uint8), "trace_agent_bins": ((10, 2), np.uint8),
               "trace_positions": ((10, 2), np.uint8), "trace_x": ((80, 2), np.float64), "trace_xa": ((10, 2), np.float64)}

# grl_fieldnet_read_rollout: name -> (shape behind (T,), per (E or B), dtype)
_ROLLOUT_BUFFERS = {"actions": ("B", (2,), np.float32), "env_actions": ("B", (2,), np.float32), "mu": ("B", (2,), np.float32),
                    "sigma": ("B", (2,), np.float32), "values": ("B", (), np.float32), "rewards": ("B", (), np.float32),
                    "y": ("B", (), np.float32), "adv": ("B", (), np.float32), "dones": ("E", (), np.uint8),
                    "locust_bins": ("E", (80, 2), np.uint8), "agent_bins": ("E", (10, 2), np.uint8), "positions": ("E", (10, 2), np.uint8)}


def field_param_shapes(height=32, width=32, channels=3, filters=5, conv_layers=2, num_actions=3, fc_hidden=32):
    """tf.trainable_variables() order of ConvPolicyVFieldNetwork (policy_v_network.py:95-168)."""
    fh, fw = int(height / (2 ** conv_layers)), int(width / (2 ** conv_layers))
    shapes, cin = [], channels
    for i in range(conv_layers):
        shapes += [("conv%d_w" % i, (3, 3, cin, filters)), ("conv%d_b" % i, (filters,))]
        cin = filters
    hwa = height * width * num_actions
    return shapes + [
        ("dense1_w", (fh * fw * filters, 2 * fc_hidden)), ("dense1_b", (2 * fc_hidden,)), ("dense2_w", (2 * fc_hidden, fc_hidden)), ("dense2_b", (fc_hidden,)),
        ("pol1_w", (fc_hidden, 2 * fc_hidden)), ("pol1_b", (2 * fc_hidden,)), ("pol2_w", (2 * fc_hidden, 2 * hwa)), ("pol2_b", (2 * hwa,)),
        ("mu_w", (2 * hwa, hwa)), ("mu_b", (hwa,)), ("sigma_w", (2 * hwa, hwa)), ("sigma_b", (hwa,)),
        ("v1_w", (fc_hidden, 2 * fc_hidden)), ("v1_b", (2 * fc_hidden,)), ("v2_w", (2 * fc_hidden, fc_hidden)), ("v2_b", (fc_hidden,)),
        ("v3_w", (fc_hidden, 1)), ("v3_b", (1,))]


def glorot_uniform_flat(seed=3, **geometry):
    """tf.layers defaults: glorot-uniform kernels, zero biases -> flat float32 vector."""
    return _ffi_paac.glorot_uniform_flat(field_param_shapes(**geometry), seed)


class FieldNet(_ffi_paac.PaacRolloutNet):
    PREFIX = "grl_fieldnet_"

    def __init__(self, engine, **kw):
        self._create(engine, dict(FIELD_SIGNATURES, **dict(FIELD_ROLLOUT_SIGNATURES, **FIELD_EVAL_SIGNATURES)), GrlFieldnetConfig(), kw)

    def _inputs(self, states, positions):
        c = self.cfg
        s = np.ascontiguousarray(states, np.float32)
        p = np.ascontiguousarray(positions, np.int32)
        if s.ndim != 4 or s.shape[1:] != (c.height, c.width, c.channels) or p.shape != (s.shape[0], 2):
            raise ValueError("expected states (n,%d,%d,%d) and positions (n,2), got %s and %s" % (c.height, c.width, c.channels, s.shape, p.shape))
        return s, p

    def predict(self, states, positions):
        s, p = self._inputs(states, positions)
        n, A = s.shape[0], int(self.cfg.num_actions)
        mu, sg, vs = np.empty((n, A), np.float32), np.empty((n, A), np.float32), np.empty(n, np.float32)
        self._check(self.lib.grl_fieldnet_predict(self.n, n, _ffi._ptr(s), _ffi._ptr(p), _ffi._ptr(mu), _ffi._ptr(sg), _ffi._ptr(vs)))
        return {"mu": mu, "sigma": sg, "vs": vs}

    def train(self, states, positions, actions, advantages, critic_target, lr, apply_update=True):
        s, p = self._inputs(states, positions)
        n = s.shape[0]
        a = np.ascontiguousarray(actions, np.float32)
        adv, y = np.ascontiguousarray(advantages, np.float32), np.ascontiguousarray(critic_target, np.float32)
        if a.shape != (n, int(self.cfg.num_actions)) or adv.shape != (n,) or y.shape != (n,):
            raise ValueError("train: actions (n,A), advantages (n,), critic_target (n,) expected")
        return self._stats4("train", n, _ffi._ptr(s), _ffi._ptr(p), _ffi._ptr(a), _ffi._ptr(adv), _ffi._ptr(y), lr, 1 if apply_update else 0)

    # -- acting and learning on the Swarm handle the net was created on (include/goldsrl_fieldrollout.h)
    def rollout_bind(self, gamma):
        self._check(self.lib.grl_fieldnet_rollout_bind(self.n, gamma))

    def predict_swarm(self):
        """predict on the handle's current observation: B = 10 * E agent-samples in env-major order."""
        B = self.eng.E * 10
        mu, sg, vs = np.empty((B, 2), np.float32), np.empty((B, 2), np.float32), np.empty(B, np.float32)
        self._check(self.lib.grl_fieldnet_predict_swarm(self.n, _ffi._ptr(mu), _ffi._ptr(sg), _ffi._ptr(vs)))
        return {"mu": mu, "sigma": sg, "vs": vs}

    def debug_grid(self, locust_bins, agent_bins):
        """The (n_envs, G, G, 2) density images the device builds from host observations."""
        lb = np.ascontiguousarray(locust_bins, np.uint8); ab = np.ascontiguousarray(agent_bins, np.uint8)
        G = int(self.cfg.height)
        out = np.empty((lb.shape[0], G, G, 2), np.float32)
        self._check(self.lib.grl_fieldnet_debug_grid(self.n, lb.shape[0], _ffi._ptr(lb), _ffi._ptr(ab), _ffi._ptr(out), out.nbytes))
        return out

    # -- whole episodes in one launch (include/goldsrl_fieldeval.h)
    def read_eval(self, which, max_steps):
        """An output of the last eval of max_steps steps by name."""
        E, S = self.eng.E, int(max_steps)
        if which in _EVAL_TRACE:
            inner, dtype = _EVAL_TRACE[which]
            a = np.empty((S,) + inner, dtype)
        else:
            shape, dtype = {"rewards": ((E, S), np.float64), "length": ((E,), np.int32), "finished": ((E,), np.uint8),
                            "actions": ((E, S, 10, 2), np.float64)}.get(which, ((0,), np.uint8))      # an unknown name is the library's to refuse
            a = np.empty(shape, dtype)
        self._check(self.lib.grl_fieldnet_read_eval(self.n, which.encode(), _ffi._ptr(a), a.nbytes))
        return a

    def eval(self, max_steps, greedy=True, rows32=False, keep_actions=False, trace_env=-1):
        """Every env of the engine plays one episode from its CURRENT state (reset first), at most max_steps steps, in one kernel
        launch; the engine and the net are left as they were.  greedy: the action is the norm-clipped mu, else mu + sigma N(0,1)
        drawn with the rollout's noise key at the net's action counter (which stays).  rows32: step with the float32 row, as the
        training rollout does, else with its float64 widening (SwarmEnv.step called directly).  Returns rewards (E,S) float64,
        length (E), finished (E), total_reward (E) -- the float64 sum in step order -- plus actions (E,S,10,2) with keep_actions
        and the trace_* outputs of env trace_env."""
        S = int(max_steps)
        self._check(self.lib.grl_fieldnet_eval(self.n, S, 1 if greedy else 0, 1 if rows32 else 0, 1 if keep_actions else 0, int(trace_env)))
        names = ["rewards", "length", "finished"] + (["actions"] if keep_actions else []) + (sorted(_EVAL_TRACE) if trace_env >= 0 else [])
        out = {k: self.read_eval(k, S) for k in names}
        total = np.zeros(self.eng.E, np.float64)
        for t in range(S):      # step order; rewards past an env's length are zero
            total = total + out["rewards"][:, t]
        out["total_reward"] = total
        return out

    def rollout(self, T, layout=0):
        self._check(self.lib.grl_fieldnet_rollout(self.n, T, layout))

    def read_rollout(self, which, T=None):
        """A buffer of the last rollout of T steps by name; "boot" is (B,)."""
        E = self.eng.E
        if which == "boot":
            a = np.empty(E * 10, np.float32)
        else:
            if which not in _ROLLOUT_BUFFERS:
                raise ValueError("unknown rollout buffer %r" % (which,))
            per, inner, dtype = _ROLLOUT_BUFFERS[which]
            a = np.empty((int(T), E * 10 if per == "B" else E) + inner, dtype)
        self._check(self.lib.grl_fieldnet_read_rollout(self.n, which.encode(), _ffi._ptr(a), a.nbytes))
        return a
