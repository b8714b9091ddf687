"""ctypes binding of FlatPolicyVNetwork on the device (C ABI: include/goldsrl_flatnet.h)."""
import ctypes as C

import numpy as np

from . import _ffi, _ffi_paac

_P, _I, _F, _SZ = C.c_void_p, C.c_int32, C.c_float, C.c_size_t


class GrlFnetConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("static_size", C.c_int32), ("temporal_size", C.c_int32), ("rnn_length", C.c_int32),
                ("num_actions", C.c_int32), ("rnn_hidden", C.c_int32), ("static_hidden", C.c_int32), ("max_samples", C.c_int32),
                ("scale", C.c_float), ("clip_norm", C.c_float), ("gamma", C.c_float), ("mu_bound", C.c_float), ("gae_lambda", C.c_float)]


FNET_SIGNATURES = {
    "grl_fnet_config_default": (C.c_int, [C.POINTER(GrlFnetConfig)]),
    "grl_fnet_create": (C.c_int, [_P, C.POINTER(GrlFnetConfig), C.POINTER(_P)]),
    "grl_fnet_destroy": (C.c_int, [_P]),
    "grl_fnet_last_error": (C.c_char_p, [_P]),
    "grl_fnet_num_params": (C.c_int64, [_P]),
    "grl_fnet_set_params": (C.c_int, [_P, _P, C.c_int64]),
    "grl_fnet_get_params": (C.c_int, [_P, _P, C.c_int64]),
    "grl_fnet_get_grads": (C.c_int, [_P, _P, C.c_int64]),
    "grl_fnet_get_action_counter": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "grl_fnet_set_action_counter": (C.c_int, [_P, C.c_uint64]),
    "grl_fnet_get_optimizer_state": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "grl_fnet_set_optimizer_state": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64]),
    "grl_fnet_predict": (C.c_int, [_P, _I, _P, _P, _P, _P, _P]),
    "grl_fnet_predict_env": (C.c_int, [_P, _P, _P, _P]),
    "grl_fnet_train": (C.c_int, [_P, _I, _P, _P, _P, _P, _P, _F, _I, _P]),
    "grl_fnet_rollout": (C.c_int, [_P, _I]),
    "grl_fnet_set_keep_activations": (C.c_int, [_P, _I]),
    "grl_fnet_train_rollout": (C.c_int, [_P, _F, _P]),
    "grl_fnet_read_rollout": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
    "grl_fnet_train_rollout_grads": (C.c_int, [_P, _P]),
    "grl_fnet_set_grads": (C.c_int, [_P, _P, C.c_int64]),
    "grl_fnet_apply_grads": (C.c_int, [_P, _F, _F, _P]),
    "grl_fnet_comm_init": (C.c_int, [_P, _P, _SZ, _I, _I]),
    "grl_fnet_comm_broadcast_params": (C.c_int, [_P, _I]),
    "grl_fnet_comm_destroy": (C.c_int, [_P]),
    "grl_fnet_comm_info": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "grl_fnet_rollout_stage_times": (C.c_int, [_P, _P, _I, _P]),
    "grl_comm_unique_id_bytes": (C.c_size_t, []),
    "grl_comm_unique_id": (C.c_int, [_P, _SZ]),
}

# include/goldsrl_flateval.h: greedy acting and the one-launch evaluation (tests/test_flat_eval_header.py holds the two together)
FNET_EVAL_SIGNATURES = {
    "grl_fnet_set_greedy": (C.c_int, [_P, _I]),
    "grl_fnet_eval": (C.c_int, [_P, _I, _I, _I]),
    "grl_fnet_read_eval": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}

# include/goldsrl_flatwindow.h: the true history window (tests/test_flat_window_header.py holds the two together)
FNET_WINDOW_SIGNATURES = {
    "grl_fnet_set_true_window": (C.c_int, [_P, _I]),
    "grl_fnet_read_windows": (C.c_int, [_P, _I, _I, _P, _SZ]),
}


def flat_param_shapes(static_size=2, temporal_size=2, num_actions=1, H=32, S=32):
    """tf.trainable_variables() order of FlatPolicyVNetwork (policy_v_network.py:207-244, a3c/estimators.py:18-28)."""
    return [
        ("gru_gates_w", (temporal_size + H, 2 * H)), ("gru_gates_b", (2 * H,)), ("gru_cand_w", (temporal_size + H, H)), ("gru_cand_b", (H,)),
        ("temporal_w", (H, 2 * H)), ("temporal_b", (2 * H,)), ("static1_w", (static_size, 2 * H)), ("static1_b", (2 * H,)),
        ("static2_w", (2 * H, H)), ("static2_b", (H,)),
        ("mu1_w", (3 * H, 2 * S)), ("mu1_b", (2 * S,)), ("mu2_w", (2 * S, S)), ("mu2_b", (S,)), ("mu3_w", (S, num_actions)), ("mu3_b", (num_actions,)),
        ("sig1_w", (3 * H, 2 * S)), ("sig1_b", (2 * S,)), ("sig2_w", (2 * S, S)), ("sig2_b", (S,)), ("sig3_w", (S, num_actions)), ("sig3_b", (num_actions,)),
        ("v1_w", (3 * H, 2 * S)), ("v1_b", (2 * S,)), ("v2_w", (2 * S, 1)), ("v2_b", (1,)),
    ]


def default_init_flat(seed=3, **kw):
    """glorot-uniform kernels, zero biases except GRU gate bias = 1 and sigma-head bias = -1."""
    rng = np.random.RandomState(seed)
    parts = []
    for name, shape in flat_param_shapes(**kw):
        if name.endswith("_w"):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            parts.append(rng.uniform(-lim, lim, size=shape).reshape(-1))
        elif name == "gru_gates_b":
            parts.append(np.ones(shape))
        elif name == "sig3_b":
            parts.append(-np.ones(shape))
        else:
            parts.append(np.zeros(shape))
    return np.concatenate(parts).astype(np.float32)


class FlatNet(_ffi_paac.PaacTrainerNet):
    PREFIX = "grl_fnet_"

    def __init__(self, engine, **kw):
        self._create(engine, dict(FNET_SIGNATURES, **FNET_EVAL_SIGNATURES, **FNET_WINDOW_SIGNATURES), GrlFnetConfig(), kw)

    def _outs(self, n):
        A = self.cfg.num_actions
        return np.empty((n, A), np.float32), np.empty((n, A), np.float32), np.empty(n, np.float32)

    def predict(self, states, histories):
        s = np.ascontiguousarray(states, np.float32); h = np.ascontiguousarray(histories, np.float32)
        mu, sg, vs = self._outs(s.shape[0])
        self._check(self.lib.grl_fnet_predict(self.n, s.shape[0], _ffi._ptr(s), _ffi._ptr(h), _ffi._ptr(mu), _ffi._ptr(sg), _ffi._ptr(vs)))
        return {"mu": mu, "sigma": sg, "vs": vs}

    def predict_env(self):
        mu, sg, vs = self._outs(self.eng.E)
        self._check(self.lib.grl_fnet_predict_env(self.n, _ffi._ptr(mu), _ffi._ptr(sg), _ffi._ptr(vs)))
        return {"mu": mu, "sigma": sg, "vs": vs}

    def train(self, states, histories, actions, advantages, critic_target, lr, apply_update=True):
        arrs = [np.ascontiguousarray(a, np.float32) for a in (states, histories, actions, advantages, critic_target)]
        return self._stats4("train", arrs[0].shape[0], *([_ffi._ptr(a) for a in arrs] + [lr, 1 if apply_update else 0]))

    _last_T = 0

    def rollout(self, T):
        self._check(self.lib.grl_fnet_rollout(self.n, T))
        self._last_T = int(T)

    def set_keep_activations(self, on):
        """The rollouts that follow fill the training workspace; train_rollout on them starts at the backward pass (bit-identical
        gradients, the rollout pays the stores).  Off by default."""
        self._check(self.lib.grl_fnet_set_keep_activations(self.n, 1 if on else 0))

    def set_greedy(self, on):
        """on: rollout draws nothing, raw = mu ("actions" reads back equal to mu); the action counter stands still."""
        self._check(self.lib.grl_fnet_set_greedy(self.n, 1 if on else 0))

    def set_true_window(self, on):
        """on: rollout, predict_env, eval and train_rollout run the net under the true window -- the last min(k + 1, rnn) states of
        the env's episode -- instead of the worker's copies of the current state (quirk Q11).  Restarts every window."""
        self._check(self.lib.grl_fnet_set_true_window(self.n, 1 if on else 0))

    def read_windows(self, first=0, count=None):
        """Dense (count, rnn, D) true windows of samples [first, first + count) of the last rollout's flattened (T * E) batch."""
        if count is None:
            count = self._last_T * self.eng.E - first
        a = np.empty((count, self.cfg.rnn_length, self.cfg.temporal_size), np.float32)
        self._check(self.lib.grl_fnet_read_windows(self.n, int(first), int(count), _ffi._ptr(a), a.nbytes))
        return a

    EVAL_TRACE = ("states", "nhist", "mu", "sigma", "raw", "actions", "values", "rewards", "dones")

    def eval(self, max_steps, trace_steps=0, greedy=False, trace_fields=EVAL_TRACE):
        """Episodes of every env from the engine's current state (reset it first), one kernel launch; the engine is reset afterwards.
        greedy=False draws the rollout's action noise at counters action_counter + t and advances the counter by max_steps.
        Returns total_reward (E) float64, length (E) int32, finished (E) uint8 and, with trace_steps > 0, states (S,E,S0), nhist
        (S,E) int32, mu, sigma, raw, actions (S,E,A), values, rewards, dones (S,E) of the first S = min(trace_steps, steps played)
        steps, each defined up to its env's own end (trace_fields: the ones to read back)."""
        self._check(self.lib.grl_fnet_eval(self.n, int(max_steps), int(trace_steps), 1 if greedy else 0))
        E, A, S0 = self.eng.E, self.cfg.num_actions, self.cfg.static_size
        out = {"total_reward": np.empty(E, np.float64), "length": np.empty(E, np.int32), "finished": np.empty(E, np.uint8)}
        for k in ("total_reward", "length", "finished"):
            self._check(self.lib.grl_fnet_read_eval(self.n, k.encode(), _ffi._ptr(out[k]), out[k].nbytes))
        if trace_steps > 0:
            S = min(int(trace_steps), int(max_steps), int(out["length"].max()))
            tails = {"states": (S0,), "nhist": (), "mu": (A,), "sigma": (A,), "raw": (A,), "actions": (A,), "values": (), "rewards": (),
                     "dones": ()}
            for k in trace_fields:
                out[k] = np.empty((S, E) + tails[k], np.int32 if k == "nhist" else np.float32)
                self._check(self.lib.grl_fnet_read_eval(self.n, k.encode(), _ffi._ptr(out[k]), out[k].nbytes))
        return out

    def rollout_stage_times(self):
        """Constant-clock ticks (10 ns) of workgroup 0 at every barrier of the last persistent rollout (first call: attaches)."""
        buf = np.zeros(4096, np.int64)
        n = C.c_int32()
        self._check(self.lib.grl_fnet_rollout_stage_times(self.n, _ffi._ptr(buf), 4096, C.byref(n)))
        return buf[:n.value].copy()

    def read_rollout(self, which, shape):
        a = np.empty(shape, np.float32)
        self._check(self.lib.grl_fnet_read_rollout(self.n, which.encode(), _ffi._ptr(a), a.nbytes))
        return a
