"""ctypes binding of the Ticker gated trader on the device (C ABI: include/goldsrl_gatednet.h)."""
import ctypes as C

import numpy as np

from . import _ffi

_P, _I, _F, _SZ = C.c_void_p, C.c_int32, C.c_float, C.c_size_t

N_ASSETS, N_CHOICES, STATIC_SIZE, TEMPORAL_SIZE = 2, 3, 7, 4
STAT_NAMES = ("policy_loss", "value_loss", "entropy_mean", "policy_norm", "value_norm", "lr")


class GrlGnetConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("rnn_length", C.c_int32), ("max_samples", C.c_int32), ("lr_decay_steps", C.c_int32),
                ("scale", C.c_float), ("gamma", C.c_float), ("gae_lambda", C.c_float), ("clip_norm", C.c_float),
                ("rms_decay", C.c_float), ("rms_epsilon", C.c_float), ("lr_decay_rate", C.c_float)]


GNET_SIGNATURES = {
    "grl_gnet_config_default": (C.c_int, [C.POINTER(GrlGnetConfig)]),
    "grl_gnet_create": (C.c_int, [_P, C.POINTER(GrlGnetConfig), C.POINTER(_P)]),
    "grl_gnet_destroy": (C.c_int, [_P]),
    "grl_gnet_last_error": (C.c_char_p, [_P]),
    "grl_gnet_num_params": (C.c_int64, [_P]),
    "grl_gnet_set_params": (C.c_int, [_P, _P, C.c_int64]),
    "grl_gnet_get_params": (C.c_int, [_P, _P, C.c_int64]),
    "grl_gnet_get_grads": (C.c_int, [_P, _I, _P, C.c_int64]),
    "grl_gnet_get_optimizer_state": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "grl_gnet_set_optimizer_state": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64]),
    "grl_gnet_get_action_counter": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "grl_gnet_set_action_counter": (C.c_int, [_P, C.c_uint64]),
    "grl_gnet_predict": (C.c_int, [_P, _I, _P, _P, _P, _P, _P, _P]),
    "grl_gnet_train": (C.c_int, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _F, _F, _I, _P]),
    "grl_gnet_rollout": (C.c_int, [_P, _I]),
    "grl_gnet_train_rollout": (C.c_int, [_P, _F, _P]),
    "grl_gnet_read_rollout": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}
# include/goldsrl_gatedeval.h: a dict of its own, as the header is a file of its own (GNET_SIGNATURES is pinned to goldsrl_gatednet.h's
# 17 training functions by tests/test_oracle_gated.py; these three are pinned by tests/test_gated_eval_header.py)
GNET_EVAL_SIGNATURES = {
    "grl_gnet_set_greedy": (C.c_int, [_P, _I]),
    "grl_gnet_eval": (C.c_int, [_P, _I, _I]),
    "grl_gnet_read_eval": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}


def gated_param_shapes(static_size=STATIC_SIZE, temporal_size=TEMPORAL_SIZE, H=32, S=128):
    """tf.trainable_variables() order: the trunk (the flat net's first ten blocks), the class tower, the normal tower, the value head."""
    X = 3 * H
    return [
        ("gru_gates_w", (temporal_size + H, 2 * H)), ("gru_gates_b", (2 * H,)), ("gru_cand_w", (temporal_size + H, H)), ("gru_cand_b", (H,)),
        ("temporal_w", (H, 2 * H)), ("temporal_b", (2 * H,)), ("static1_w", (static_size, 2 * H)), ("static1_b", (2 * H,)),
        ("static2_w", (2 * H, H)), ("static2_b", (H,)),
        ("class1_w", (X, 2 * S)), ("class1_b", (2 * S,)), ("class2_w", (2 * S, S)), ("class2_b", (S,)),
        ("class3_w", (S, N_ASSETS * N_CHOICES)), ("class3_b", (N_ASSETS * N_CHOICES,)),
        ("normal1_w", (X, 2 * S)), ("normal1_b", (2 * S,)), ("normal2_w", (2 * S, S)), ("normal2_b", (S,)),
        ("normal3_w", (S, N_ASSETS * N_CHOICES * 2)), ("normal3_b", (N_ASSETS * N_CHOICES * 2,)),
        ("value1_w", (X, 2 * S)), ("value1_b", (2 * S,)), ("value2_w", (2 * S, 1)), ("value2_b", (1,)),
    ]


def default_init_gated(seed=3):
    """flat_init's rule: glorot-uniform kernels, zero biases, GRU gate bias 1."""
    rng = np.random.RandomState(seed)
    parts = []
    for name, shape in gated_param_shapes():
        if name.endswith("_w"):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            parts.append(rng.uniform(-lim, lim, size=shape).reshape(-1))
        elif name == "gru_gates_b":
            parts.append(np.ones(shape))
        else:
            parts.append(np.zeros(shape))
    return np.concatenate(parts).astype(np.float32)


class GatedNet(object):
    """The gated trader on a Ticker Engine: predict / train on host samples, device-resident rollout + update."""

    def __init__(self, engine, **kw):
        self.lib = _ffi.load_library(extra_signatures=dict(GNET_SIGNATURES, **GNET_EVAL_SIGNATURES))
        self.eng = engine
        cfg = GrlGnetConfig()
        self.lib.grl_gnet_config_default(C.byref(cfg))
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError("unknown grl_gnet_config field %r" % k)
            setattr(cfg, k, v)
        self.cfg = cfg
        self.R = cfg.rnn_length
        n = C.c_void_p()
        rc = self.lib.grl_gnet_create(engine.h, C.byref(cfg), C.byref(n))
        if rc != _ffi.OK:
            raise _ffi.GrlError(rc, self.lib.grl_last_error(engine.h).decode())
        self.n = n
        self.num_params = int(self.lib.grl_gnet_num_params(n))
        self.T = 0

    def _check(self, rc):
        if rc != _ffi.OK:
            raise _ffi.GrlError(rc, self.lib.grl_gnet_last_error(self.n).decode())

    def close(self):
        if getattr(self, "n", None):
            self.lib.grl_gnet_destroy(self.n)
            self.n = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, flat):
        a = np.ascontiguousarray(flat, np.float32)
        self._check(self.lib.grl_gnet_set_params(self.n, _ffi._ptr(a), a.size))

    def get_params(self):
        a = np.empty(self.num_params, np.float32)
        self._check(self.lib.grl_gnet_get_params(self.n, _ffi._ptr(a), a.size))
        return a

    def get_grads(self, which="policy"):
        a = np.empty(self.num_params, np.float32)
        self._check(self.lib.grl_gnet_get_grads(self.n, {"policy": 0, "value": 1}[which], _ffi._ptr(a), a.size))
        return a

    def get_optimizer_state(self):
        msp, msv = np.empty(self.num_params, np.float32), np.empty(self.num_params, np.float32)
        step = C.c_int64(0)
        self._check(self.lib.grl_gnet_get_optimizer_state(self.n, _ffi._ptr(msp), _ffi._ptr(msv), msp.size, C.byref(step)))
        return {"ms_policy": msp, "ms_value": msv, "global_step": int(step.value)}

    def set_optimizer_state(self, ms_policy, ms_value, global_step):
        a, b = np.ascontiguousarray(ms_policy, np.float32), np.ascontiguousarray(ms_value, np.float32)
        self._check(self.lib.grl_gnet_set_optimizer_state(self.n, _ffi._ptr(a), _ffi._ptr(b), a.size, int(global_step)))

    def get_action_counter(self):
        v = C.c_uint64(0)
        self._check(self.lib.grl_gnet_get_action_counter(self.n, C.byref(v)))
        return int(v.value)

    def set_action_counter(self, value):
        self._check(self.lib.grl_gnet_set_action_counter(self.n, int(value)))

    def save_checkpoint(self, path, **extra):
        """Parameters, both RMSProp ms vectors, the global step and the action counter (.npz), plus the caller's scalars."""
        st = self.get_optimizer_state()
        np.savez(path, params=self.get_params(), ms_policy=st["ms_policy"], ms_value=st["ms_value"], global_step=st["global_step"],
                 action_counter=self.get_action_counter(), **{k: np.asarray(v) for k, v in extra.items()})

    def load_checkpoint(self, path):
        with np.load(path) as z:
            self.set_params(z["params"])
            self.set_optimizer_state(z["ms_policy"], z["ms_value"], int(z["global_step"]))
            self.set_action_counter(int(z["action_counter"]))
            return {k: z[k] for k in z.files if k not in ("params", "ms_policy", "ms_value", "global_step", "action_counter")}

    def predict(self, states, windows):
        s = np.ascontiguousarray(states, np.float32)
        w = np.ascontiguousarray(windows, np.float32)
        n = s.shape[0]
        assert s.shape == (n, STATIC_SIZE) and w.shape == (n, self.R, TEMPORAL_SIZE), (s.shape, w.shape)
        probs, mu, sigma = [np.empty((n, N_ASSETS, N_CHOICES), np.float32) for _ in range(3)]
        vals = np.empty(n, np.float32)
        self._check(self.lib.grl_gnet_predict(self.n, n, _ffi._ptr(s), _ffi._ptr(w), _ffi._ptr(probs), _ffi._ptr(mu), _ffi._ptr(sigma),
                                              _ffi._ptr(vals)))
        return {"probs": probs, "mu": mu, "sigma": sigma, "values": vals}

    def train(self, states, windows, choices, raw, adv, targets, weights=None, grad_mult=1.0, lr=1e-4, apply_update=True):
        s = np.ascontiguousarray(states, np.float32)
        n = s.shape[0]
        w = np.ascontiguousarray(windows, np.float32)
        ch = np.ascontiguousarray(choices, np.int32)
        arrs = [np.ascontiguousarray(a, np.float32) for a in (raw, adv, targets)]
        assert w.shape == (n, self.R, TEMPORAL_SIZE) and ch.shape == (n, N_ASSETS) and arrs[0].shape == (n, N_ASSETS)
        wt = None if weights is None else np.ascontiguousarray(weights, np.float32)
        stats = np.zeros(6, np.float32)
        self._check(self.lib.grl_gnet_train(self.n, n, _ffi._ptr(s), _ffi._ptr(w), _ffi._ptr(ch), *[_ffi._ptr(a) for a in arrs],
                                            None if wt is None else _ffi._ptr(wt), float(grad_mult), float(lr), 1 if apply_update else 0,
                                            _ffi._ptr(stats)))
        return dict(zip(STAT_NAMES, stats.tolist()))

    def rollout(self, T):
        self._check(self.lib.grl_gnet_rollout(self.n, int(T)))
        self.T = int(T)

    def train_rollout(self, lr=1e-4):
        stats = np.zeros(6, np.float32)
        self._check(self.lib.grl_gnet_train_rollout(self.n, float(lr), _ffi._ptr(stats)))
        return dict(zip(STAT_NAMES, stats.tolist()))

    def read_rollout(self, which):
        T, E, R = self.T, self.eng.E, self.R
        shapes = {"states": (T, E, STATIC_SIZE), "windows": (T, E, R, TEMPORAL_SIZE), "choices": (T, E, N_ASSETS), "raw": (T, E, N_ASSETS),
                  "probs": (T, E, N_ASSETS, N_CHOICES), "mu": (T, E, N_ASSETS, N_CHOICES), "sigma": (T, E, N_ASSETS, N_CHOICES),
                  "values": (T, E), "rewards": (T, E), "dones": (T, E), "weights": (T, E), "adv": (T, E), "targets": (T, E),
                  "actions": (T, E, 2 * N_ASSETS), "boot": (E,)}
        a = np.empty(shapes[which], np.int32 if which == "choices" else np.float32)
        self._check(self.lib.grl_gnet_read_rollout(self.n, which.encode(), _ffi._ptr(a), a.nbytes))
        return a

    def set_greedy(self, on):
        """on: rollout draws nothing -- per asset the choice is the first argmax of the float32 probs, raw = mu[choice]; the action
        counter stands still."""
        self._check(self.lib.grl_gnet_set_greedy(self.n, 1 if on else 0))

    EVAL_TRACE = ("states", "probs", "mu", "choices", "actions", "rewards", "dones")

    def eval(self, max_steps, trace_steps=0, trace_fields=EVAL_TRACE):
        """Greedy episodes of every env from the engine's current state (reset it first), one kernel launch; the engine is reset
        afterwards.  Returns total_reward (E) float64, length (E) int32, finished (E) uint8 and, with trace_steps > 0, states (S,E,7),
        probs, mu (S,E,2,3), choices (S,E,2) int32, actions (S,E,4), rewards, dones (S,E) of the first S = min(trace_steps, steps
        played) steps, each defined up to its env's own end (trace_fields: the ones to read back)."""
        self._check(self.lib.grl_gnet_eval(self.n, int(max_steps), int(trace_steps)))
        E = self.eng.E
        out = {"total_reward": np.empty(E, np.float64), "length": np.empty(E, np.int32), "finished": np.empty(E, np.uint8)}
        for k in ("total_reward", "length", "finished"):
            self._check(self.lib.grl_gnet_read_eval(self.n, k.encode(), _ffi._ptr(out[k]), out[k].nbytes))
        if trace_steps > 0:
            S = min(int(trace_steps), int(max_steps), int(out["length"].max()))
            tails = {"states": (STATIC_SIZE,), "probs": (N_ASSETS, N_CHOICES), "mu": (N_ASSETS, N_CHOICES), "choices": (N_ASSETS,),
                     "actions": (2 * N_ASSETS,), "rewards": (), "dones": ()}
            for k in trace_fields:
                out[k] = np.empty((S, E) + tails[k], np.int32 if k == "choices" else np.float32)
                self._check(self.lib.grl_gnet_read_eval(self.n, k.encode(), _ffi._ptr(out[k]), out[k].nbytes))
        return out
