"""ctypes binding of the A3C Gaussian agent on the device (SolowWorker / TradeWorker; C ABI: include/goldsrl_gaussnet.h)."""
import ctypes as C

import numpy as np

from . import _ffi

_P, _I, _F, _SZ = C.c_void_p, C.c_int32, C.c_float, C.c_size_t

STAT_NAMES = ("policy_loss", "value_loss", "entropy_mean", "policy_norm", "value_norm", "lr")
SOLOW_SIZES = dict(static_size=2, temporal_size=2, num_actions=1)       # scripts/train_solow.py:40-42
TRADE_SIZES = dict(static_size=5, temporal_size=5, num_actions=2)       # scripts/train_trade.py (2 assets)


class GrlAnetConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("rnn_length", C.c_int32), ("max_samples", C.c_int32), ("lr_decay_steps", C.c_int32),
                ("always_bootstrap", C.c_int32), ("scale", C.c_float), ("gamma", C.c_float), ("gae_lambda", C.c_float),
                ("clip_norm", C.c_float), ("rms_decay", C.c_float), ("rms_epsilon", C.c_float), ("lr_decay_rate", C.c_float)]


ANET_SIGNATURES = {
    "grl_anet_config_default": (C.c_int, [C.POINTER(GrlAnetConfig)]),
    "grl_anet_create": (C.c_int, [_P, C.POINTER(GrlAnetConfig), C.POINTER(_P)]),
    "grl_anet_destroy": (C.c_int, [_P]),
    "grl_anet_last_error": (C.c_char_p, [_P]),
    "grl_anet_num_params": (C.c_int64, [_P]),
    "grl_anet_set_params": (C.c_int, [_P, _P, C.c_int64]),
    "grl_anet_get_params": (C.c_int, [_P, _P, C.c_int64]),
    "grl_anet_get_grads": (C.c_int, [_P, _I, _P, C.c_int64]),
    "grl_anet_get_optimizer_state": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
    "grl_anet_set_optimizer_state": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64]),
    "grl_anet_get_action_counter": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "grl_anet_set_action_counter": (C.c_int, [_P, C.c_uint64]),
    "grl_anet_predict": (C.c_int, [_P, _I, _P, _P, _P, _P, _P]),
    "grl_anet_train": (C.c_int, [_P, _I, _P, _P, _P, _P, _P, _P, _F, _F, _I, _P]),
    "grl_anet_rollout": (C.c_int, [_P, _I]),
    "grl_anet_train_rollout": (C.c_int, [_P, _F, _P]),
    "grl_anet_read_rollout": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}
# include/goldsrl_gausseval.h: a dict of its own, as the header is a file of its own (ANET_SIGNATURES is pinned to goldsrl_gaussnet.h's
# 17 training functions by tests/test_oracle_gauss.py; these three are pinned by tests/test_gauss_eval_header.py)
ANET_EVAL_SIGNATURES = {
    "grl_anet_set_greedy": (C.c_int, [_P, _I]),
    "grl_anet_eval": (C.c_int, [_P, _I, _I]),
    "grl_anet_read_eval": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}


def gauss_param_shapes(static_size=2, temporal_size=2, num_actions=1, H=32, S=128):
    """tf.trainable_variables() order of scripts/train_solow.py:63-73: the trunk (the flat net's first ten blocks), the mu tower, the
    sigma tower, the value head."""
    X = 3 * H
    return [
        ("gru_gates_w", (temporal_size + H, 2 * H)), ("gru_gates_b", (2 * H,)), ("gru_cand_w", (temporal_size + H, H)), ("gru_cand_b", (H,)),
        ("temporal_w", (H, 2 * H)), ("temporal_b", (2 * H,)), ("static1_w", (static_size, 2 * H)), ("static1_b", (2 * H,)),
        ("static2_w", (2 * H, H)), ("static2_b", (H,)),
        ("mu1_w", (X, 2 * S)), ("mu1_b", (2 * S,)), ("mu2_w", (2 * S, S)), ("mu2_b", (S,)), ("mu3_w", (S, num_actions)), ("mu3_b", (num_actions,)),
        ("sigma1_w", (X, 2 * S)), ("sigma1_b", (2 * S,)), ("sigma2_w", (2 * S, S)), ("sigma2_b", (S,)),
        ("sigma3_w", (S, num_actions)), ("sigma3_b", (num_actions,)),
        ("value1_w", (X, 2 * S)), ("value1_b", (2 * S,)), ("value2_w", (2 * S, 1)), ("value2_b", (1,)),
    ]


def default_init_gauss(seed=3, static_size=2, temporal_size=2, num_actions=1):
    """TF's defaults: glorot-uniform kernels, zero biases; the sigma3 bias at -1 (a3c/estimators.py:289); the GRU as
    default_init_gated does it (gate bias 1)."""
    rng = np.random.RandomState(seed)
    parts = []
    for name, shape in gauss_param_shapes(static_size, temporal_size, num_actions):
        if name.endswith("_w"):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            parts.append(rng.uniform(-lim, lim, size=shape).reshape(-1))
        elif name == "gru_gates_b":
            parts.append(np.ones(shape))
        elif name == "sigma3_b":
            parts.append(-np.ones(shape))
        else:
            parts.append(np.zeros(shape))
    return np.concatenate(parts).astype(np.float32)


class GaussNet(object):
    """The Gaussian agent on a Solow or 2-asset TradeAR1 Engine: predict / train on host samples, device-resident rollout + update.
    always_bootstrap defaults to what the engine's env takes (Solow 1, TradeAR1 0)."""

    def __init__(self, engine, **kw):
        self.lib = _ffi.load_library(extra_signatures=dict(ANET_SIGNATURES, **ANET_EVAL_SIGNATURES))
        self.eng = engine
        cfg = GrlAnetConfig()
        self.lib.grl_anet_config_default(C.byref(cfg))
        kw.setdefault("always_bootstrap", 1 if engine.kind == _ffi.ENV_SOLOW else 0)
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError("unknown grl_anet_config field %r" % k)
            setattr(cfg, k, v)
        self.cfg = cfg
        self.R = cfg.rnn_length
        n = C.c_void_p()
        rc = self.lib.grl_anet_create(engine.h, C.byref(cfg), C.byref(n))
        if rc != _ffi.OK:
            raise _ffi.GrlError(rc, self.lib.grl_last_error(engine.h).decode())
        self.n = n
        self.sizes = dict(SOLOW_SIZES if engine.kind == _ffi.ENV_SOLOW else TRADE_SIZES)
        self.S0, self.D, self.A = self.sizes["static_size"], self.sizes["temporal_size"], self.sizes["num_actions"]
        self.num_params = int(self.lib.grl_anet_num_params(n))
        self.T = 0

    def _check(self, rc):
        if rc != _ffi.OK:
            raise _ffi.GrlError(rc, self.lib.grl_anet_last_error(self.n).decode())

    def close(self):
        if getattr(self, "n", None):
            self.lib.grl_anet_destroy(self.n)
            self.n = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, flat):
        a = np.ascontiguousarray(flat, np.float32)
        self._check(self.lib.grl_anet_set_params(self.n, _ffi._ptr(a), a.size))

    def get_params(self):
        a = np.empty(self.num_params, np.float32)
        self._check(self.lib.grl_anet_get_params(self.n, _ffi._ptr(a), a.size))
        return a

    def get_grads(self, which="policy"):
        a = np.empty(self.num_params, np.float32)
        self._check(self.lib.grl_anet_get_grads(self.n, {"policy": 0, "value": 1}[which], _ffi._ptr(a), a.size))
        return a

    def get_optimizer_state(self):
        msp, msv = np.empty(self.num_params, np.float32), np.empty(self.num_params, np.float32)
        step = C.c_int64(0)
        self._check(self.lib.grl_anet_get_optimizer_state(self.n, _ffi._ptr(msp), _ffi._ptr(msv), msp.size, C.byref(step)))
        return {"ms_policy": msp, "ms_value": msv, "global_step": int(step.value)}

    def set_optimizer_state(self, ms_policy, ms_value, global_step):
        a, b = np.ascontiguousarray(ms_policy, np.float32), np.ascontiguousarray(ms_value, np.float32)
        self._check(self.lib.grl_anet_set_optimizer_state(self.n, _ffi._ptr(a), _ffi._ptr(b), a.size, int(global_step)))

    def get_action_counter(self):
        v = C.c_uint64(0)
        self._check(self.lib.grl_anet_get_action_counter(self.n, C.byref(v)))
        return int(v.value)

    def set_action_counter(self, value):
        self._check(self.lib.grl_anet_set_action_counter(self.n, int(value)))

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
        assert s.shape == (n, self.S0) and w.shape == (n, self.R, self.D), (s.shape, w.shape)
        mu, sigma = np.empty((n, self.A), np.float32), np.empty((n, self.A), np.float32)
        vals = np.empty(n, np.float32)
        self._check(self.lib.grl_anet_predict(self.n, n, _ffi._ptr(s), _ffi._ptr(w), _ffi._ptr(mu), _ffi._ptr(sigma), _ffi._ptr(vals)))
        return {"mu": mu, "sigma": sigma, "values": vals}

    def train(self, states, windows, raw, adv, targets, weights=None, grad_mult=1.0, lr=1e-4, apply_update=True):
        s = np.ascontiguousarray(states, np.float32)
        n = s.shape[0]
        w = np.ascontiguousarray(windows, np.float32)
        arrs = [np.ascontiguousarray(a, np.float32) for a in (raw, adv, targets)]
        assert s.shape == (n, self.S0) and w.shape == (n, self.R, self.D) and arrs[0].shape == (n, self.A)
        assert arrs[1].shape == (n,) and arrs[2].shape == (n,)
        wt = None if weights is None else np.ascontiguousarray(weights, np.float32)
        stats = np.zeros(6, np.float32)
        self._check(self.lib.grl_anet_train(self.n, n, _ffi._ptr(s), _ffi._ptr(w), *[_ffi._ptr(a) for a in arrs],
                                            None if wt is None else _ffi._ptr(wt), float(grad_mult), float(lr), 1 if apply_update else 0,
                                            _ffi._ptr(stats)))
        return dict(zip(STAT_NAMES, stats.tolist()))

    def rollout(self, T):
        self._check(self.lib.grl_anet_rollout(self.n, int(T)))
        self.T = int(T)

    def train_rollout(self, lr=1e-4):
        stats = np.zeros(6, np.float32)
        self._check(self.lib.grl_anet_train_rollout(self.n, float(lr), _ffi._ptr(stats)))
        return dict(zip(STAT_NAMES, stats.tolist()))

    def read_rollout(self, which):
        T, E, R, D, A = self.T, self.eng.E, self.R, self.D, self.A
        shapes = {"states": (T, E, self.S0), "windows": (T, E, R, D), "raw": (T, E, A), "mu": (T, E, A), "sigma": (T, E, A), "actions": (T, E, A),
                  "values": (T, E), "rewards": (T, E), "dones": (T, E), "weights": (T, E), "adv": (T, E), "targets": (T, E),
                  "term_values": (T, E), "term_states": (T, E, self.S0), "term_windows": (T, E, R, D), "boot": (E,)}
        a = np.empty(shapes[which], np.float32)
        self._check(self.lib.grl_anet_read_rollout(self.n, which.encode(), _ffi._ptr(a), a.nbytes))
        return a

    def set_greedy(self, on):
        """on: rollout draws nothing, raw = mu (run_n_steps(stochastic=False), a3c/worker.py:180-230); the action counter stands still."""
        self._check(self.lib.grl_anet_set_greedy(self.n, 1 if on else 0))

    EVAL_TRACE = ("states", "mu", "actions", "rewards", "dones")

    def eval(self, max_steps, trace_steps=0, trace_fields=EVAL_TRACE):
        """Greedy episodes of every env from the engine's current state (reset it first), one kernel launch; the engine is reset
        afterwards.  Returns total_reward (E) float64, length (E) int32, finished (E) uint8 and, with trace_steps > 0, states
        (S,E,S0), mu, actions (S,E,A), rewards, dones (S,E) of the first S = min(trace_steps, steps played) steps, each defined up to
        its env's own end (trace_fields: the ones to read back)."""
        self._check(self.lib.grl_anet_eval(self.n, int(max_steps), int(trace_steps)))
        E = self.eng.E
        out = {"total_reward": np.empty(E, np.float64), "length": np.empty(E, np.int32), "finished": np.empty(E, np.uint8)}
        for k in ("total_reward", "length", "finished"):
            self._check(self.lib.grl_anet_read_eval(self.n, k.encode(), _ffi._ptr(out[k]), out[k].nbytes))
        if trace_steps > 0:
            S = min(int(trace_steps), int(max_steps), int(out["length"].max()))
            tails = {"states": (self.S0,), "mu": (self.A,), "actions": (self.A,), "rewards": (), "dones": ()}
            for k in trace_fields:
                tail = tails[k]
                out[k] = np.empty((S, E) + tail, np.float32)
                self._check(self.lib.grl_anet_read_eval(self.n, k.encode(), _ffi._ptr(out[k]), out[k].nbytes))
        return out
