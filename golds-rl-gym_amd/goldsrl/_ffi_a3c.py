"""What the ctypes bindings of the three A3C nets share (GatedNet in _ffi_gated.py, GaussNet in _ffi_gauss.py, DiscreteNet in
_ffi_discrete.py): the three C ABIs name the same functions behind another prefix (grl_gnet_ / grl_anet_ / grl_dnet_), with their
heads' arrays in predict and train."""
import ctypes as C

import numpy as np

from . import _ffi

STAT_NAMES = ("policy_loss", "value_loss", "entropy_mean", "policy_norm", "value_norm", "lr")
_CHECKPOINT = ("params", "ms_policy", "ms_value", "global_step", "action_counter")
_P, _I, _F, _SZ = C.c_void_p, C.c_int32, C.c_float, C.c_size_t


def signatures(prefix, config, predict, train):
    """The signature dicts of one net's two headers, (training: 17 functions, evaluation: 3).  predict: the output arrays of
    grl_*net_predict behind (net, n, states, windows); train: the input arrays of grl_*net_train between windows and weights."""
    cfg = C.POINTER(config)
    training = {
        "config_default": (C.c_int, [cfg]),
        "create": (C.c_int, [_P, cfg, C.POINTER(_P)]),
        "destroy": (C.c_int, [_P]),
        "last_error": (C.c_char_p, [_P]),
        "num_params": (C.c_int64, [_P]),
        "set_params": (C.c_int, [_P, _P, C.c_int64]),
        "get_params": (C.c_int, [_P, _P, C.c_int64]),
        "get_grads": (C.c_int, [_P, _I, _P, C.c_int64]),
        "get_optimizer_state": (C.c_int, [_P, _P, _P, C.c_int64, C.POINTER(C.c_int64)]),
        "set_optimizer_state": (C.c_int, [_P, _P, _P, C.c_int64, C.c_int64]),
        "get_action_counter": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
        "set_action_counter": (C.c_int, [_P, C.c_uint64]),
        "predict": (C.c_int, [_P, _I, _P, _P] + [_P] * len(predict)),
        "train": (C.c_int, [_P, _I, _P, _P] + [_P] * len(train) + [_P, _F, _F, _I, _P]),      # .., weights, grad_mult, lr0, apply, stats
        "rollout": (C.c_int, [_P, _I]),
        "train_rollout": (C.c_int, [_P, _F, _P]),
        "read_rollout": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
    }
    evaluation = {"set_greedy": (C.c_int, [_P, _I]), "eval": (C.c_int, [_P, _I, _I]), "read_eval": (C.c_int, [_P, C.c_char_p, _P, _SZ])}
    return {prefix + k: v for k, v in training.items()}, {prefix + k: v for k, v in evaluation.items()}


class A3cNet(object):
    PREFIX = None       # "grl_gnet_" / "grl_anet_" / "grl_dnet_"
    # set by the net: S0, D (the widths of a state and of a window row) and R

    def _create(self, engine, signatures, cfg, kw):
        """The net on the engine's handle from the C defaults overridden by kw."""
        self.lib = _ffi.load_library(extra_signatures=signatures)
        self.eng = engine
        self._fn("config_default")(C.byref(cfg))
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError("unknown %sconfig field %r" % (self.PREFIX, k))
            setattr(cfg, k, v)
        self.cfg = cfg
        self.R = cfg.rnn_length
        n = C.c_void_p()
        rc = self._fn("create")(engine.h, C.byref(cfg), C.byref(n))
        if rc != _ffi.OK:
            raise _ffi.GrlError(rc, self.lib.grl_last_error(engine.h).decode())
        self.n = n
        self.num_params = int(self._fn("num_params")(n))
        self.T = 0

    def _fn(self, name):
        return getattr(self.lib, self.PREFIX + name)

    def _check(self, rc):
        if rc != _ffi.OK:
            raise _ffi.GrlError(rc, self._fn("last_error")(self.n).decode())

    def close(self):
        if getattr(self, "n", None):
            self._fn("destroy")(self.n)
            self.n = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_params(self, flat):
        a = np.ascontiguousarray(flat, np.float32)
        self._check(self._fn("set_params")(self.n, _ffi._ptr(a), a.size))

    def get_params(self):
        a = np.empty(self.num_params, np.float32)
        self._check(self._fn("get_params")(self.n, _ffi._ptr(a), a.size))
        return a

    def get_grads(self, which="policy"):
        a = np.empty(self.num_params, np.float32)
        self._check(self._fn("get_grads")(self.n, {"policy": 0, "value": 1}[which], _ffi._ptr(a), a.size))
        return a

    def get_optimizer_state(self):
        msp, msv = np.empty(self.num_params, np.float32), np.empty(self.num_params, np.float32)
        step = C.c_int64(0)
        self._check(self._fn("get_optimizer_state")(self.n, _ffi._ptr(msp), _ffi._ptr(msv), msp.size, C.byref(step)))
        return {"ms_policy": msp, "ms_value": msv, "global_step": int(step.value)}

    def set_optimizer_state(self, ms_policy, ms_value, global_step):
        a, b = np.ascontiguousarray(ms_policy, np.float32), np.ascontiguousarray(ms_value, np.float32)
        self._check(self._fn("set_optimizer_state")(self.n, _ffi._ptr(a), _ffi._ptr(b), a.size, int(global_step)))

    def get_action_counter(self):
        v = C.c_uint64(0)
        self._check(self._fn("get_action_counter")(self.n, C.byref(v)))
        return int(v.value)

    def set_action_counter(self, value):
        self._check(self._fn("set_action_counter")(self.n, int(value)))

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
            return {k: z[k] for k in z.files if k not in _CHECKPOINT}

    def _stage(self, states, windows):
        """n and the float32 states (n,S0) and windows (n,R,D) of a predict or train call"""
        s, w = np.ascontiguousarray(states, np.float32), np.ascontiguousarray(windows, np.float32)
        n = s.shape[0]
        assert s.shape == (n, self.S0) and w.shape == (n, self.R, self.D), (s.shape, w.shape)
        return n, s, w

    def _predict(self, states, windows, heads):
        """grl_*net_predict: heads = (name, shape behind n) of the output arrays in the C order, before values."""
        n, s, w = self._stage(states, windows)
        out = {k: np.empty((n,) + tail, np.float32) for k, tail in heads + (("values", ()),)}
        self._check(self._fn("predict")(self.n, n, _ffi._ptr(s), _ffi._ptr(w), *[_ffi._ptr(a) for a in out.values()]))
        return out

    def _train(self, states, windows, heads, adv, targets, weights, grad_mult, lr, apply_update):
        """grl_*net_train: heads = (array, dtype, shape behind n) of the net's own inputs in the C order; the six stats by name."""
        n, s, w = self._stage(states, windows)
        arrs = [np.ascontiguousarray(a, dt) for a, dt, _ in heads] + [np.ascontiguousarray(a, np.float32) for a in (adv, targets)]
        assert [a.shape for a in arrs] == [(n,) + tail for _, _, tail in heads] + [(n,), (n,)], [a.shape for a in arrs]
        wt = None if weights is None else np.ascontiguousarray(weights, np.float32)
        stats = np.zeros(6, np.float32)
        self._check(self._fn("train")(self.n, n, _ffi._ptr(s), _ffi._ptr(w), *[_ffi._ptr(a) for a in arrs], None if wt is None else _ffi._ptr(wt),
                                      float(grad_mult), float(lr), 1 if apply_update else 0, _ffi._ptr(stats)))
        return dict(zip(STAT_NAMES, stats.tolist()))

    def rollout(self, T):
        self._check(self._fn("rollout")(self.n, int(T)))
        self.T = int(T)

    def train_rollout(self, lr=1e-4):
        stats = np.zeros(6, np.float32)
        self._check(self._fn("train_rollout")(self.n, float(lr), _ffi._ptr(stats)))
        return dict(zip(STAT_NAMES, stats.tolist()))

    def _read(self, fn, which, shape):
        a = np.empty(shape, np.int32 if which == "choices" else np.float32)
        self._check(self._fn(fn)(self.n, which.encode(), _ffi._ptr(a), a.nbytes))
        return a

    def set_greedy(self, on):
        """on: rollout draws nothing and acts by the net's greedy rule (see the class); the action counter stands still."""
        self._check(self._fn("set_greedy")(self.n, 1 if on else 0))

    def _eval(self, max_steps, trace_steps, trace_fields, tails):
        """grl_*net_eval and its read-back: the per-env results, then the trace fields asked for, (S,E) + tails[field]."""
        self._check(self._fn("eval")(self.n, int(max_steps), int(trace_steps)))
        E = self.eng.E
        out = {"total_reward": np.empty(E, np.float64), "length": np.empty(E, np.int32), "finished": np.empty(E, np.uint8)}
        for k in ("total_reward", "length", "finished"):
            self._check(self._fn("read_eval")(self.n, k.encode(), _ffi._ptr(out[k]), out[k].nbytes))
        if trace_steps > 0:
            S = min(int(trace_steps), int(max_steps), int(out["length"].max()))
            for k in trace_fields:
                out[k] = self._read("read_eval", k, (S, E) + tails[k])
        return out
