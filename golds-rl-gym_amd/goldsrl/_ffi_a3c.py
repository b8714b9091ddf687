"""What the ctypes bindings of the two A3C nets share (GatedNet in _ffi_gated.py, GaussNet in _ffi_gauss.py): the two C ABIs name the
same functions behind another prefix (grl_gnet_ / grl_anet_)."""
import ctypes as C

import numpy as np

from . import _ffi

STAT_NAMES = ("policy_loss", "value_loss", "entropy_mean", "policy_norm", "value_norm", "lr")
_CHECKPOINT = ("params", "ms_policy", "ms_value", "global_step", "action_counter")


class A3cNet(object):
    PREFIX = None       # "grl_gnet_" / "grl_anet_"

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

    def _train(self, *arrays_and_scalars):
        """grl_*net_train on pointers / scalars in the C order; the six stats by name."""
        stats = np.zeros(6, np.float32)
        self._check(self._fn("train")(self.n, *(arrays_and_scalars + (_ffi._ptr(stats),))))
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
