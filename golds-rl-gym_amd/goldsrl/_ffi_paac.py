"""What the ctypes bindings of the three PAAC nets share (ConvNet in _ffi_net.py, FlatNet in _ffi_flat.py, FieldNet in _ffi_field.py):
the three C ABIs name the same functions behind another prefix (grl_net_ / grl_fnet_ / grl_fieldnet_)."""
import ctypes as C

import numpy as np

from . import _ffi

STAT_NAMES = ("loss", "policy_loss", "critic_loss_mean", "global_norm")
_CHECKPOINT = ("params", "adam_m", "adam_v", "adam_step", "action_counter")


def glorot_uniform_flat(shapes, seed):
    """tf.layers defaults over (name, shape) pairs: glorot-uniform kernels (*_w), zero biases -> flat float32 vector."""
    rng = np.random.RandomState(seed)
    parts = []
    for name, shape in shapes:
        if name.endswith("_w"):
            if len(shape) == 2:
                fan_in, fan_out = shape
            else:
                rf = int(np.prod(shape[:-2]))
                fan_in, fan_out = rf * shape[-2], rf * shape[-1]
            lim = np.sqrt(6.0 / (fan_in + fan_out))
            parts.append(rng.uniform(-lim, lim, size=shape).reshape(-1))
        else:
            parts.append(np.zeros(int(np.prod(shape))))
    return np.concatenate(parts).astype(np.float32)


class PaacNet(object):
    """What all three nets have: the handle, the error check and the flat copies."""
    PREFIX = None       # "grl_net_" / "grl_fnet_" / "grl_fieldnet_"

    def _create(self, engine, signatures, cfg, kw, *default_args):
        """The net on the engine's handle from the C defaults (default_args: what config_default takes in front of the struct)
        overridden by kw."""
        self.lib = _ffi.load_library(extra_signatures=signatures)
        self.eng = engine
        rc = self._fn("config_default")(*(default_args + (C.byref(cfg),)))
        if rc != _ffi.OK:
            raise _ffi.GrlError(rc, self.PREFIX + "config_default")
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError("unknown %sconfig field %r" % (self.PREFIX, k))
            setattr(cfg, k, v)
        self.cfg = cfg
        n = C.c_void_p()
        rc = self._fn("create")(engine.h, C.byref(cfg), C.byref(n))
        if rc != _ffi.OK:
            raise _ffi.GrlError(rc, self.lib.grl_last_error(engine.h).decode())
        self.n = n
        self.num_params = int(self._fn("num_params")(n))

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

    def get_grads(self):
        a = np.empty(self.num_params, np.float32)
        self._check(self._fn("get_grads")(self.n, _ffi._ptr(a), a.size))
        return a

    def _stats4(self, name, *args):
        """grl_*_<name>(net, args.., stats): the four stats by name."""
        stats = np.zeros(4, np.float32)
        self._check(self._fn(name)(self.n, *(args + (_ffi._ptr(stats),))))
        return dict(zip(STAT_NAMES, stats.tolist()))


class PaacRolloutNet(PaacNet):
    """What the nets that act and train over rollouts on the device have (ConvNet, FlatNet, FieldNet)."""

    def get_optimizer_state(self):
        """Adam moments and the number of updates applied: with the parameters, the estimator's whole training state."""
        m, v = np.empty(self.num_params, np.float32), np.empty(self.num_params, np.float32)
        step = C.c_int64(0)
        self._check(self._fn("get_optimizer_state")(self.n, _ffi._ptr(m), _ffi._ptr(v), m.size, C.byref(step)))
        return {"adam_m": m, "adam_v": v, "adam_step": int(step.value)}

    def set_optimizer_state(self, adam_m, adam_v, adam_step):
        m, v = np.ascontiguousarray(adam_m, np.float32), np.ascontiguousarray(adam_v, np.float32)
        self._check(self._fn("set_optimizer_state")(self.n, _ffi._ptr(m), _ffi._ptr(v), m.size, int(adam_step)))

    def get_action_counter(self):
        v = C.c_uint64(0)
        self._check(self._fn("get_action_counter")(self.n, C.byref(v)))
        return int(v.value)

    def set_action_counter(self, value):
        self._check(self._fn("set_action_counter")(self.n, int(value)))

    def save_checkpoint(self, path, **extra):
        """Flat-weights checkpoint (.npz): parameters in tf.trainable_variables() order, Adam state, caller's scalars."""
        st = self.get_optimizer_state()
        np.savez(path, params=self.get_params(), adam_m=st["adam_m"], adam_v=st["adam_v"], adam_step=st["adam_step"], action_counter=self.get_action_counter(),
                 **{k: np.asarray(v) for k, v in extra.items()})

    def load_checkpoint(self, path):
        with np.load(path) as z:
            self.set_params(z["params"])
            self.set_optimizer_state(z["adam_m"], z["adam_v"], int(z["adam_step"]))
            if "action_counter" in z.files:      # the action-noise stream continues where the saved run stopped
                self.set_action_counter(int(z["action_counter"]))
            return {k: z[k] for k in z.files if k not in _CHECKPOINT}

    def train_rollout(self, lr):
        return self._stats4("train_rollout", lr)

    def train_rollout_grads(self):
        """Loss + backward over the last rollout only: the local mean gradient stays in the net (get_grads)."""
        return self._stats4("train_rollout_grads")


class PaacTrainerNet(PaacRolloutNet):
    """What the two nets that also train over ranks have (ConvNet, FlatNet)."""

    def set_grads(self, flat):
        a = np.ascontiguousarray(flat, np.float32)
        self._check(self._fn("set_grads")(self.n, _ffi._ptr(a), a.size))

    def apply_grads(self, lr, grad_scale=1.0):
        """clip_by_global_norm(grad_scale * grads) + Adam(lr) on the gradient currently in the net."""
        return self._stats4("apply_grads", lr, grad_scale)

    # -- multi-GPU (RCCL): rank 0 makes the id, everybody attaches; one all-reduce of the flat gradient per rollout
    def comm_unique_id(self):
        n = int(self.lib.grl_comm_unique_id_bytes())
        buf = np.zeros(n, np.uint8)
        rc = self.lib.grl_comm_unique_id(_ffi._ptr(buf), n)
        if rc != _ffi.OK:
            raise _ffi.GrlError(rc, "grl_comm_unique_id")
        return buf

    def comm_init(self, unique_id, rank, world_size):
        buf = np.ascontiguousarray(unique_id, np.uint8)
        self._check(self._fn("comm_init")(self.n, _ffi._ptr(buf), buf.size, rank, world_size))

    def comm_broadcast_params(self, root=0):
        self._check(self._fn("comm_broadcast_params")(self.n, root))

    def comm_info(self):
        """What RCCL reports for the attached communicator (ranks = ncclCommCount, 0 without one) and the all-reduce timing."""
        cnt, ur, calls, tot, last = C.c_int32(), C.c_int32(), C.c_int64(), C.c_double(), C.c_float()
        self._check(self._fn("comm_info")(self.n, C.byref(cnt), C.byref(ur), C.byref(calls), C.byref(tot), C.byref(last)))
        return {"rccl_ranks": cnt.value, "rccl_user_rank": ur.value, "allreduce_calls": calls.value,
                "allreduce_ms_total": tot.value, "allreduce_ms_last": last.value}

    def comm_destroy(self):
        self._check(self._fn("comm_destroy")(self.n))
