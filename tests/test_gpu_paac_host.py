"""The host surface the three PAAC nets share behind their prefixes (grl_net_ conv, grl_fnet_ flat, grl_fieldnet_ field): what each
refuses, with which code and which message, and the small state it keeps (action counter, communicator).  Every refusal is argument
validation on the host; the expected strings are the C sources'.  Called through the C symbols so that a wrong length can be passed
to the getters too."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NETS = ("conv", "flat", "field")
PREFIX = {"conv": "grl_net_", "flat": "grl_fnet_", "field": "grl_fieldnet_"}
# which messages carry the C function's name differs from net to net
SIZE_MSG = {
    "conv": {"set_params": "grl_net_set_params: ", "get_params": "", "get_grads": "", "set_grads": "grl_net_set_grads: ",
             "set_optimizer_state": "grl_net_set_optimizer_state: ", "get_optimizer_state": ""},
    "flat": {"set_params": "", "get_params": "", "get_grads": "", "set_grads": "", "set_optimizer_state": "", "get_optimizer_state": ""},
    "field": {"set_params": "", "get_params": "", "get_grads": ""},
}
NO_GRADS = {"conv": "grl_net_apply_grads: no gradient step has run yet", "flat": "grl_fnet_apply_grads: no gradient pass has run yet"}


@pytest.fixture(scope="module")
def nets():
    from goldsrl import _ffi, _ffi_field, _ffi_flat, _ffi_net
    swarm = _ffi.Engine(_ffi.ENV_SWARM, 2, seed=7)
    solow = _ffi.Engine(_ffi.ENV_SOLOW, 4, seed=7)
    swarm.reset(); solow.reset()
    out = {"conv": (swarm, _ffi_net.ConvNet(swarm, max_chunk_samples=20)),
           "flat": (solow, _ffi_flat.FlatNet(solow, max_samples=64)),
           "field": (solow, _ffi_field.FieldNet(solow, height=8, width=8, conv_layers=2, max_samples=5))}
    out["conv"][1].set_params(_ffi_net.glorot_uniform_flat(seed=3))
    out["flat"][1].set_params(_ffi_flat.default_init_flat(3))
    yield out
    for _, net in out.values():
        net.close()
    swarm.close(); solow.close()


def _call(net, kind, name, *args):
    """(return code, last error) of one C call"""
    rc = getattr(net.lib, PREFIX[kind] + name)(net.n, *args)
    return rc, getattr(net.lib, PREFIX[kind] + "last_error")(net.n).decode()


@pytest.mark.parametrize("kind", NETS)
def test_wrong_lengths_are_refused_with_the_size(nets, kind):
    from goldsrl import _ffi
    net = nets[kind][1]
    N = net.num_params
    before = net.get_params()
    for short in (N - 1, N + 1, 0):
        a, b = np.zeros(N + 1, np.float32), np.zeros(N + 1, np.float32)
        step = C.c_int64(0)
        calls = {"set_params": (_ffi._ptr(a), short), "get_params": (_ffi._ptr(a), short), "get_grads": (_ffi._ptr(a), short),
                 "set_grads": (_ffi._ptr(a), short), "set_optimizer_state": (_ffi._ptr(a), _ffi._ptr(b), short, 3),
                 "get_optimizer_state": (_ffi._ptr(a), _ffi._ptr(b), short, C.byref(step))}
        for name, lead in SIZE_MSG[kind].items():
            assert _call(net, kind, name, *calls[name]) == (_ffi.E_SIZE, "%sexpected %d floats" % (lead, N)), (name, short)
    assert np.array_equal(net.get_params(), before)
    if kind != "field":
        assert net.get_optimizer_state()["adam_step"] == 0      # the refused set_optimizer_state left the step alone
    # the Python methods raise the same
    with pytest.raises(_ffi.GrlError) as ei:
        net.set_params(np.zeros(N - 1, np.float32))
    assert ei.value.code == _ffi.E_SIZE and str(ei.value).endswith("expected %d floats" % N)


@pytest.mark.parametrize("kind", ("conv", "flat"))
def test_training_entry_points_need_their_predecessor(kind):
    """apply_grads before any gradient pass, train_rollout / train_rollout_grads before any rollout: fresh nets."""
    from goldsrl import _ffi, _ffi_flat, _ffi_net
    if kind == "conv":
        eng = _ffi.Engine(_ffi.ENV_SWARM, 2, seed=7)
        net = _ffi_net.ConvNet(eng, max_chunk_samples=20)
    else:
        eng = _ffi.Engine(_ffi.ENV_SOLOW, 4, seed=7)
        net = _ffi_flat.FlatNet(eng, max_samples=64)
    eng.reset()
    stats = np.zeros(4, np.float32)
    assert _call(net, kind, "apply_grads", 1e-3, 1.0, _ffi._ptr(stats)) == (_ffi.E_STATE, NO_GRADS[kind])
    assert _call(net, kind, "train_rollout", 1e-3, _ffi._ptr(stats)) == (_ffi.E_STATE, PREFIX[kind] + "train_rollout: no rollout to train on")
    # the conv net's two entry points share one message; the flat net's carry their own names
    name = "train_rollout" if kind == "conv" else "train_rollout_grads"
    assert _call(net, kind, "train_rollout_grads", _ffi._ptr(stats)) == (_ffi.E_STATE, PREFIX[kind] + name + ": no rollout to train on")
    with pytest.raises(_ffi.GrlError) as ei:
        net.train_rollout(1e-3)
    assert ei.value.code == _ffi.E_STATE
    assert not stats.any()
    net.close(); eng.close()


@pytest.mark.parametrize("kind", ("conv", "flat"))
def test_action_counter_round_trip(nets, kind):
    net = nets[kind][1]
    for v in (0, 12345, 2 ** 40 + 3):
        net.set_action_counter(v)
        assert net.get_action_counter() == v
    net.set_action_counter(0)


@pytest.mark.parametrize("kind", ("conv", "flat"))
def test_communicator_refusals_and_state(nets, kind):
    from goldsrl import _ffi
    net = nets[kind][1]
    p = PREFIX[kind]
    def ranks():
        info = net.comm_info()
        return info["rccl_ranks"], info["rccl_user_rank"]
    calls = net.comm_info()["allreduce_calls"]
    assert ranks() == (0, -1)
    assert _call(net, kind, "comm_broadcast_params", 0) == (_ffi.E_STATE, p + "comm_broadcast_params: no communicator")
    assert _call(net, kind, "comm_destroy")[0] == _ffi.OK      # nothing attached: nothing to do
    uid = net.comm_unique_id()
    bad = (_ffi.E_INVALID, p + "comm_init: bad argument")
    assert _call(net, kind, "comm_init", _ffi._ptr(uid), uid.size, 1, 1) == bad          # rank >= world_size
    assert _call(net, kind, "comm_init", _ffi._ptr(uid), uid.size, 2, 2) == bad
    assert _call(net, kind, "comm_init", _ffi._ptr(uid), uid.size, -1, 1) == bad
    assert _call(net, kind, "comm_init", _ffi._ptr(uid), uid.size, 0, 0) == bad
    assert _call(net, kind, "comm_init", _ffi._ptr(uid), uid.size - 1, 0, 1) == bad      # a short id
    assert _call(net, kind, "comm_init", None, uid.size, 0, 1) == bad
    assert ranks() == (0, -1)
    net.comm_init(uid, 0, 1)
    assert _call(net, kind, "comm_init", _ffi._ptr(uid), uid.size, 0, 1) == (_ffi.E_STATE, p + "comm_init: communicator already attached")
    assert ranks() == (1, 0)
    before = net.get_params()
    net.comm_broadcast_params(0)
    assert np.array_equal(net.get_params(), before)
    assert _call(net, kind, "comm_destroy")[0] == _ffi.OK
    assert _call(net, kind, "comm_destroy")[0] == _ffi.OK      # twice
    assert ranks() == (0, -1) and net.comm_info()["allreduce_calls"] == calls      # no update ran: nothing was reduced
    assert _call(net, kind, "comm_broadcast_params", 0) == (_ffi.E_STATE, p + "comm_broadcast_params: no communicator")


def test_conv_net_rccl_communicator_world_size_1_rollout(nets):
    """init, broadcast, the all-reduce inside train_rollout and its accounting with the one rank a one-GPU box allows."""
    eng, net = nets["conv"]
    calls = net.comm_info()["allreduce_calls"]
    assert calls == 0      # no other test of this module trains with a communicator attached
    net.comm_init(net.comm_unique_id(), 0, 1)
    net.comm_broadcast_params(0)
    p0 = net.get_params()
    net.rollout(1, 0)
    eng.wait()
    st = net.train_rollout(1e-3)
    assert np.isfinite(list(st.values())).all() and st["global_norm"] > 0
    assert not np.array_equal(p0, net.get_params())
    info = net.comm_info()
    assert info["allreduce_calls"] == calls + 1 and info["rccl_ranks"] == 1 and info["rccl_user_rank"] == 0
    assert info["allreduce_ms_last"] >= 0 and info["allreduce_ms_total"] >= info["allreduce_ms_last"]
    net.comm_destroy()
    net.comm_destroy()
    assert net.comm_info()["rccl_ranks"] == 0 and net.comm_info()["allreduce_calls"] == calls + 1      # the timing outlives the communicator
    # without the communicator the next update runs alone
    net.rollout(1, 0)
    eng.wait()
    assert np.isfinite(list(net.train_rollout(1e-3).values())).all()
    assert net.comm_info()["allreduce_calls"] == calls + 1
