"""The host surface the three A3C nets share behind their prefixes (grl_gnet_ gated Ticker trader, grl_anet_ Gaussian agent on Solow and
TradeAR1, grl_dnet_ savings-grid agent): what each refuses, with which code and which message, the small state it keeps (action
counter, optimizer state), and that every named read-back has its documented shape.  Every refusal is argument or state validation
on the host, before any launch; the expected strings are the C sources'."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ("gated", "solow", "trade", "grid")
PREFIX = {"gated": "grl_gnet_", "solow": "grl_anet_", "trade": "grl_anet_", "grid": "grl_dnet_"}
E, MS, T, R, K, CAP = 2, 4, 2, 5, 51, 5
# (S0, D): observation width, temporal row width
WIDTHS = {"gated": (7, 4), "solow": (2, 2), "trade": (5, 5), "grid": (2, 2)}
ROLLOUT = {
    "gated": {"states": (T, E, 7), "windows": (T, E, R, 4), "choices": (T, E, 2), "raw": (T, E, 2), "probs": (T, E, 2, 3), "mu": (T, E, 2, 3),
              "sigma": (T, E, 2, 3), "values": (T, E), "rewards": (T, E), "dones": (T, E), "weights": (T, E), "adv": (T, E),
              "targets": (T, E), "actions": (T, E, 4), "boot": (E,)},
    "solow": {"states": (T, E, 2), "windows": (T, E, R, 2), "raw": (T, E, 1), "mu": (T, E, 1), "sigma": (T, E, 1), "actions": (T, E, 1),
              "values": (T, E), "rewards": (T, E), "dones": (T, E), "weights": (T, E), "adv": (T, E), "targets": (T, E),
              "term_values": (T, E), "term_states": (T, E, 2), "term_windows": (T, E, R, 2), "boot": (E,)},
    "trade": {"states": (T, E, 5), "windows": (T, E, R, 5), "raw": (T, E, 2), "mu": (T, E, 2), "sigma": (T, E, 2), "actions": (T, E, 2),
              "values": (T, E), "rewards": (T, E), "dones": (T, E), "weights": (T, E), "adv": (T, E), "targets": (T, E),
              "term_values": (T, E), "boot": (E,)},
    "grid": {"states": (T, E, 2), "windows": (T, E, R, 2), "probs": (T, E, K), "choices": (T, E), "actions": (T, E), "values": (T, E),
             "rewards": (T, E), "dones": (T, E), "weights": (T, E), "adv": (T, E), "targets": (T, E), "term_values": (T, E),
             "term_states": (T, E, 2), "term_windows": (T, E, R, 2), "boot": (E,)},
}
# the trace of eval(3, trace_steps=3): (S, E) + tail
TRACE = {
    "gated": {"states": (7,), "probs": (2, 3), "mu": (2, 3), "choices": (2,), "actions": (4,), "rewards": (), "dones": ()},
    "solow": {"states": (2,), "mu": (1,), "actions": (1,), "rewards": (), "dones": ()},
    "trade": {"states": (5,), "mu": (2,), "actions": (2,), "rewards": (), "dones": ()},
    "grid": {"states": (2,), "choices": (), "actions": (), "rewards": (), "dones": ()},
}
RESULTS = {"total_reward": np.float64, "length": np.int32, "finished": np.uint8}


def _engine(kind):
    from goldsrl import _ffi
    if kind == "gated":
        eng = _ffi.Engine(_ffi.ENV_TICKER, E, seed=7, max_episode_steps=CAP)
        eng.ticker_set_table(np.load(os.path.join(HERE, "golden", "ticker.npz"))["matrix"])
    elif kind == "trade":
        eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=7, n_assets=2, max_episode_steps=CAP)
    else:
        eng = _ffi.Engine(_ffi.ENV_SOLOW, E, seed=7, max_episode_steps=CAP)
    eng.reset()
    return eng


def _net(kind, eng, **kw):
    from goldsrl import _ffi_discrete, _ffi_gated, _ffi_gauss
    kw = dict(dict(rnn_length=R, max_samples=MS), **kw)
    if kind == "gated":
        return _ffi_gated.GatedNet(eng, **kw)
    if kind == "grid":
        return _ffi_discrete.DiscreteNet(eng, **dict(dict(num_choices=K), **kw))
    return _ffi_gauss.GaussNet(eng, **kw)


def _init(kind):
    from goldsrl import _ffi_discrete, _ffi_gated, _ffi_gauss
    if kind == "gated":
        return _ffi_gated.default_init_gated(3)
    if kind == "grid":
        return _ffi_discrete.default_init_discrete(3, K)
    return _ffi_gauss.default_init_gauss(3, **(_ffi_gauss.SOLOW_SIZES if kind == "solow" else _ffi_gauss.TRADE_SIZES))


@pytest.fixture(scope="module")
def nets():
    out = {}
    for kind in KINDS:
        eng = _engine(kind)
        net = _net(kind, eng)
        net.set_params(_init(kind))
        out[kind] = (eng, net)
    yield out
    for eng, net in out.values():
        net.close(); eng.close()


def _call(net, kind, name, *args):
    """(return code, last error) of one C call"""
    rc = getattr(net.lib, PREFIX[kind] + name)(net.n, *args)
    return rc, getattr(net.lib, PREFIX[kind] + "last_error")(net.n).decode()


def _refused(code, msg, fn, *args, **kw):
    """the Python method raises the C call's code and message"""
    from goldsrl import _ffi
    with pytest.raises(_ffi.GrlError) as ei:
        fn(*args, **kw)
    assert (ei.value.code, str(ei.value)) == (code, "libgoldsrl error %d: %s" % (code, msg))


def _samples(kind, n, choice=0):
    """the positional arguments of predict (the first two) and train for n zero samples"""
    s0, d = WIDTHS[kind]
    head = (np.zeros((n, s0), np.float32), np.zeros((n, R, d), np.float32))
    one = np.zeros(n, np.float32)
    if kind == "gated":
        return head + (np.full((n, 2), choice, np.int32), np.zeros((n, 2), np.float32), one, one)
    if kind == "grid":
        return head + (np.full(n, choice, np.int32), one, one)
    return head + (np.zeros((n, 1 if kind == "solow" else 2), np.float32), one, one)


@pytest.mark.parametrize("kind", KINDS)
def test_wrong_lengths_which_and_step_are_refused(nets, kind):
    from goldsrl import _ffi
    net = nets[kind][1]
    N = net.num_params
    before, opt = net.get_params(), net.get_optimizer_state()
    size = (_ffi.E_SIZE, "length must be num_params")
    for short in (N - 1, N + 1, 0):
        a, b = np.zeros(N + 1, np.float32), np.zeros(N + 1, np.float32)
        step = C.c_int64(-5)
        assert _call(net, kind, "set_params", _ffi._ptr(a), short) == size, short
        assert _call(net, kind, "get_params", _ffi._ptr(a), short) == size, short
        assert _call(net, kind, "get_grads", 0, _ffi._ptr(a), short) == size, short
        assert _call(net, kind, "set_optimizer_state", _ffi._ptr(a), _ffi._ptr(b), short, 3) == size, short
        assert _call(net, kind, "get_optimizer_state", _ffi._ptr(a), _ffi._ptr(b), short, C.byref(step)) == size, short
        assert step.value == -5
    a = np.zeros(N, np.float32)
    assert _call(net, kind, "get_grads", 2, _ffi._ptr(a), N) == (_ffi.E_INVALID, PREFIX[kind] + "get_grads: which is 0 or 1")
    assert _call(net, kind, "get_grads", -1, _ffi._ptr(a), N) == (_ffi.E_INVALID, PREFIX[kind] + "get_grads: which is 0 or 1")
    assert _call(net, kind, "set_optimizer_state", _ffi._ptr(a), _ffi._ptr(a), N, -1) == (_ffi.E_INVALID, "global step must be >= 0")
    # nothing was written
    assert np.array_equal(net.get_params(), before)
    now = net.get_optimizer_state()
    assert now["global_step"] == opt["global_step"] and np.array_equal(now["ms_policy"], opt["ms_policy"])
    # the Python methods raise the same
    _refused(_ffi.E_SIZE, "length must be num_params", net.set_params, np.zeros(N - 1, np.float32))
    _refused(_ffi.E_INVALID, "global step must be >= 0", net.set_optimizer_state, opt["ms_policy"], opt["ms_value"], -3)


@pytest.mark.parametrize("kind", KINDS)
def test_sample_calls_are_refused_past_max_samples_and_out_of_range(nets, kind):
    from goldsrl import _ffi
    net = nets[kind][1]
    p = PREFIX[kind]
    big = _samples(kind, MS + 1)
    _refused(_ffi.E_SIZE, p + "predict: n exceeds max_samples", net.predict, *big[:2])
    _refused(_ffi.E_SIZE, p + "train: n exceeds max_samples", net.train, *big, apply_update=False)
    if kind == "gated":
        for bad in (3, -1):
            _refused(_ffi.E_INVALID, "grl_gnet_train: choices must be 0, 1 or 2", net.train, *_samples(kind, 2, bad), apply_update=False)
    if kind == "grid":
        for bad in (K, -1):
            _refused(_ffi.E_INVALID, "grl_dnet_train: a choice outside [0, num_choices)", net.train, *_samples(kind, 2, bad),
                     apply_update=False)
    _refused(_ffi.E_INVALID, p + "rollout: T >= 1", net.rollout, 0)
    _refused(_ffi.E_INVALID, p + "rollout: T >= 1", net.rollout, -2)
    _refused(_ffi.E_INVALID, p + "eval: max_steps >= 1, trace_steps >= 0", net.eval, 0, 0)
    _refused(_ffi.E_INVALID, p + "eval: max_steps >= 1, trace_steps >= 0", net.eval, 1, -1)


@pytest.mark.parametrize("kind", KINDS)
def test_reads_and_the_update_need_their_predecessor(kind):
    """train_rollout / read_rollout before any rollout, read_eval before any evaluation: a fresh net."""
    from goldsrl import _ffi
    eng = _engine(kind)
    net = _net(kind, eng)
    p = PREFIX[kind]
    stats = np.zeros(6, np.float32)
    buf = np.zeros(T * E * 7, np.float32)
    assert _call(net, kind, "train_rollout", 1e-3, _ffi._ptr(stats)) == (_ffi.E_STATE, p + "train_rollout: no rollout yet")
    assert not stats.any()
    for name in ("states", "nope"):      # the state comes before the name
        assert _call(net, kind, "read_rollout", name.encode(), _ffi._ptr(buf), buf.nbytes) == (_ffi.E_STATE, p + "read_rollout: no rollout yet")
    for name in ("total_reward", "states", "nope"):
        assert _call(net, kind, "read_eval", name.encode(), _ffi._ptr(buf), 16) == (_ffi.E_STATE, p + "read_eval: no evaluation yet")
    _refused(_ffi.E_STATE, p + "train_rollout: no rollout yet", net.train_rollout, 1e-3)
    net.close(); eng.close()


@pytest.mark.parametrize("kind", KINDS)
def test_every_named_buffer_reads_back_and_the_others_are_refused(nets, kind):
    from goldsrl import _ffi
    eng, net = nets[kind]
    p = PREFIX[kind]
    drawn = net.get_action_counter()
    net.rollout(T)
    for name, shape in ROLLOUT[kind].items():
        a = net.read_rollout(name)
        assert a.shape == shape and a.dtype == (np.int32 if name == "choices" else np.float32), name
        assert np.isfinite(a).all(), name
    assert net.get_action_counter() == drawn + T
    buf = np.zeros(T * E * R * 7 + 1, np.float32)
    assert _call(net, kind, "read_rollout", b"nope", _ffi._ptr(buf), 16) == (_ffi.E_INVALID, p + "read_rollout: unknown buffer nope")
    for name, shape in ROLLOUT[kind].items():
        nbytes = int(np.prod(shape)) * 4
        for wrong in (nbytes - 4, nbytes + 4, 0):
            assert _call(net, kind, "read_rollout", name.encode(), _ffi._ptr(buf), wrong) == (_ffi.E_SIZE, p + "read_rollout: wrong size for " + name)
    if kind == "trade":      # kept with always_bootstrap only: absent comes before the size
        for name, nbytes in (("term_states", T * E * 5 * 4), ("term_windows", T * E * R * 5 * 4), ("term_states", 0)):
            assert _call(net, kind, "read_rollout", name.encode(), _ffi._ptr(buf), nbytes) == \
                (_ffi.E_STATE, "grl_anet_read_rollout: %s exists with always_bootstrap = 1 only" % name)
    # the evaluation: 3 steps, all of them traced (no episode ends before the cap of 5)
    eng.reset()
    ev = net.eval(3, trace_steps=3)
    assert set(ev) == set(RESULTS) | set(TRACE[kind])
    for name, dt in RESULTS.items():
        assert ev[name].shape == (E,) and ev[name].dtype == dt, name
    assert (ev["length"] == 3).all() and not ev["finished"].any()
    for name, tail in TRACE[kind].items():
        assert ev[name].shape == (3, E) + tail and ev[name].dtype == (np.int32 if name == "choices" else np.float32), name
        assert np.isfinite(ev[name]).all(), name
    assert _call(net, kind, "read_eval", b"nope", _ffi._ptr(buf), 16) == (_ffi.E_INVALID, p + "read_eval: unknown buffer nope")
    sizes = {"total_reward": E * 8, "length": E * 4, "finished": E}
    sizes.update({name: 3 * E * int(np.prod(tail, dtype=np.int64)) * 4 for name, tail in TRACE[kind].items()})
    for name, nbytes in sizes.items():
        for wrong in (nbytes - 1, nbytes + 4, 0):
            assert _call(net, kind, "read_eval", name.encode(), _ffi._ptr(buf), wrong) == (_ffi.E_SIZE, p + "read_eval: wrong size for " + name)
    # a trace longer than the evaluation is cut to it
    eng.reset()
    assert net.eval(2, trace_steps=9)["rewards"].shape == (2, E)
    eng.reset()


@pytest.mark.parametrize("kind", KINDS)
def test_action_counter_and_optimizer_state_round_trip(nets, kind):
    net = nets[kind][1]
    N = net.num_params
    keep_counter, keep = net.get_action_counter(), net.get_optimizer_state()
    for v in (0, 12345, 2 ** 40 + 3):
        net.set_action_counter(v)
        assert net.get_action_counter() == v
    rng = np.random.RandomState(5)
    msp, msv = rng.rand(N).astype(np.float32), rng.rand(N).astype(np.float32)
    net.set_optimizer_state(msp, msv, 2 ** 33 + 4)
    got = net.get_optimizer_state()
    assert np.array_equal(got["ms_policy"], msp) and np.array_equal(got["ms_value"], msv) and got["global_step"] == 2 ** 33 + 4
    net.set_optimizer_state(keep["ms_policy"], keep["ms_value"], keep["global_step"])
    net.set_action_counter(keep_counter)


def test_a_fresh_net_has_ms_at_one_and_counters_at_zero():
    eng = _engine("solow")
    net = _net("solow", eng)
    st = net.get_optimizer_state()
    assert (st["ms_policy"] == 1).all() and (st["ms_value"] == 1).all() and st["global_step"] == 0 and net.get_action_counter() == 0
    assert not net.get_params().any()
    net.close(); eng.close()


def test_create_refusals(nets):
    """On the engine's handle: no net exists to carry the message."""
    from goldsrl import _ffi
    inv = _ffi.E_INVALID
    eng = {k: nets[k][0] for k in KINDS}
    # wrong env kind
    for other in ("solow", "trade"):
        _refused(inv, "grl_gnet_create: the gated trader needs a Ticker handle", _net, "gated", eng[other])
    _refused(inv, "grl_anet_create: the Gaussian agent needs a Solow handle or a TradeAR1 handle with 2 assets", _net, "solow", eng["gated"])
    three = _ffi.Engine(_ffi.ENV_TRADE, E, seed=7, n_assets=3)
    _refused(inv, "grl_anet_create: the Gaussian agent needs a Solow handle or a TradeAR1 handle with 2 assets", _net, "trade", three)
    three.close()
    for other in ("gated", "trade"):
        _refused(inv, "grl_dnet_create: the savings-grid agent needs a Solow handle", _net, "grid", eng[other])
    for kind in KINDS:
        p = PREFIX[kind] + "create: "
        # the env kind comes before the range check, the range check before the net's own bounds
        for bad in (dict(rnn_length=21), dict(rnn_length=0), dict(max_samples=0), dict(lr_decay_steps=0), dict(scale=0.0),
                    dict(gae_lambda=0.0), dict(gae_lambda=1.5)):
            _refused(inv, p + "config out of range (rnn_length 1..20)", _net, kind, eng[kind], **bad)
        _refused(inv, p + "config size mismatch", _net, kind, eng[kind], struct_size=4)
    _refused(inv, "grl_gnet_create: config size mismatch", _net, "gated", eng["solow"], struct_size=4)      # the size comes first
    # always_bootstrap against the env
    _refused(inv, "grl_anet_create: a Solow handle needs always_bootstrap = 1", _net, "solow", eng["solow"], always_bootstrap=0)
    _refused(inv, "grl_anet_create: a TradeAR1 handle needs always_bootstrap = 0", _net, "trade", eng["trade"], always_bootstrap=1)
    _refused(inv, "grl_dnet_create: a Solow handle needs always_bootstrap = 1", _net, "grid", eng["solow"], always_bootstrap=0)
    _refused(inv, "grl_anet_create: config out of range (rnn_length 1..20)", _net, "solow", eng["solow"], always_bootstrap=0, rnn_length=21)
    # the grid
    grid = "grl_dnet_create: num_choices 2..64, grid_lb < grid_ub"
    for bad in (dict(num_choices=1), dict(num_choices=65), dict(grid_lb=0.5, grid_ub=0.5), dict(grid_lb=0.6, grid_ub=0.5)):
        _refused(inv, grid, _net, "grid", eng["solow"], **bad)
    _refused(inv, grid, _net, "grid", eng["solow"], num_choices=1, always_bootstrap=0)      # the grid comes before always_bootstrap
    _refused(inv, "grl_dnet_create: config out of range (rnn_length 1..20)", _net, "grid", eng["solow"], num_choices=1, rnn_length=21)
    # the handles still make nets
    for kind in KINDS:
        _net(kind, eng[kind]).close()
