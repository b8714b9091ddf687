"""CPU: goldsrl/_ffi_episode.py, what the bindings of the seven whole-episode launches share, on a stub engine and a stub read
function -- no library is loaded."""
import ctypes as C

import numpy as np
import pytest


class _Cfg(object):
    def __init__(self, cap):
        self.max_episode_steps = cap


class _Engine(object):
    def __init__(self, E=3, cap=24):
        self.E, self.h, self.cfg, self.checked = E, object(), _Cfg(cap), []

    def _check(self, rc):
        self.checked.append(rc)


def test_read_outputs_asks_for_each_name_once_with_its_dtype_shape_and_bytes():
    from goldsrl._ffi_episode import read_outputs
    eng, calls = _Engine(), []

    def read(h, name, ptr, nbytes):
        assert h is eng.h
        calls.append((name, nbytes))
        C.memset(ptr, len(calls), nbytes)            # call i fills its buffer with the byte i
        return 100 + len(calls)

    specs = (("total", np.float64, ()), ("length", np.int32, ()), ("finished", np.uint8, ()), ("trace_actions", np.float32, (4,)),
             ("trace_x", np.float64, (80, 2)))
    out = read_outputs(eng, read, specs, (5, 3))
    assert list(out) == [s[0] for s in specs]
    assert calls == [(b"total", 120), (b"length", 60), (b"finished", 15), (b"trace_actions", 240), (b"trace_x", 5 * 3 * 160 * 8)]
    assert eng.checked == [101, 102, 103, 104, 105]                      # every return code went through the engine's check
    for i, (name, dt, inner) in enumerate(specs):
        a = out[name]
        assert a.dtype == dt and a.shape == (5, 3) + inner and a.flags["C_CONTIGUOUS"]
        assert (a.view(np.uint8) == i + 1).all()                         # the buffer the read function was handed is the one returned
    one = read_outputs(eng, read, (("policy", np.float32, (4, 7, 5, 3)),), ())
    assert one["policy"].shape == (4, 7, 5, 3) and calls[-1] == (b"policy", 4 * 7 * 5 * 3 * 4)


def test_steps_and_trace_defaults_and_refusals():
    from goldsrl._ffi_episode import steps_and_trace
    eng = _Engine(cap=24)
    assert steps_and_trace(eng, "solow_sweep", None, None) == (24, -1)
    assert steps_and_trace(eng, "solow_sweep", 7, 2) == (7, 2)
    assert steps_and_trace(eng, "solow_dp_play", np.int64(5)) == (5, -1)
    got = steps_and_trace(eng, "trade_sweep", 3.0, np.int32(0))
    assert got == (3, 0) and all(type(v) is int for v in got)
    names = ("solow_sweep", "trade_sweep", "ticker_sweep", "ticker_foresight", "solow_dp_play", "swarm_rules")
    for name in names:
        for bad in (0, -3):
            with pytest.raises(ValueError) as e:
                steps_and_trace(eng, name, bad, None)
            assert str(e.value) == name + ": max_steps must be at least 1 (an engine without a TimeLimit has no default)"
        with pytest.raises(ValueError) as e:                              # no TimeLimit: the default is 0
            steps_and_trace(_Engine(cap=0), name, None, 1)
        assert str(e.value) == name + ": max_steps must be at least 1 (an engine without a TimeLimit has no default)"


def test_reward_moments_is_importable_from_the_sweep_binding_and_is_the_population_form():
    from goldsrl import _ffi_episode, _ffi_sweep
    assert _ffi_sweep.reward_moments is _ffi_episode.reward_moments
    r = np.array([[0.5, -1.0, 2.0, 0.25], [1.0, 1.0, 1.0, 1.0]])
    mean, std = _ffi_sweep.reward_moments(r.sum(1), (r * r).sum(1), np.array([4, 4], np.int32))
    np.testing.assert_allclose(mean, r.mean(1), rtol=1e-15)
    np.testing.assert_allclose(std, r.std(1), rtol=1e-14, atol=1e-15)
