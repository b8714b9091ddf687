"""GPU: the Swarm step's exact path with one shared reciprocal per pair (the default) against the same path with the compiler's three
IEEE divisions (GRL_SWARM_DIV=ref, read at grl_create).  The two are the same correctly rounded quotients, so every state and
every output of a long run is equal bit for bit; tests/test_swarm_div_exact.py holds the arithmetic itself on the CPU."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E, STEPS, LIMIT = 2048, 200, 64
STATES = ("SWARM_X", "SWARM_XA")
OUTPUTS = ("reward_f64", "reward", "done", "elapsed", "locust_bins", "agent_bins", "positions")


def _run(monkeypatch, div):
    from goldsrl import _ffi
    if div is None:
        monkeypatch.delenv("GRL_SWARM_DIV", raising=False)
    else:
        monkeypatch.setenv("GRL_SWARM_DIV", div)
    # TimeLimit at 64 steps: three boundaries inside the run, where every env resets (burn-in steps included) in one launch;
    # an env whose reward reaches 0 resets on its own in between
    eng = _ffi.Engine(_ffi.ENV_SWARM, E, device_id=0, seed=20260, max_episode_steps=LIMIT)
    eng.reset()
    rng = np.random.RandomState(11)
    trace = [[eng.get_state(s) for s in STATES] + [eng.read(o) for o in OUTPUTS]]
    for t in range(STEPS):
        act = rng.normal(scale=1.0 + (t % 7), size=(E, 10, 2)).astype(np.float32)
        eng.step(act)
        trace.append([eng.get_state(s) for s in STATES] + [eng.read(o) for o in OUTPUTS])
    eng.close()
    return trace


def test_one_reciprocal_per_pair_steps_exactly_as_three_divisions(monkeypatch):
    ref = _run(monkeypatch, "ref")
    new = _run(monkeypatch, None)
    assert len(ref) == len(new) == STEPS + 1
    done_steps = 0
    for t, (a, b) in enumerate(zip(ref, new)):
        for name, u, v in zip(STATES + OUTPUTS, a, b):
            assert u.dtype == v.dtype and u.shape == v.shape
            # bytes, not values: -0.0 and NaN payloads count
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), "%s differs at step %d" % (name, t)
        done_steps += int(a[len(STATES) + OUTPUTS.index("done")].any())
    # the run did cross TimeLimit boundaries (all envs done at once) -- the reset kernel's burn-in steps were compared too
    assert done_steps >= STEPS // LIMIT
    assert all(r[len(STATES) + OUTPUTS.index("done")].all() for r in (ref[LIMIT], ref[2 * LIMIT], ref[3 * LIMIT]))
