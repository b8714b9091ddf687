"""GPU: the attainable optimum of the TradeAR1 env (grl_trade_dp_* of include/goldsrl_tradedp.h; csrc/trade_dp.hip).

The solve is held to the float64 numpy restatement of the recurrence (tests/_trade_dp_oracle.py): the top stage's value within
horizon * 64 * 2^-52 * max(1, max|V|) -- a stage adds a few dozen roundings at the magnitude of V plus an ulp or two of exp / log
at g near 1, and max and a convex combination do not amplify what came before -- and the policy by value, because the model has
exact ties (selling from an empty holding, buying with no cash).  The play is held to the per-step path, as the sweep is
(tests/test_gpu_trade_sweep.py)."""
import ctypes as C

import numpy as np
import pytest

import _trade_dp_oracle as TO

pytestmark = pytest.mark.gpu

X_MAX = 0.1     # std_e is 0.0218: 0.9 * x_max plus the upper node is past x_max, so the edge nodes' moves are clamped


def _engine(E, n, cap=0, inject=False, seed=0):
    from goldsrl import _ffi
    eng = _ffi.Engine(_ffi.ENV_TRADE, E, seed=seed, n_assets=n, max_episode_steps=cap, flags=_ffi.F_INJECT_NOISE if inject else 0)
    eng.reset()
    return eng


def _grid(eng, nu=5, nx=4, na=5, nq=3):
    from goldsrl._ffi_tradedp import trade_dp_grid
    return trade_dp_grid(nu=nu, nx=nx, na=na, nq=nq, x_max=X_MAX, std_p=eng.cfg.trade_std_p)


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("nu,nx,na,nq,horizon", [(3, 3, 3, 2, 3), (5, 4, 5, 3, 4), (4, 3, 9, 2, 2)])
def test_solve_against_the_oracle(nu, nx, na, nq, horizon, n):
    from goldsrl._ffi_tradedp import trade_dp_solve
    eng = _engine(2, n)
    grid = _grid(eng, nu, nx, na, nq)
    assert 0.9 * X_MAX + grid["e_nodes"][-1] > X_MAX
    NU, NX = nu ** n, nx ** n
    got = trade_dp_solve(eng, grid, horizon)
    assert got["policy"].shape == (horizon,) + (nu,) * n + (nx,) * n + (n,) and got["value"].shape == (nu,) * n + (nx,) * n
    _, value = TO.solve(grid, n, horizon)
    tol = horizon * 64 * 2.0 ** -52 * max(1.0, np.abs(value).max())
    dev = np.abs(got["value"].reshape(NU, NX) - value).max()
    print("trade_dp n=%d grid %s: |value - oracle| %.3e (tolerance %.3e), max |V| %.3e" % (n, (nu, nx, na, nq, horizon), dev, tol, np.abs(value).max()))
    assert dev <= tol
    # every stage's decisions by value, on the device's own value of the stage below
    below = np.zeros((NU, NX))
    for s in range(horizon):
        Q = TO.q_values(grid, n, below, TO.actions(grid, n)[None, None])
        chosen = TO.q_values(grid, n, below, got["policy"][s].reshape(NU, NX, 1, n).astype(np.float64))[..., 0]
        assert (chosen >= Q.max(axis=2) - 2 * tol).all(), s
        below = got["value"].reshape(NU, NX) if s + 1 == horizon else trade_dp_solve(eng, grid, s + 1)["value"].reshape(NU, NX)
        assert np.abs(below - Q.max(axis=2)).max() <= tol, s
    assert np.abs(got["policy"]).max() == 1.0 and (got["value"] >= 0).all() and got["value"].max() > 0
    eng.close()


def _everything(eng):
    fields = ("TRADE_CASH", "TRADE_ASSETS", "TRADE_QUANTITY", "TRADE_PRICES", "ELAPSED", "EPISODE", "NHIST")
    d = {f: eng.get_state(f) for f in fields}
    d.update({o: eng.read(o) for o in ("reward", "done", "elapsed", "obs", "obs_raw", "done_count")})
    return d


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("E", [1, 5, 130])
def test_play_is_the_per_step_path(E, n):
    """A 35-step TimeLimit, a start 4 steps into the episode, a table of 6 stages (shorter than the 31 steps left) and a tape."""
    from goldsrl._ffi_tradedp import trade_dp_actions, trade_dp_play, trade_dp_solve
    cap, pre, H, T = 35, 4, 6, 40
    rng = np.random.RandomState(E + n)
    tape = rng.normal(size=(pre + T, E, n)).astype(np.float32)
    first = rng.uniform(-0.5, 0.5, size=(pre, E, n)).astype(np.float32)

    def make():
        eng = _engine(E, n, cap, inject=True, seed=E)
        for t in range(pre):
            eng.set_state("TRADE_NORMALS", tape[t])
            eng.step(first[t])
        return eng

    eng, twin = make(), make()
    grid = _grid(eng)
    policy = trade_dp_solve(eng, grid, H)["policy"]
    before = _everything(eng)
    got = trade_dp_play(eng, T, trace_steps=T, normals=tape[pre:])
    after = _everything(eng)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    left = cap - pre
    assert (got["length"] == left).all() and (got["finished"] == 1).all() and not got["depleted"].any()
    rewards = np.zeros((left, E), np.float32)
    for t in range(left):
        cash, q, p = twin.get_state("TRADE_CASH"), twin.get_state("TRADE_QUANTITY"), twin.get_state("TRADE_PRICES")
        want = trade_dp_actions(policy, grid, H, cash, q.reshape(E, n), p.reshape(E, n), cap - twin.get_state("ELAPSED"))
        assert np.abs(got["actions"][t] - want).max() <= 2.0 ** -23, t
        twin.set_state("TRADE_NORMALS", tape[pre + t])
        twin.step(got["actions"][t])
        rewards[t] = twin.read("reward")
        if t + 1 < left:                                                 # the last step resets the twin
            assert got["assets"][t].tobytes() == twin.get_state("TRADE_ASSETS").tobytes(), t
    assert got["rewards"][:left].tobytes() == rewards.tobytes() and (twin.read("done") > 0).all()
    assert (got["rewards"][left:] == 0).all() and (got["actions"][left - 1] == 0).all() and np.abs(got["actions"][0]).max() > 0
    assert got["total"].tobytes() == np.cumsum(rewards.astype(np.float64), axis=0)[-1].tobytes()
    eng.close(); twin.close()


@pytest.mark.parametrize("n", [1, 2])
def test_cash_totals_zero_and_the_foresight_bound_stands_above(n):
    from goldsrl._ffi_tradedp import table_shape, trade_dp_play, trade_dp_set_policy, trade_dp_solve
    from goldsrl._ffi_tradeforesight import trade_foresight
    E, cap = 70, 35
    eng, twin = _engine(E, n, cap, seed=3), _engine(E, n, cap, seed=3)
    tape = np.random.RandomState(n).normal(size=(cap, E, n)).astype(np.float32)
    grid = _grid(eng)
    trade_dp_set_policy(eng, grid, np.zeros(table_shape(n, grid, 2), np.float32))
    held = trade_dp_play(eng, cap, normals=tape)
    assert (held["total"] == 0).all() and (held["length"] == cap).all() and (held["final_assets"] == eng.get_state("TRADE_ASSETS")).all()
    trade_dp_solve(eng, grid, 8, read=False)
    got = trade_dp_play(eng, cap, normals=tape)
    bound = trade_foresight(eng, [0], cap, normals=tape)["bound"][0]
    allow = got["length"] * 2.0 ** -24 * np.maximum(np.abs(got["min"]), np.abs(got["max"])).astype(np.float64) + 1e-10
    print("trade_dp n=%d: played mean %.6f, foresight bound mean %.6f" % (n, got["total"].mean(), bound.mean()))
    assert (got["total"] <= bound + allow).all() and got["total"].mean() > 0
    own = trade_dp_play(eng, cap)                                        # the handle's generator; its counters stay where they were
    assert own["total"].tobytes() != got["total"].tobytes()
    act = np.full((E, n), 0.25, np.float32)
    for _ in range(2):
        eng.step(act); twin.step(act)
    a, b = _everything(eng), _everything(twin)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    eng.close(); twin.close()


@pytest.mark.parametrize("case,code,word", [("n_assets", "E_INVALID", b"n_assets"), ("na", "E_INVALID", b"na must be odd"),
                                            ("slab", "E_SIZE", b"nu = 4096"), ("table", "E_SIZE", b"horizon * nu^n"),
                                            ("play", "E_STATE", b"grl_trade_dp_solve"), ("tape", "E_INVALID", b"pass a tape")])
def test_refusals(case, code, word):
    from goldsrl import _ffi, _ffi_tradedp
    lib = _ffi.load_library(extra_signatures=_ffi_tradedp.TRADE_DP_SIGNATURES)
    eng = _engine(4, 3 if case == "n_assets" else 2, 8, inject=case == "tape")
    sizes = {"na": dict(na=4), "slab": dict(nu=4096, nx=2, nq=3), "table": dict(nu=9, nx=64)}.get(case, {})
    g = _ffi_tradedp._grid_struct(_grid(eng, **sizes))
    if case == "play":
        rc = lib.grl_trade_dp_play(eng.h, None, 4, 0)
    elif case == "tape":
        _ffi_tradedp.trade_dp_solve(eng, _grid(eng), 2, read=False)
        rc = lib.grl_trade_dp_play(eng.h, None, 4, 0)
    else:
        rc = lib.grl_trade_dp_solve(eng.h, C.byref(g), 512 if case == "table" else 2)
    assert rc == getattr(_ffi, code) and word in lib.grl_last_error(eng.h), lib.grl_last_error(eng.h)
    eng.close()


def test_baseline_monitor_and_script(capsys):
    from goldsrl.agents.a3c.policy_monitor import PolicyMonitor
    from goldsrl.baselines import TradeOptimalBaseline
    from goldsrl.scripts import optimal_trade
    mon = PolicyMonitor("TradeAR1-v0", n_envs=3, max_episode_steps=16)
    grid = _grid(mon.net.eng)
    total = mon.trade_optimal(grid=grid, horizon=4)
    assert total == mon.attainable_total_reward == mon.attainable_stats["total"].mean() and total > 0
    assert (mon.net.eng.get_state("ELAPSED") == 0).all() and (mon.net.eng.get_state("TRADE_PRICES") == 1).all()
    mon.net.eng.reset()
    b = TradeOptimalBaseline(mon.net.eng, grid=grid, horizon=4)
    assert b.run()["total"].tobytes() == mon.attainable_stats["total"].tobytes() and b.total() == total
    mon.close()
    rec = optimal_trade.main(["--envs", "4", "--steps", "16", "--grid", "5", "4", "5", "3", "--horizon", "4", "--assets", "1"])
    assert rec["rule"] <= rec["foresight"] and rec["optimal"] <= rec["foresight"] and "attainable" in capsys.readouterr().out
