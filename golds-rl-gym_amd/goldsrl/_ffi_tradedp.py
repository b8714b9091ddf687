"""ctypes binding of the attainable optimum of the TradeAR1 env (C ABI: include/goldsrl_tradedp.h): backward induction over
non-anticipating policies on a (shares, log prices) grid, one kernel launch per stage, and the play of the tabulated policy, every
env a whole episode in one launch.  trade_dp_actions is the host form of the play's look-up, device-free."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_episode import read_outputs, steps_and_trace

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t
MAX_NODES = 15

# include/goldsrl_tradedp.h: a dict of its own, as the header is a file of its own (tests/test_trade_dp_header.py pins both)
TRADE_DP_SIGNATURES = {
    "grl_trade_dp_solve": (C.c_int, [_P, _P, _I]),
    "grl_trade_dp_set_policy": (C.c_int, [_P, _P, _I, _P]),
    "grl_trade_dp_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
    "grl_trade_dp_play": (C.c_int, [_P, _P, _I, _I]),
    "grl_trade_dp_play_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}

# LABNOTES "Attainable optimum of TradeAR1": the refinement sequence these came from
DEFAULT_HORIZON = 64
DEFAULT_SIZES = {"nu": 17, "nx": 17, "na": 17, "nq": 3}
TRADE_STD_P = 0.05          # grl_config's default (fed_env.py:269): of the log price's stationary law; std_e^2 = std_p^2 (1 - 0.81)


class TradeDpGrid(C.Structure):
    """grl_trade_dp_grid"""
    _fields_ = [("x_max", C.c_double), ("e_nodes", C.c_double * MAX_NODES), ("e_weights", C.c_double * MAX_NODES),
                ("nu", _I), ("nx", _I), ("na", _I), ("nq", _I)]


def trade_dp_grid(nu=None, nx=None, na=None, nq=None, x_max=None, std_e=None, std_p=TRADE_STD_P):
    """The grid as a dict: the sizes, x_max (default 4 * std_p) and the Gauss-Hermite rule for eps ~ N(0, std_e^2): e_nodes =
    std_e * x_k (ascending) and e_weights normalised to sum 1, float64 (numpy.polynomial.hermite_e.hermegauss).  std_e defaults to
    the env's sqrt(std_p^2 (1 - 0.81))."""
    nu, nx, na, nq = (int(DEFAULT_SIZES[k] if v is None else v) for k, v in (("nu", nu), ("nx", nx), ("na", na), ("nq", nq)))
    if not 1 <= nq <= MAX_NODES:
        raise ValueError("nq must be in 1..%d" % MAX_NODES)
    if std_e is None:
        std_e = float(np.sqrt((std_p * std_p) * (1 - 0.9 * 0.9)))      # the handle's statement (csrc/flat_envs.hip)
    x, w = np.polynomial.hermite_e.hermegauss(nq)
    return {"nu": nu, "nx": nx, "na": na, "nq": nq, "x_max": float(4.0 * std_p if x_max is None else x_max), "std_e": float(std_e),
            "e_nodes": np.asarray(float(std_e) * x, np.float64), "e_weights": np.asarray(w / w.sum(), np.float64)}


def _grid_struct(grid):
    g = TradeDpGrid()
    for name in ("x_max", "nu", "nx", "na", "nq"):
        setattr(g, name, grid[name])
    for j in range(min(int(grid["nq"]), MAX_NODES)):
        g.e_nodes[j], g.e_weights[j] = float(grid["e_nodes"][j]), float(grid["e_weights"][j])
    return g


def table_shape(n_assets, grid, horizon):
    """(horizon, [nu]^n, [nx]^n, n) of the policy table on `grid`"""
    n = int(n_assets)
    return (int(horizon),) + (grid["nu"],) * n + (grid["nx"],) * n + (n,)


def _trade(engine, who):
    if engine.kind != _ffi.ENV_TRADE:
        raise ValueError("%s: the engine is not a TradeAR1 engine" % who)
    return _ffi.load_library(extra_signatures=TRADE_DP_SIGNATURES)


def trade_dp_solve(engine, grid=None, horizon=DEFAULT_HORIZON, read=True):
    """Backward induction over `horizon` stages on `grid` (default: trade_dp_grid() at the engine's shock) for the engine's model;
    the engine keeps the tables for trade_dp_play.  Returns {"grid", "horizon"} and, with read, "policy" (horizon, [nu]^n, [nx]^n,
    n) float32 -- row s the decisions with s + 1 price moves left -- and "value" ([nu]^n, [nx]^n) float64, the top stage's."""
    lib = _trade(engine, "trade_dp_solve")
    if grid is None:
        grid = trade_dp_grid(std_p=engine.cfg.trade_std_p)
    g = _grid_struct(grid)
    engine._check(lib.grl_trade_dp_solve(engine.h, C.byref(g), int(horizon)))
    out = {"grid": grid, "horizon": int(horizon)}
    if read:
        shape = table_shape(engine.cfg.n_assets, grid, horizon)
        out.update(read_outputs(engine, lib.grl_trade_dp_read, (("policy", np.float32, shape), ("value", np.float64, shape[1:-1])), ()))
    return out


def trade_dp_set_policy(engine, grid, policy):
    """Upload policy (horizon, [nu]^n, [nx]^n, n) in place of a solved table: trade_dp_play then plays it."""
    lib = _trade(engine, "trade_dp_set_policy")
    p = np.ascontiguousarray(policy, np.float32)
    want = table_shape(engine.cfg.n_assets, grid, 1)[1:]
    if p.ndim != len(want) + 1 or p.shape[1:] != want:
        raise ValueError("trade_dp_set_policy: expected (horizon,) + %s, got %s" % (want, p.shape))
    g = _grid_struct(grid)
    engine._check(lib.grl_trade_dp_set_policy(engine.h, C.byref(g), p.shape[0], _ffi._ptr(p)))


_ENV_DTYPES = (("total", np.float64, ()), ("sum_sq", np.float64, ()), ("final_assets", np.float64, ()), ("min", np.float32, ()),
               ("max", np.float32, ()), ("length", np.int32, ()), ("finished", np.uint8, ()), ("depleted", np.uint8, ()))


def trade_dp_play(engine, max_steps=None, trace_steps=0, normals=None):
    """Every env plays a whole episode from the engine's CURRENT state under the engine's table, for up to max_steps steps
    (default: the engine's max_episode_steps); the engine's state is left as it was.  normals: None (the engine's own generator,
    at the counters its next steps would use) or a tape (max_steps, E, n_assets) whose row t moves the prices after step t.
    Returns total, sum_sq, final_assets (float64), min, max (float32), length (int32), finished, depleted (uint8), each (E,), and
    with trace_steps the first trace_steps steps of every env: actions (trace_steps, E, n_assets) float32, rewards (trace_steps, E)
    float32 and assets (trace_steps, E) float64, the account's value after the step; zero past an env's length."""
    lib = _trade(engine, "trade_dp_play")
    max_steps, _ = steps_and_trace(engine, "trade_dp_play", max_steps)
    n = int(engine.cfg.n_assets)
    tape = None
    if normals is not None:
        tape = np.asarray(normals, np.float32)
        if tape.shape != (max_steps, engine.E, n):
            raise ValueError("trade_dp_play: normals must be (max_steps, E, n_assets) = %s, got %s" % ((max_steps, engine.E, n), tape.shape))
        tape = np.ascontiguousarray(tape.transpose(0, 2, 1))        # the device layout: a * E + env per step
    engine._check(lib.grl_trade_dp_play(engine.h, None if tape is None else _ffi._ptr(tape), max_steps, int(trace_steps)))
    out = read_outputs(engine, lib.grl_trade_dp_play_read, _ENV_DTYPES, (engine.E,))
    if trace_steps > 0:
        T = int(trace_steps)
        out.update(read_outputs(engine, lib.grl_trade_dp_play_read, (("rewards", np.float32, ()), ("assets", np.float64, ())), (T, engine.E)))
        act = read_outputs(engine, lib.grl_trade_dp_play_read, (("actions", np.float32, ()),), (T, n, engine.E))["actions"]
        out["actions"] = np.ascontiguousarray(act.transpose(0, 2, 1))
    return out


def _axis(pos, n):
    pos = np.clip(pos, 0.0, float(n - 1))
    i = np.minimum(pos.astype(np.int64), n - 2)
    return i, pos - i


def _lerp(f, lo, hi):
    return (1.0 - f) * lo + f * hi


def trade_dp_actions(policy, grid, horizon, cash, q, p, remaining):
    """The look-up grl_trade_dp_play makes, in numpy float64.  policy: (horizon, [nu]^n, [nx]^n, n); cash (E,), q, p (E, n): the
    account the step begins with; remaining (E,): the steps left to the TimeLimit including this one, None without a TimeLimit.
    Row min(remaining - 1, horizon) - 1, the action 0 when remaining - 1 = 0; the 2n-linear blend (price axes first, asset 1
    innermost) at u_a = q_a p_a / W and x_a = log p_a, clamped to the grid, rounded once to float32.  Returns (E, n) float32."""
    tab = np.asarray(policy, np.float64)
    horizon = int(horizon)
    cash, q, p = np.asarray(cash, np.float64), np.asarray(q, np.float64), np.asarray(p, np.float64)
    E, n = q.shape
    nu, nx = int(grid["nu"]), int(grid["nx"])
    moves = np.full(E, horizon, np.int64) if remaining is None else np.asarray(remaining, np.int64) - 1
    row = np.minimum(np.maximum(moves, 1), horizon) - 1
    val = q * p
    W = cash.copy()
    for a in range(n):
        W = W + val[:, a]
    dx = (grid["x_max"] + grid["x_max"]) / float(nx - 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        axes = [_axis(np.nan_to_num(val[:, a] / W * float(nu - 1), nan=0.0), nu) for a in range(n)]
        axes += [_axis((np.log(p[:, a]) + grid["x_max"]) / dx, nx) for a in range(n)]

    def blend(d, index):
        if d == 2 * n:
            return tab[(row,) + tuple(index)]                       # (E, n)
        i, f = axes[d]
        return _lerp(f[:, None], blend(d + 1, index + [i]), blend(d + 1, index + [i + 1]))

    act = blend(0, []).astype(np.float32)
    act[moves <= 0] = 0.0
    return act
