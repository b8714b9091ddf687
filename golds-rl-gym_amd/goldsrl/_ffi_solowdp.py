"""ctypes binding of the optimal-savings yardstick of the Solow env (C ABI: include/goldsrl_solowdp.h): backward induction on a
(k, z, e) grid, one kernel launch per stage, and the play of the tabulated policy, every env a whole episode in one launch."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_episode import read_outputs, steps_and_trace

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t
MAX_NODES = 15

# include/goldsrl_solowdp.h: a dict of its own, as the header is a file of its own (tests/test_solow_dp_header.py pins both)
SOLOW_DP_SIGNATURES = {
    "grl_solow_dp_solve": (C.c_int, [_P, _P, _I]),
    "grl_solow_dp_set_policy": (C.c_int, [_P, _P, _I, _P]),
    "grl_solow_dp_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
    "grl_solow_dp_play": (C.c_int, [_P, _I, _I]),
    "grl_solow_dp_play_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}

DEFAULT_HORIZON = 256


class SolowDpGrid(C.Structure):
    """grl_solow_dp_grid"""
    _fields_ = [("k_lo", C.c_double), ("k_hi", C.c_double), ("z_max", C.c_double), ("s_lo", C.c_double), ("s_hi", C.c_double),
                ("e_nodes", C.c_double * MAX_NODES), ("e_weights", C.c_double * MAX_NODES),
                ("nk", _I), ("nz", _I), ("nq", _I), ("ns", _I)]


def solow_dp_grid(nk=96, nz=25, nq=7, ns=96, k_lo=5.0, k_hi=400.0, z_max=1.6, s_lo=0.001, s_hi=0.999, sigma=0.1):
    """The grid as a dict: the sizes, the ranges, and the Gauss-Hermite rule for eps ~ N(0, sigma^2): e_nodes = sigma * x_j
    (ascending) and e_weights normalised to sum 1, float64 (numpy.polynomial.hermite_e.hermegauss).  sigma is the engine's
    solow_sigma."""
    if not 1 <= int(nq) <= MAX_NODES:
        raise ValueError("nq must be in 1..%d" % MAX_NODES)
    x, w = np.polynomial.hermite_e.hermegauss(int(nq))
    return {"nk": int(nk), "nz": int(nz), "nq": int(nq), "ns": int(ns), "k_lo": float(k_lo), "k_hi": float(k_hi), "z_max": float(z_max),
            "s_lo": float(s_lo), "s_hi": float(s_hi), "sigma": float(sigma),
            "e_nodes": np.asarray(float(sigma) * x, np.float64), "e_weights": np.asarray(w / w.sum(), np.float64)}


def _grid_struct(grid):
    g = SolowDpGrid()
    for name in ("k_lo", "k_hi", "z_max", "s_lo", "s_hi", "nk", "nz", "nq", "ns"):
        setattr(g, name, grid[name])
    for j in range(min(int(grid["nq"]), MAX_NODES)):
        g.e_nodes[j], g.e_weights[j] = float(grid["e_nodes"][j]), float(grid["e_weights"][j])
    return g


def table_shape(engine, grid, horizon):
    """(horizon, nk, nz, ne) of the engine's policy table on `grid`: ne = nq for q = 1, 1 for q = 0"""
    return (int(horizon), grid["nk"], grid["nz"], grid["nq"] if engine.cfg.solow_q > 0 else 1)


def _solow(engine, who):
    if engine.kind != _ffi.ENV_SOLOW:
        raise ValueError("%s: the engine is not a Solow engine" % who)
    return _ffi.load_library(extra_signatures=SOLOW_DP_SIGNATURES)


def solow_dp_solve(engine, grid=None, horizon=DEFAULT_HORIZON, read=True):
    """Backward induction over `horizon` stages on `grid` (default: solow_dp_grid() at the engine's sigma) for the engine's model;
    the engine keeps the tables for solow_dp_play.  Returns {"grid", "horizon"} and, with read, "policy" (horizon, nk, nz, ne)
    float32 and "value" (nk, nz, ne) float64, stage 0's."""
    lib = _solow(engine, "solow_dp_solve")
    if grid is None:
        grid = solow_dp_grid(sigma=engine.cfg.solow_sigma)
    g = _grid_struct(grid)
    engine._check(lib.grl_solow_dp_solve(engine.h, C.byref(g), int(horizon)))
    out = {"grid": grid, "horizon": int(horizon)}
    if read:
        shape = table_shape(engine, grid, horizon)
        out.update(read_outputs(engine, lib.grl_solow_dp_read, (("policy", np.float32, shape), ("value", np.float64, shape[1:])), ()))
    return out


def solow_dp_set_policy(engine, grid, policy):
    """Upload policy (horizon, nk, nz, ne) in place of a solved table: solow_dp_play then plays it."""
    lib = _solow(engine, "solow_dp_set_policy")
    p = np.ascontiguousarray(policy, np.float32)
    if p.ndim != 4 or p.shape[1:] != table_shape(engine, grid, 1)[1:]:
        raise ValueError("solow_dp_set_policy: expected (horizon,) + %s, got %s" % (table_shape(engine, grid, 1)[1:], p.shape))
    g = _grid_struct(grid)
    engine._check(lib.grl_solow_dp_set_policy(engine.h, C.byref(g), p.shape[0], _ffi._ptr(p)))


_ENV_DTYPES = (("total", np.float64, ()), ("sum_sq", np.float64, ()), ("min", np.float32, ()), ("max", np.float32, ()),
               ("length", np.int32, ()), ("finished", np.uint8, ()))
_TRACE_DTYPES = (("actions", np.float32, ()), ("rewards", np.float32, ()), ("k", np.float32, ()))


def solow_dp_play(engine, max_steps=None, trace_steps=0):
    """Every env plays a whole episode from the engine's CURRENT state (reset it first) under the engine's table, for up to
    max_steps steps (default: the engine's max_episode_steps); the engine's state is left as it was.  Returns total, sum_sq
    (float64), min, max (float32), length (int32), finished (uint8), each (E,), and with trace_steps the first trace_steps steps of
    every env: actions, rewards and k (the capital after the step), each (trace_steps, E) float32."""
    lib = _solow(engine, "solow_dp_play")
    max_steps, _ = steps_and_trace(engine, "solow_dp_play", max_steps)
    engine._check(lib.grl_solow_dp_play(engine.h, max_steps, int(trace_steps)))
    out = read_outputs(engine, lib.grl_solow_dp_play_read, _ENV_DTYPES, (engine.E,))
    if trace_steps > 0:
        out.update(read_outputs(engine, lib.grl_solow_dp_play_read, _TRACE_DTYPES, (int(trace_steps), engine.E)))
    return out


def _axis(x, lo, step, n):
    u = np.clip((x - lo) / step, 0.0, float(n - 1))
    i = np.minimum(u.astype(np.int64), n - 2)
    return i, u - i


def solow_dp_policy_actions(grid, table, k, z, e):
    """The look-up grl_solow_dp_play makes, in numpy float64: the trilinear blend of one stage's table (nk, nz, ne) at the states
    (k, z, e) (arrays of one shape, e the previous innovation), clamped to the grid, rounded once to float32."""
    tab = np.asarray(table, np.float64)
    nk, nz, ne = tab.shape
    k, z, e = (np.asarray(v, np.float64) for v in (k, z, e))
    lk_lo = np.log(grid["k_lo"])
    dlk = (np.log(grid["k_hi"]) - lk_lo) / float(nk - 1)
    dz = (grid["z_max"] + grid["z_max"]) / float(nz - 1)
    ik, fk = _axis(np.log(k), lk_lo, dlk, nk)
    iz, fz = _axis(z, -grid["z_max"], dz, nz)
    if ne > 1:
        nodes = np.asarray(grid["e_nodes"], np.float64)[:ne]
        ee = np.clip(e, nodes[0], nodes[-1])
        j0 = np.clip(np.searchsorted(nodes, ee, side="right") - 1, 0, ne - 2)
        fe = (ee - nodes[j0]) / (nodes[j0 + 1] - nodes[j0])
        j1 = j0 + 1
    else:
        j0 = j1 = np.zeros(k.shape, np.int64)
        fe = np.zeros(k.shape)

    def plane(j):
        v0 = (1.0 - fk) * tab[ik, iz, j] + fk * tab[ik + 1, iz, j]
        v1 = (1.0 - fk) * tab[ik, iz + 1, j] + fk * tab[ik + 1, iz + 1, j]
        return (1.0 - fz) * v0 + fz * v1

    return ((1.0 - fe) * plane(j0) + fe * plane(j1)).astype(np.float32)
