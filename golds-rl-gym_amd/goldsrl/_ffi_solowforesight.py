"""ctypes binding of the perfect-foresight ceiling of the Solow env (C ABI: include/goldsrl_solowforesight.h): the shock path of an
episode is fixed by the tape its reset drew, so every env solves its own episode by backward induction on capital alone and plays
the plan, one workgroup per env, in one kernel launch.  The ARMA order is data: every (p, q) a handle can hold is served."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_episode import read_outputs, steps_and_trace
from ._ffi_solowarmadp import handle_rhos

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t
MAX_NK, MAX_NS = 1024, 256

# include/goldsrl_solowforesight.h: a dict of its own, as the header is a file of its own (tests/test_solow_foresight_header.py pins both)
SOLOW_FORESIGHT_SIGNATURES = {
    "grl_solow_foresight": (C.c_int, [_P, _P, _I, _I]),
    "grl_solow_foresight_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}


class SolowForesightGrid(C.Structure):
    """grl_solow_foresight_grid"""
    _fields_ = [("k_lo", C.c_double), ("k_hi", C.c_double), ("s_lo", C.c_double), ("s_hi", C.c_double), ("nk", _I), ("ns", _I)]


def shock_deviation(p, q, sigma):
    """The stationary deviation of z for the orders (p, q) under the handle's coefficients: sigma * sqrt(sum psi_j^2) over 4096
    impulse responses psi_0 = 1, psi_j = th_j + sum_l phi_l psi_{j-l}.  Any order."""
    rho_z, rho_e = handle_rhos(p, q)
    p, q = len(rho_z), len(rho_e)
    phi, th = rho_z[::-1], rho_e[::-1]                        # lag 1 first
    psi = [1.0]
    for j in range(1, 4096):
        a = th[j - 1] if j <= q else 0.0
        for l in range(1, min(j, p) + 1):
            a += phi[l - 1] * psi[j - l]
        psi.append(a)
    return float(sigma) * float(np.sqrt(np.sum(np.square(psi))))


def default_k_range(p, q, sigma, delta, sigmas=3.0):
    """(k_lo, k_hi) around the reset capital k_ss = (0.33 / delta)^(1 / 0.67).  Capital held at the steady state of a shock z is
    k_ss * exp(z / 0.67); the range reaches `sigmas` stationary deviations of z above it, and as far below with a further factor
    2.4 for the last steps of an episode, where the plan stops saving and capital runs down."""
    kss = (0.33 / float(delta)) ** (1.0 / 0.67)
    spread = float(np.exp(float(sigmas) * shock_deviation(p, q, sigma) / 0.67))
    return kss / (2.4 * spread), kss * spread


def solow_foresight_grid(engine, nk=96, ns=96, k_lo=None, k_hi=None, s_lo=0.001, s_hi=0.999):
    """The grid as a dict: nk points uniform in log k on [k_lo, k_hi] (default: default_k_range of the engine's orders, sigma and
    delta), ns rates uniform on [s_lo, s_hi]."""
    cfg = engine.cfg
    lo, hi = default_k_range(cfg.solow_p, cfg.solow_q, cfg.solow_sigma, cfg.solow_delta)
    return {"nk": int(nk), "ns": int(ns), "k_lo": float(lo if k_lo is None else k_lo), "k_hi": float(hi if k_hi is None else k_hi),
            "s_lo": float(s_lo), "s_hi": float(s_hi)}


def _grid_struct(grid):
    g = SolowForesightGrid()
    for name, _ in SolowForesightGrid._fields_:
        setattr(g, name, grid[name])
    return g


def _solow(engine, who):
    if engine.kind != _ffi.ENV_SOLOW:
        raise ValueError("%s: the engine is not a Solow engine" % who)
    return _ffi.load_library(extra_signatures=SOLOW_FORESIGHT_SIGNATURES)


_ENV_DTYPES = (("total", np.float64, ()), ("sum_sq", np.float64, ()), ("min", np.float32, ()), ("max", np.float32, ()),
               ("length", np.int32, ()), ("finished", np.uint8, ()), ("value", np.float64, ()), ("clamped", np.int32, ()))
_TRACE_DTYPES = (("actions", np.float32, ()), ("rewards", np.float32, ()), ("k", np.float32, ()))


def solow_foresight(engine, max_steps=None, trace_steps=0, grid=None, decisions=False):
    """Every env plans and plays a whole episode from the engine's CURRENT state (reset it first) knowing its shock path, for up to
    max_steps steps (default: the engine's max_episode_steps); the engine's state is left as it was.  Returns total, sum_sq, value
    (float64), min, max (float32), length, clamped (int32), finished (uint8), each (E,); ez (max_steps, E) float32, the path; "grid";
    with trace_steps the first trace_steps steps of every env: actions, rewards and k (the capital after the step), each
    (trace_steps, E) float32; with decisions the table (E, max_steps, nk) uint8 (refused when the call took several launches)."""
    lib = _solow(engine, "solow_foresight")
    max_steps, _ = steps_and_trace(engine, "solow_foresight", max_steps)
    if grid is None:
        grid = solow_foresight_grid(engine)
    g = _grid_struct(grid)
    engine._check(lib.grl_solow_foresight(engine.h, C.byref(g), max_steps, int(trace_steps)))
    out = read_outputs(engine, lib.grl_solow_foresight_read, _ENV_DTYPES, (engine.E,))
    out.update(read_outputs(engine, lib.grl_solow_foresight_read, (("ez", np.float32, ()),), (max_steps, engine.E)))
    if trace_steps > 0:
        out.update(read_outputs(engine, lib.grl_solow_foresight_read, _TRACE_DTYPES, (int(trace_steps), engine.E)))
    if decisions:
        out.update(read_outputs(engine, lib.grl_solow_foresight_read, (("decisions", np.uint8, ()),), (engine.E, max_steps, grid["nk"])))
    out["grid"] = grid
    return out


def solow_foresight_actions(decisions, grid, t, k):
    """The look-up the play makes at step t, in numpy float64: the rates s_lo + a * ds of the two nodes bracketing log k, blended,
    clamped to the grid, rounded once to float32.  decisions (E, T, nk) uint8, k (E,)."""
    dec = np.asarray(decisions)
    nk, ns = int(grid["nk"]), int(grid["ns"])
    lk_lo = np.log(grid["k_lo"])
    dlk = (np.log(grid["k_hi"]) - lk_lo) / float(nk - 1)
    ds = (grid["s_hi"] - grid["s_lo"]) / float(ns - 1)
    u = np.clip((np.log(np.asarray(k, np.float64)) - lk_lo) / dlk, 0.0, float(nk - 1))
    i = np.minimum(u.astype(np.int64), nk - 2)
    f = u - i
    env = np.arange(dec.shape[0])
    s0 = grid["s_lo"] + dec[env, t, i].astype(np.float64) * ds
    s1 = grid["s_lo"] + dec[env, t, i + 1].astype(np.float64) * ds
    return ((1.0 - f) * s0 + f * s1).astype(np.float32)
