"""ctypes binding of the optimal-savings yardstick of the Solow env at the orders _ffi_solowdp refuses (C ABI:
include/goldsrl_solowarmadp.h): backward induction on a (f_0, .., f_{m-1}, k) grid, f the m = max(p, q + 1) forecasts that make the
ARMA(p, q) shock Markov, one kernel launch per stage, and the play of the tabulated policy, every env a whole episode in one
launch.  The model derivation is restated here in the C side's operation order, so that a grid can be built without a device."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_episode import read_outputs, steps_and_trace

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t
MAX_DIM, MAX_LAGS, MAX_NODES = 4, 8, 15

# include/goldsrl_solowarmadp.h: a dict of its own, as the header is a file of its own (tests/test_solow_arma_dp_header.py pins both)
SOLOW_ARMA_DP_SIGNATURES = {
    "grl_solow_arma_model": (C.c_int, [_P, _P]),
    "grl_solow_arma_dp_solve": (C.c_int, [_P, _P, _I]),
    "grl_solow_arma_dp_set_policy": (C.c_int, [_P, _P, _I, _P]),
    "grl_solow_arma_dp_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
    "grl_solow_arma_dp_play": (C.c_int, [_P, _I, _I]),
    "grl_solow_arma_dp_play_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}

DEFAULT_HORIZON = 128


class SolowArmaCoef(C.Structure):
    """grl_solow_arma_coef"""
    _fields_ = [("A", C.c_double * (MAX_DIM * MAX_DIM)), ("b", C.c_double * MAX_DIM), ("Mz", C.c_double * (MAX_DIM * MAX_LAGS)),
                ("Me", C.c_double * (MAX_DIM * MAX_LAGS)), ("f_std", C.c_double * MAX_DIM), ("m", _I), ("p", _I), ("q", _I)]


class SolowArmaDpGrid(C.Structure):
    """grl_solow_arma_dp_grid"""
    _fields_ = [("k_lo", C.c_double), ("k_hi", C.c_double), ("x_max", C.c_double * MAX_DIM), ("s_lo", C.c_double), ("s_hi", C.c_double),
                ("e_nodes", C.c_double * MAX_NODES), ("e_weights", C.c_double * MAX_NODES),
                ("nk", _I), ("ns", _I), ("nq", _I), ("nx", _I * MAX_DIM)]


def handle_rhos(p, q):
    """rho_z (p,) and rho_e (max(q, 1),) as a handle holds them: SolowEnv.__init__'s numbers rounded to float32, here as float64.
    With q = 0 the env keeps one innovation under rho_e = [0.5] (fed_env.py:184-187, 226)."""
    w = 0.5 ** np.arange(1, p + 1)
    rho_z = (w / (w.sum() / 0.95)).astype(np.float32).astype(np.float64)
    rho_e = (0.5 ** np.arange(1, max(q, 1) + 1)).astype(np.float32).astype(np.float64)
    return rho_z, rho_e


def solow_arma_model(p, q, sigma=0.1, rho_z=None, rho_e=None):
    """The model of include/goldsrl_solowarmadp.h for the orders (p, q), float64, in grl_solow_arma_model's operation order:
    {"m", "p", "q" (as the handle counts it: at least 1), "A" (m, m), "b" (m,), "Mz" (m, p), "Me" (m, q), "f_std" (m,)}.
    rho_z, rho_e: the coefficients oldest lag first (default: the handle's float32 ones).  ValueError for p < 1 or m > 4."""
    p, q = int(p), max(int(q), 1)
    m = max(p, q + 1)
    if p < 1 or m > MAX_DIM:
        raise ValueError("Solow-%d-%d: the shock's state has m = max(p, q + 1) = %d numbers; the grid covers p >= 1 and m <= %d" % (p, q, m, MAX_DIM))
    if rho_z is None:
        rho_z, rho_e = handle_rhos(p, q)
    phi = [0.0] + [float(rho_z[p - l]) for l in range(1, p + 1)]
    th = [0.0] + [float(rho_e[q - l]) for l in range(1, q + 1)] + [0.0] * MAX_DIM
    b = [1.0]
    for j in range(1, m):
        a = th[j]
        for l in range(1, min(j, p) + 1):
            a += phi[l] * b[j - l]
        b.append(a)
    A = np.zeros((m, m))
    for j in range(m - 1):
        A[j, j + 1] = 1.0
    for l in range(1, p + 1):
        A[m - 1, m - l] = phi[l]
    Mz, Me = np.zeros((m, p)), np.zeros((m, q))
    Mz[0, p - 1] = 1.0
    for j in range(1, m):
        for i in range(p):
            a = 0.0
            for l in range(1, p + 1):
                if j - l >= 0:
                    a += phi[l] * Mz[j - l, i]
                elif i == p - 1 - (l - j):
                    a += phi[l]
            Mz[j, i] = a
        for i in range(q):
            a = 0.0
            for l in range(1, min(j, p) + 1):
                a += phi[l] * Me[j - l, i]
            for l in range(j, q + 1):
                if i == q - 1 - (l - j):
                    a += th[l]
            Me[j, i] = a
    v, acc = list(b), [0.0] * m
    for _ in range(1024):
        nv = []
        for j in range(m):
            acc[j] += v[j] * v[j]
            a = 0.0
            for l in range(m):
                a += float(A[j, l]) * v[l]
            nv.append(a)
        v = nv
    return {"m": m, "p": p, "q": q, "A": A, "b": np.array(b), "Mz": Mz, "Me": Me, "f_std": float(sigma) * np.sqrt(np.array(acc))}


def solow_arma_model_device(engine):
    """grl_solow_arma_model of the engine's handle, in solow_arma_model's form"""
    lib = _solow(engine, "solow_arma_model_device")
    c = SolowArmaCoef()
    engine._check(lib.grl_solow_arma_model(engine.h, C.byref(c)))
    m, p, q = c.m, c.p, c.q
    return {"m": m, "p": p, "q": q, "A": np.array(c.A).reshape(MAX_DIM, MAX_DIM)[:m, :m], "b": np.array(c.b)[:m],
            "Mz": np.array(c.Mz).reshape(MAX_DIM, MAX_LAGS)[:m, :p], "Me": np.array(c.Me).reshape(MAX_DIM, MAX_LAGS)[:m, :q],
            "f_std": np.array(c.f_std)[:m]}


def solow_arma_dp_grid(p, q, nk=48, nx=9, nq=3, ns=48, k_lo=5.0, k_hi=400.0, x_max=None, x_sigmas=3.0, s_lo=0.001, s_hi=0.999, sigma=0.1):
    """The grid of the orders (p, q) as a dict: the sizes (nx: one number for every axis, or m of them), the ranges (x_max: m
    half-widths; default x_sigmas stationary deviations of each forecast), the Gauss-Hermite rule for eps ~ N(0, sigma^2) as in
    _ffi_solowdp.solow_dp_grid, and "model", solow_arma_model(p, q, sigma).  sigma is the engine's solow_sigma."""
    if not 1 <= int(nq) <= MAX_NODES:
        raise ValueError("nq must be in 1..%d" % MAX_NODES)
    model = solow_arma_model(p, q, sigma)
    m = model["m"]
    nx = [int(nx)] * m if np.ndim(nx) == 0 else [int(n) for n in nx]
    x_max = [float(x_sigmas) * float(s) for s in model["f_std"]] if x_max is None else [float(x) for x in x_max]
    if len(nx) != m or len(x_max) != m:
        raise ValueError("Solow-%d-%d has m = %d shock axes: nx and x_max need %d numbers each" % (p, q, m, m))
    x, w = np.polynomial.hermite_e.hermegauss(int(nq))
    return {"nk": int(nk), "nx": nx, "nq": int(nq), "ns": int(ns), "k_lo": float(k_lo), "k_hi": float(k_hi), "x_max": x_max,
            "s_lo": float(s_lo), "s_hi": float(s_hi), "sigma": float(sigma), "model": model,
            "e_nodes": np.asarray(float(sigma) * x, np.float64), "e_weights": np.asarray(w / w.sum(), np.float64)}


def _grid_struct(grid):
    g = SolowArmaDpGrid()
    for name in ("k_lo", "k_hi", "s_lo", "s_hi", "nk", "ns", "nq"):
        setattr(g, name, grid[name])
    for j in range(min(len(grid["nx"]), MAX_DIM)):
        g.nx[j], g.x_max[j] = grid["nx"][j], grid["x_max"][j]
    for j in range(min(int(grid["nq"]), MAX_NODES)):
        g.e_nodes[j], g.e_weights[j] = float(grid["e_nodes"][j]), float(grid["e_weights"][j])
    return g


def table_shape(grid, horizon):
    """(horizon, nx[0], .., nx[m-1], nk)"""
    return (int(horizon),) + tuple(grid["nx"]) + (grid["nk"],)


def _solow(engine, who):
    if engine.kind != _ffi.ENV_SOLOW:
        raise ValueError("%s: the engine is not a Solow engine" % who)
    return _ffi.load_library(extra_signatures=SOLOW_ARMA_DP_SIGNATURES)


def engine_grid(engine, **sizes):
    """solow_arma_dp_grid for the engine's orders and sigma"""
    return solow_arma_dp_grid(engine.cfg.solow_p, engine.cfg.solow_q, sigma=engine.cfg.solow_sigma, **sizes)


def solow_arma_dp_solve(engine, grid=None, horizon=DEFAULT_HORIZON, read=True):
    """Backward induction over `horizon` stages on `grid` (default: engine_grid(engine)) for the engine's model; the engine keeps
    the tables for solow_arma_dp_play.  Returns {"grid", "horizon"} and, with read, "policy" (horizon, nx.., nk) float32 and
    "value" (nx.., nk) float64, stage 0's."""
    lib = _solow(engine, "solow_arma_dp_solve")
    if grid is None:
        grid = engine_grid(engine)
    g = _grid_struct(grid)
    engine._check(lib.grl_solow_arma_dp_solve(engine.h, C.byref(g), int(horizon)))
    out = {"grid": grid, "horizon": int(horizon)}
    if read:
        shape = table_shape(grid, horizon)
        out.update(read_outputs(engine, lib.grl_solow_arma_dp_read, (("policy", np.float32, shape), ("value", np.float64, shape[1:])), ()))
    return out


def solow_arma_dp_set_policy(engine, grid, policy):
    """Upload policy (horizon, nx.., nk) in place of a solved table: solow_arma_dp_play then plays it."""
    lib = _solow(engine, "solow_arma_dp_set_policy")
    p = np.ascontiguousarray(policy, np.float32)
    if p.ndim < 3 or p.shape[1:] != table_shape(grid, 1)[1:]:
        raise ValueError("solow_arma_dp_set_policy: expected (horizon,) + %s, got %s" % (table_shape(grid, 1)[1:], p.shape))
    g = _grid_struct(grid)
    engine._check(lib.grl_solow_arma_dp_set_policy(engine.h, C.byref(g), p.shape[0], _ffi._ptr(p)))


_ENV_DTYPES = (("total", np.float64, ()), ("sum_sq", np.float64, ()), ("min", np.float32, ()), ("max", np.float32, ()),
               ("length", np.int32, ()), ("finished", np.uint8, ()))
_TRACE_DTYPES = (("actions", np.float32, ()), ("rewards", np.float32, ()), ("k", np.float32, ()))


def solow_arma_dp_play(engine, max_steps=None, trace_steps=0):
    """Every env plays a whole episode from the engine's CURRENT state (reset it first) under the engine's table, for up to
    max_steps steps (default: the engine's max_episode_steps); the engine's state is left as it was.  Returns total, sum_sq
    (float64), min, max (float32), length (int32), finished (uint8), each (E,), and with trace_steps the first trace_steps steps of
    every env: actions, rewards and k (the capital after the step), each (trace_steps, E) float32."""
    lib = _solow(engine, "solow_arma_dp_play")
    max_steps, _ = steps_and_trace(engine, "solow_arma_dp_play", max_steps)
    engine._check(lib.grl_solow_arma_dp_play(engine.h, max_steps, int(trace_steps)))
    out = read_outputs(engine, lib.grl_solow_arma_dp_play_read, _ENV_DTYPES, (engine.E,))
    if trace_steps > 0:
        out.update(read_outputs(engine, lib.grl_solow_arma_dp_play_read, _TRACE_DTYPES, (int(trace_steps), engine.E)))
    return out


def _axis(x, lo, step, n):
    u = np.clip((x - lo) / step, 0.0, float(n - 1))
    i = np.minimum(u.astype(np.int64), n - 2)
    return i, u - i


def solow_arma_dp_policy_actions(grid, table, k, zv, ev):
    """The look-up grl_solow_arma_dp_play makes, in numpy float64: f = Mz zv + Me ev (z terms, then e terms, oldest lag first), then
    the (m+1)-linear blend of one stage's table (nx.., nk) at (f, k) -- corners of the f-axes ascending, bit d the upper neighbour on
    axis d, the blend in k innermost -- clamped to the grid, rounded once to float32.  k (E,), zv (E, p), ev (E, q)."""
    tab = np.asarray(table, np.float64)
    model, m, nk = grid["model"], grid["model"]["m"], tab.shape[-1]
    k, zv, ev = np.asarray(k, np.float64), np.asarray(zv, np.float64), np.asarray(ev, np.float64)
    lk_lo = np.log(grid["k_lo"])
    ik, fk = _axis(np.log(k), lk_lo, (np.log(grid["k_hi"]) - lk_lo) / float(nk - 1), nk)
    cx = []
    for d in range(m):
        f = np.zeros(k.shape)
        for i in range(model["p"]):
            f = f + model["Mz"][d, i] * zv[:, i]
        for i in range(model["q"]):
            f = f + model["Me"][d, i] * ev[:, i]
        x_max, n = grid["x_max"][d], grid["nx"][d]
        cx.append(_axis(f, -x_max, (x_max + x_max) / float(n - 1), n))
    acc = np.zeros(k.shape)
    for c in range(1 << m):
        wt, idx = np.ones(k.shape), []
        for d in range(m):
            bit = (c >> d) & 1
            idx.append(cx[d][0] + bit)
            wt = wt * (cx[d][1] if bit else 1.0 - cx[d][1])
        acc = acc + wt * ((1.0 - fk) * tab[tuple(idx) + (ik,)] + fk * tab[tuple(idx) + (ik + 1,)])
    return acc.astype(np.float32)
