"""The recurrence of include/goldsrl_tradedp.h in plain numpy float64, one IEEE operation after the other in the header's order, so
that only exp / log differ from csrc/trade_dp.hip.  Tables are ([nu]^n flattened, [nx]^n flattened): share node s = i_0 * nu + i_1,
price node i_0 * nx + i_1."""
import numpy as np


def _axis(pos, n):
    pos = np.clip(pos, 0.0, float(n - 1))
    i = np.minimum(pos.astype(np.int64), n - 2)
    return i, pos - i


def _lerp(f, lo, hi):
    return (1.0 - f) * lo + f * hi


def actions(grid, n):
    """(na^n, n): the joint action grid, joint index i_0 * na + i_1"""
    na = grid["na"]
    a = (2 * np.arange(na) - (na - 1)).astype(np.float64) / float(na - 1)
    return a[:, None] if n == 1 else np.stack([np.repeat(a, na), np.tile(a, na)], axis=1)


def shares(grid, n):
    """(nu^n, n): the state every share node stands for"""
    nu = grid["nu"]
    u = np.arange(nu).astype(np.float64) / float(nu - 1)
    if n == 1:
        return u[:, None]
    u0, u1 = np.repeat(u, nu), np.tile(u, nu)
    s = u0 + u1
    over = s > 1.0
    return np.stack([np.where(over, u0 / np.where(over, s, 1.0), u0), np.where(over, u1 / np.where(over, s, 1.0), u1)], axis=1)


def q_values(grid, n, V, act):
    """Q (NU, NX, A) of the actions act, broadcastable to (NU, NX, A, n), over the value V (NU, NX) of the stage below."""
    nu, nx, nq = grid["nu"], grid["nx"], grid["nq"]
    NU, NX = nu ** n, nx ** n
    e, w = np.asarray(grid["e_nodes"], np.float64), np.asarray(grid["e_weights"], np.float64)
    dx = (grid["x_max"] + grid["x_max"]) / float(nx - 1)
    x = -grid["x_max"] + np.arange(nx).astype(np.float64) * dx
    xp = (0.9 * x)[:, None] + e[None]                                   # (nx, nq)
    R = np.exp(xp - x[:, None])
    ix, fx = _axis((xp + grid["x_max"]) / dx, nx)
    act = np.asarray(act, np.float64)
    u = shares(grid, n)[:, None, None, :]                               # (NU, 1, 1, n)
    c = 1.0 - u[..., 0]
    if n == 2:
        c = c - u[..., 1]
    up = np.where(act > 0.0, u + (act / float(n)) * c[..., None], u * (1.0 + act))
    cp = 1.0 - up[..., 0]
    if n == 2:
        cp = cp - up[..., 1]
    xn = np.arange(NX)
    x0, x1 = (xn, None) if n == 1 else (xn // nx, xn % nx)
    Vg = V.reshape((NU,) + (nx,) * n)
    acc = 0.0
    for k0 in range(nq):
        y0 = up[..., 0] * R[x0, k0][None, :, None]
        if n == 1:
            S = _lerp(fx[x0, k0][None], Vg[:, ix[x0, k0]], Vg[:, ix[x0, k0] + 1])             # (NU, NX): the slab of node k0
            g = cp + y0
            i0, f0 = _axis(y0 / g * float(nu - 1), nu)
            v = _lerp(f0, S[i0, xn[None, :, None]], S[i0 + 1, xn[None, :, None]])
            acc = acc + w[k0] * (np.log(g) + v)
            continue
        for k1 in range(nq):
            a0, a1, f1 = ix[x0, k0], ix[x1, k1], fx[x1, k1][None]
            S = _lerp(fx[x0, k0][None], _lerp(f1, Vg[:, a0, a1], Vg[:, a0, a1 + 1]), _lerp(f1, Vg[:, a0 + 1, a1], Vg[:, a0 + 1, a1 + 1]))
            S = S.reshape(nu, nu, NX)
            y1 = up[..., 1] * R[x1, k1][None, :, None]
            g = cp + y0
            g = g + y1
            (i0, f0), (i1, f1) = _axis(y0 / g * float(nu - 1), nu), _axis(y1 / g * float(nu - 1), nu)
            col = xn[None, :, None]
            v = _lerp(f0, _lerp(f1, S[i0, i1, col], S[i0, i1 + 1, col]), _lerp(f1, S[i0 + 1, i1, col], S[i0 + 1, i1 + 1, col]))
            acc = acc + (w[k0] * w[k1]) * (np.log(g) + v)
    return acc


def stage(grid, n, V):
    """(V_{j+1} (NU, NX), its policy (NU, NX, n) float32) from V_j: the lowest joint index keeps a tie"""
    acts = actions(grid, n)
    Q = q_values(grid, n, V, acts[None, None])
    best = Q.argmax(axis=2)
    return np.take_along_axis(Q, best[..., None], axis=2)[..., 0], acts[best].astype(np.float32)


def solve(grid, n, horizon):
    """(policy (horizon, NU, NX, n) float32, row s with s + 1 moves left; the top stage's value (NU, NX))"""
    V = np.zeros((grid["nu"] ** n, grid["nx"] ** n))
    rows = []
    for _ in range(horizon):
        V, pol = stage(grid, n, V)
        rows.append(pol)
    return np.stack(rows), V
