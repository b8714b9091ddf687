"""The savings problem of the Solow env at any ARMA(p, q) shock by backward induction on the shock's minimal state, in numpy
float64: the yardstick of grl_solow_arma_dp_solve (include/goldsrl_solowarmadp.h).  Written from the header, one IEEE operation
per operation of the formulas and in their order, so that a faithful float64 implementation differs only through exp / log / pow.

    f_j = E_t[z_{t+j}], j < m = max(p, q + 1);  f' = A f + b eps;  f = Mz zv + Me ev
    W(f; k) = sum_j w_j sum_corners wt * V_next[corner of A f + b e_j][k]          nodes outer, corners ascending inner
    Q(k, f; s) = log((1 - s) y + 1e-4) + lerp(W(f; .), log k'),  y = exp(f_0) k^0.33,  k' = (1 - delta) k + s y

grid: the dict of goldsrl._ffi_solowarmadp.solow_arma_dp_grid, of which only the sizes, ranges, nodes and weights are read."""
import numpy as np

ALPHA = 0.33


def model(rho_z, rho_e):
    """(A, b, Mz, Me) from the env's coefficients, oldest lag first, as SolowEnv._step multiplies them."""
    p, q = len(rho_z), len(rho_e)
    m = max(p, q + 1)
    phi = [0.0] + [float(rho_z[p - l]) for l in range(1, p + 1)]
    th = [0.0] + [float(rho_e[q - l]) for l in range(1, q + 1)] + [0.0] * m
    psi = [1.0]
    for j in range(1, m):
        a = th[j]
        for l in range(1, min(j, p) + 1):
            a += phi[l] * psi[j - l]
        psi.append(a)
    A = np.zeros((m, m))
    A[np.arange(m - 1), np.arange(1, m)] = 1.0
    for l in range(1, p + 1):
        A[m - 1, m - l] = phi[l]
    # E_t[z_{t+j}] = sum_l phi_l E_t[z_{t+j-l}] + sum_{l >= j} th_l eps_{t+j-l}: a term at or before t is a lag of the env
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
    return A, np.array(psi), Mz, Me


def f_std(A, b, sigma):
    """sigma * sqrt(sum_{i < 1024} (A^i b)_j^2), the rows of A v added left to right"""
    v, acc = np.array(b, np.float64), np.zeros(len(b))
    for _ in range(1024):
        acc = acc + v * v
        nv = np.zeros(len(b))
        for l in range(len(b)):
            nv = nv + A[:, l] * v[l]
        v = nv
    return sigma * np.sqrt(acc)


def coord(x, lo, step, n):
    u = np.clip((x - lo) / step, 0.0, float(n - 1))
    i = np.minimum(u.astype(np.int64), n - 2)
    return i, u - i


def corners_of(cx):
    """[(index tuple, weight)] of the 2^m corners around the coordinates cx = [(i, fraction)] per axis: ascending, bit d of the
    corner the upper neighbour on axis d, the weight multiplied up from axis 0"""
    out = []
    for c in range(1 << len(cx)):
        wt, idx = np.ones(len(cx[0][0])), []
        for d, (i, fr) in enumerate(cx):
            bit = (c >> d) & 1
            idx.append(i + bit)
            wt = wt * (fr if bit else 1.0 - fr)
        out.append((tuple(idx), wt))
    return out


def _axes(grid, m):
    nk, ns = grid["nk"], grid["ns"]
    lk_lo = np.log(grid["k_lo"])
    dlk = (np.log(grid["k_hi"]) - lk_lo) / float(nk - 1)
    dx = [(grid["x_max"][d] + grid["x_max"][d]) / float(grid["nx"][d] - 1) for d in range(m)]
    return lk_lo, dlk, dx, (grid["s_hi"] - grid["s_lo"]) / float(ns - 1)


def solve(grid, horizon, A, b, delta):
    """Returns policy (horizon, nx.., nk) float32, value (nx.., nk) float64 of stage 0, and min_gap: the smallest difference between
    the best and the second-best Q over all states and stages."""
    m, nk, ns, nq = len(b), grid["nk"], grid["ns"], grid["nq"]
    nx = tuple(grid["nx"][:m])
    lk_lo, dlk, dx, ds = _axes(grid, m)
    nodes, w = np.asarray(grid["e_nodes"], np.float64), np.asarray(grid["e_weights"], np.float64)
    index = np.indices(nx).reshape(m, -1)                                # row-major over the f-axes, the last one fastest
    F = [-grid["x_max"][d] + index[d] * dx[d] for d in range(m)]         # m arrays (NX,)
    corners = []                                                         # [j][c] = (index tuple, weight (NX,))
    for j in range(nq):
        cx = []
        for d in range(m):
            a = np.zeros(len(F[0]))
            for l in range(m):
                a = a + A[d, l] * F[l]
            cx.append(coord(a + b[d] * nodes[j], -grid["x_max"][d], dx[d], nx[d]))
        corners.append(corners_of(cx))
    k, s = np.exp(lk_lo + np.arange(nk) * dlk), grid["s_lo"] + np.arange(ns) * ds
    y = (np.exp(F[0])[:, None] * np.power(k, ALPHA)[None, :])[:, :, None]                # (NX, nk, 1)
    r = np.log((1.0 - s) * y + 1e-4)                                                     # (NX, nk, ns)
    ik, fk = coord(np.log((1.0 - delta) * k[None, :, None] + s * y), lk_lo, dlk, nk)
    policy = np.zeros((horizon,) + nx + (nk,), np.float32)
    v_next, min_gap = None, np.inf
    for t in range(horizon - 1, -1, -1):
        cont = np.zeros(r.shape)
        if v_next is not None:
            W = np.zeros((len(F[0]), nk))
            for j in range(nq):
                inner = np.zeros(W.shape)
                for idx, wt in corners[j]:
                    inner = inner + wt[:, None] * v_next[idx]
                W = W + w[j] * inner
            lo = np.take_along_axis(W[:, None, :], ik.reshape(len(W), 1, -1), axis=2).reshape(ik.shape)
            hi = np.take_along_axis(W[:, None, :], ik.reshape(len(W), 1, -1) + 1, axis=2).reshape(ik.shape)
            cont = (1.0 - fk) * lo + fk * hi
        q = r + cont
        best = q.argmax(axis=2)
        top = np.partition(q, ns - 2, axis=2)[..., ns - 2:]
        min_gap = min(min_gap, float((top[..., 1] - top[..., 0]).min()))
        policy[t] = (grid["s_lo"] + best * ds).astype(np.float32).reshape(nx + (nk,))
        v_next = q.max(axis=2).reshape(nx + (nk,))
    return policy, v_next, min_gap


def lookup(grid, table, Mz, Me, k, zv, ev):
    """The play's action: the (m+1)-linear blend of one stage's table (nx.., nk) at f = Mz zv + Me ev and k, float32."""
    tab = np.asarray(table, np.float64)
    m, nk = len(Mz), tab.shape[-1]
    lk_lo, dlk, dx, _ = _axes(grid, m)
    ik, fk = coord(np.log(np.asarray(k, np.float64)), lk_lo, dlk, nk)
    cx = []
    for d in range(m):
        f = np.zeros(len(k))
        for i in range(Mz.shape[1]):
            f = f + Mz[d, i] * np.asarray(zv, np.float64)[:, i]
        for i in range(Me.shape[1]):
            f = f + Me[d, i] * np.asarray(ev, np.float64)[:, i]
        cx.append(coord(f, -grid["x_max"][d], dx[d], grid["nx"][d]))
    acc = np.zeros(len(k))
    for idx, wt in corners_of(cx):
        acc = acc + wt * ((1.0 - fk) * tab[idx + (ik,)] + fk * tab[idx + (ik + 1,)])
    return acc.astype(np.float32)
