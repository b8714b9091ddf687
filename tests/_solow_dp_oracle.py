"""The finite-horizon savings problem of the Solow env by backward induction, in numpy float64: the yardstick of
grl_solow_dp_solve (include/goldsrl_solowdp.h).  Written from the recurrence, one IEEE operation per operation of the formulas, so
that a faithful float64 implementation differs only through exp / log / pow:

    y = exp(z) * k^0.33;  r = log((1 - s) * y + 1e-4);  k' = (1 - delta) * k + s * y;  z' = (rho * z + theta * e) + eps;  e' = eps
    Q(k, z, e; s) = r + sum_j w_j * bilinear(V_next[:, :, j]; log k', (rho * z + theta * e) + e_nodes[j])

k is uniform in log k, z uniform, e the quadrature nodes, s uniform; coordinates are clamped to the grid, np.argmax keeps the
lowest index on a tie, the last stage has V_next = 0.  grid: the dict of goldsrl._ffi_solowdp.solow_dp_grid (sizes, ranges, e_nodes,
e_weights); ne: the size of the e-dimension (nq, or 1 for a model without the moving-average term)."""
import numpy as np

ALPHA = 0.33


def axes(grid, ne):
    nk, nz, ns = grid["nk"], grid["nz"], grid["ns"]
    lk_lo = np.log(grid["k_lo"])
    dlk = (np.log(grid["k_hi"]) - lk_lo) / float(nk - 1)
    dz = (grid["z_max"] + grid["z_max"]) / float(nz - 1)
    ds = (grid["s_hi"] - grid["s_lo"]) / float(ns - 1)
    return {"lk_lo": lk_lo, "dlk": dlk, "dz": dz, "ds": ds,
            "k": np.exp(lk_lo + np.arange(nk) * dlk), "z": -grid["z_max"] + np.arange(nz) * dz,
            "e": np.asarray(grid["e_nodes"], np.float64)[:ne], "s": grid["s_lo"] + np.arange(ns) * ds}


def coord(x, lo, step, n):
    u = np.clip((x - lo) / step, 0.0, float(n - 1))
    i = np.minimum(u.astype(np.int64), n - 2)
    return i, u - i


def bilinear(plane, ik, fk, iz, fz):
    v0 = (1.0 - fk) * plane[ik, iz] + fk * plane[ik + 1, iz]
    v1 = (1.0 - fk) * plane[ik, iz + 1] + fk * plane[ik + 1, iz + 1]
    return (1.0 - fz) * v0 + fz * v1


def solve(grid, horizon, rho, theta, delta, ne):
    """Returns policy (horizon, nk, nz, ne) float32, value (nk, nz, ne) float64 of stage 0, and min_gap: the smallest difference
    between the best and the second-best Q over all states and stages."""
    ax = axes(grid, ne)
    nk, nz, nq, ns = grid["nk"], grid["nz"], grid["nq"], grid["ns"]
    nodes, w = np.asarray(grid["e_nodes"], np.float64), np.asarray(grid["e_weights"], np.float64)
    k, z, s = ax["k"][:, None, None], ax["z"][None, :, None], ax["s"][None, None, :]
    y = np.exp(z) * np.power(k, ALPHA)                                   # (nk, nz, 1)
    r = np.log((1.0 - s) * y + 1e-4)                                     # (nk, nz, ns)
    ik, fk = coord(np.log((1.0 - delta) * k + s * y), ax["lk_lo"], ax["dlk"], nk)
    ik, fk = ik[:, :, None, :], fk[:, :, None, :]                        # (nk, nz, 1, ns)
    zc = rho * ax["z"][:, None] + theta * ax["e"][None, :]               # (nz, ne)
    cz = [coord(zc + nodes[j], -grid["z_max"], ax["dz"], nz) for j in range(nq)]
    policy = np.zeros((horizon, nk, nz, ne), np.float32)
    v_next, min_gap = None, np.inf
    for t in range(horizon - 1, -1, -1):
        acc = np.zeros((nk, nz, ne, ns))
        if v_next is not None:
            for j in range(nq):
                iz, fz = cz[j]
                acc = acc + w[j] * bilinear(v_next[:, :, j if ne > 1 else 0], ik, fk, iz[None, :, :, None], fz[None, :, :, None])
        q = r[:, :, None, :] + acc
        best = q.argmax(axis=3)
        top = np.partition(q, ns - 2, axis=3)[..., ns - 2:]
        min_gap = min(min_gap, float((top[..., 1] - top[..., 0]).min()))
        policy[t] = (grid["s_lo"] + best * ax["ds"]).astype(np.float32)
        v_next = q.max(axis=3)
    return policy, v_next, min_gap


def episode(z0, es, steps, delta, rho, theta, action):
    """SolowEnv for p = 1 in float64 from the reset state (k = k_ss(0.33), e = 0, z = z0), es popped from the end;
    action(t, k, z, e) gives the step's savings rate.  Returns the step rewards."""
    k, z, e = (ALPHA / delta) ** (1.0 / (1.0 - ALPHA)), float(z0), 0.0
    es, rewards = list(es), np.zeros(steps)
    for t in range(steps):
        s = max(1e-3, float(action(t, k, z, e)))
        y = np.exp(z) * k ** ALPHA
        rewards[t] = np.log((1.0 - s) * y + 1e-4)
        k = (1.0 - delta) * k + s * y
        e_t = es.pop()
        z, e = (rho * z + theta * e) + e_t, e_t
    return rewards
