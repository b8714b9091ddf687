"""The recurrence and the play of include/goldsrl_solowforesight.h in plain numpy float64, one IEEE operation per line of the header:
the yardstick of grl_solow_foresight.  ez: the path (L,), the float32 values exp(z_t) as float64.  grid: the dict of
goldsrl._ffi_solowforesight.solow_foresight_grid, of which only the sizes and ranges are read."""
import numpy as np


def axes(grid):
    """(log k_lo, the step in log k, the rates s_a)"""
    lk_lo = np.log(grid["k_lo"])
    dlk = (np.log(grid["k_hi"]) - lk_lo) / float(grid["nk"] - 1)
    ds = (grid["s_hi"] - grid["s_lo"]) / float(grid["ns"] - 1)
    return lk_lo, dlk, grid["s_lo"] + np.arange(grid["ns"], dtype=np.float64) * ds


def coord(x, lk_lo, dlk, nk):
    u = np.clip((x - lk_lo) / dlk, 0.0, float(nk - 1))
    i = np.minimum(u.astype(np.int64), nk - 2)
    return i, u - i


def solve(ez, grid, delta):
    """decisions (L, nk) uint8, V_0 (nk,), and the smallest gap between the best and the second-best Q of any (stage, node)"""
    nk = grid["nk"]
    lk_lo, dlk, rates = axes(grid)
    k = np.exp(lk_lo + np.arange(nk, dtype=np.float64) * dlk)
    kp, kd = np.power(k, 0.33), (1.0 - delta) * k
    s = np.maximum(1e-3, rates)[None, :]
    V, dec, gap = np.zeros(nk), np.zeros((len(ez), nk), np.uint8), np.inf
    for t in range(len(ez) - 1, -1, -1):
        y = (float(ez[t]) * kp)[:, None]
        r = np.log((1.0 - s) * y + 1e-4)
        i, f = coord(np.log(kd[:, None] + s * y), lk_lo, dlk, nk)
        Q = r + ((1.0 - f) * V[i] + f * V[i + 1])
        a = Q.argmax(axis=1)                                   # the first of equals: the lowest index
        two = np.sort(Q, axis=1)[:, -2:]
        gap = min(gap, float((two[:, 1] - two[:, 0]).min()))
        V, dec[t] = Q[np.arange(nk), a], a
    return dec, V, gap


def value_at(V, k0, grid):
    """V interpolated at k0"""
    lk_lo, dlk, _ = axes(grid)
    i, f = coord(np.log(np.float64(k0)), lk_lo, dlk, grid["nk"])
    return float((1.0 - f) * V[i] + f * V[i + 1])


def play(dec, ez, k0, grid, delta):
    """The plan played from k0 in float64: (total, the capital before every step and after the last)"""
    lk_lo, dlk, rates = axes(grid)
    k, total, ks = float(k0), 0.0, [float(k0)]
    for t in range(len(ez)):
        i, f = coord(np.log(k), lk_lo, dlk, grid["nk"])
        s = max(1e-3, float((1.0 - f) * rates[dec[t, i]] + f * rates[dec[t, i + 1]]))
        y = float(ez[t]) * k ** 0.33
        total += float(np.log((1.0 - s) * y + 1e-4))
        k = (1.0 - delta) * k + s * y
        ks.append(k)
    return total, np.array(ks)
