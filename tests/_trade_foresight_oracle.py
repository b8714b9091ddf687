"""TEST INFRASTRUCTURE: the foresight recurrence of include/goldsrl_tradeforesight.h as a plain Python loop on scalars, independent of
goldsrl/_ffi_tradeforesight.py, played through the float64 restatement of the env (oracle/oracle.py:trade_step), and the brute force
it is held against.  Shared by tests/test_trade_foresight_oracle.py, tests/test_gpu_trade_foresight.py and
tests/golden/gen_golden_trade_foresight.py."""
import itertools

import numpy as np

HORIZONS = (1, 2, 4, 16, 64, 0)
BRUTE_MOVES = (-1.0, -0.5, 0.0, 0.5, 1.0)


def walk(path, t, e):
    """The recurrence over the known rows t..e of one env's path (rows of n prices), last row first, one float64 operation per
    statement: yields (j, A, B, dec) after row j, dec being row j's decisions per asset: 0 hold, 1 buy, 2 sell."""
    n = len(path[e])
    A = 1.0
    B = [float(v) for v in path[e]]
    for j in range(e, t - 1, -1):
        p = [float(v) for v in path[j]]
        x, y = [0.0] * n, [0.0] * n
        for a in range(n):
            x[a] = B[a] / p[a]
            y[a] = p[a] * A
        g = 0.0
        dec = [0] * n
        for a in range(n):
            if x[a] > A:
                d = x[a] - A
                g = g + d
                dec[a] = 1
        for a in range(n):
            if y[a] > B[a]:
                B[a] = y[a]
                assert dec[a] == 0, "buy and sell of one asset in one row"
                dec[a] = 2
        s = g / float(n)
        A = A + s
        yield j, A, list(B), dec


def coefficients(path, t, e):
    """(A, B, dec) of the known rows t..e: the coefficients before the trade of row t and that row's decisions."""
    out = None
    for out in walk(path, t, e):
        pass
    return out[1:]


def _acts(dec):
    return [1.0 if c == 1 else (-1.0 if c == 2 else 0.0) for c in dec]


def action(horizon, path, t, last):
    """The action row, float32 (n,), of step t of a pair whose last step is `last`."""
    e = last if horizon == 0 else min(t + horizon, last)
    return np.array(_acts(coefficients(path, t, e)[2]), np.float32)


def plan(horizon, path, last):
    """The action rows of steps 0..last, (last + 1, n) float32.  Horizon 0 is one backward pass: every step's known rows end at
    `last`, so the walk from there passes through every step's coefficients."""
    out = np.zeros((last + 1, len(path[0])), np.float32)
    if horizon == 0:
        for j, _, _, dec in walk(path, 0, last):
            out[j] = _acts(dec)
    else:
        for t in range(last + 1):
            out[t] = action(horizon, path, t, last)
    return out


def bound(path, last, cash, qty, assets):
    """log((cash * A + sum_a q_a * B_a, summed in asset order) + 1e-4) - log(assets + 1e-4) with the whole-episode coefficients."""
    A, B, _ = coefficients(path, 0, last)
    v = cash * A
    for a in range(len(B)):
        w = float(qty[a]) * B[a]
        v = v + w
    return float(np.log(v + 1e-4) - np.log(assets + 1e-4))


def price_path(normals, std_e, p0=None):
    """rows 0..len(normals) of the path from p0 (ones by default): row t + 1 = row t ** 0.9 * exp(std_e * normals[t]), float64"""
    normals = np.asarray(normals, np.float64)
    rows = np.zeros((len(normals) + 1, normals.shape[1]))
    rows[0] = 1.0 if p0 is None else p0
    for t in range(len(normals)):
        rows[t + 1] = (rows[t] ** 0.9) * np.exp(std_e * normals[t])
    return rows


def play(path, acts, cash=10.0):
    """A batch of action sequences acts (N, steps, n) through oracle/oracle.py:trade_step on one price path, every account starting
    with `cash` and no holdings.  Returns rewards (N, steps) and the assets after every step (N, steps), float64."""
    from oracle import oracle as O
    acts = np.asarray(acts, np.float64)
    N, steps, n = acts.shape
    c, assets, q = np.full(N, float(cash)), np.full(N, float(cash)), np.zeros((N, n))
    rewards, after = np.zeros((N, steps)), np.zeros((N, steps))
    for t in range(steps):
        prices = np.broadcast_to(np.asarray(path[t], np.float64), (N, n))
        c, assets, q, _, _, r, _ = O.trade_step(c, assets, q, prices, acts[:, t], np.zeros((N, n)), 0.0)
        rewards[:, t], after[:, t] = r, assets
    return rewards, after


def brute_force(path, steps=4):
    """The largest final assets over all (5 ** n) ** steps sequences of BRUTE_MOVES per asset on the first `steps` rows, and the
    sequence that reaches it, (steps, n)."""
    n = len(path[0])
    per_step = np.array(list(itertools.product(BRUTE_MOVES, repeat=n)))                # (5 ** n, n)
    seqs = np.array(list(itertools.product(range(len(per_step)), repeat=steps)))        # (N, steps)
    _, after = play(path, per_step[seqs])
    best = int(np.argmax(after[:, -1]))
    return float(after[best, -1]), per_step[seqs[best]]
