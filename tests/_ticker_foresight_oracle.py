"""TEST INFRASTRUCTURE: the foresight recurrence of include/goldsrl_tickerforesight.h as a plain Python loop on scalars, played through
the float64 restatement of the env (oracle/ticker.py), and the brute force it is held against.  Shared by
tests/test_ticker_foresight_oracle.py, tests/test_gpu_ticker_foresight.py and tests/golden/gen_golden_ticker_foresight.py."""
import itertools

import numpy as np

from oracle import ticker as TK

UP, DN = 1.0 + TK.SPREAD, 1.0 - TK.SPREAD


def walk(win, t, e):
    """The recurrence over the known rows t..e of the window `win` (rows of (p0, p1, ...)), last row first, one float64 operation
    per statement: yields (j, A, B0, B1, choice0, choice1) after row j, the choices being those of row j."""
    A, B0, B1 = 1.0, float(win[e][0]), float(win[e][1])
    for j in range(e, t - 1, -1):
        p0, p1 = float(win[j][0]), float(win[j][1])
        a0 = p0 * UP
        a1 = p1 * UP
        x0 = B0 / a0
        x1 = B1 / a1
        b0 = p0 * DN
        b1 = p1 * DN
        y0 = b0 * A
        y1 = b1 * A
        An, buy = A, -1
        if x0 > An:
            An, buy = x0, 0
        if x1 > An:
            An, buy = x1, 1
        c0, c1 = (1 if buy == 0 else 0), (1 if buy == 1 else 0)
        if y0 > B0:
            B0 = y0
            c0 = c0 or 2
        if y1 > B1:
            B1 = y1
            c1 = c1 or 2
        A = An
        yield j, A, B0, B1, c0, c1


def coefficients(win, t, e):
    """(A, B0, B1, choice0, choice1) of the known rows t..e: the coefficients before the trade of row t and that row's choices."""
    out = None
    for out in walk(win, t, e):
        pass
    return out[1:]


def _row(c0, c1):
    return [c0, c1, 1.0 if c0 else 0.0, 1.0 if c1 else 0.0]


def action(horizon, win, t, last):
    """The action row (choice0, choice1, fraction0, fraction1), float32 (4,), of the step at row t of a pair whose last step is at row
    `last`."""
    e = last if horizon == 0 else min(t + horizon, last)
    return np.array(_row(*coefficients(win, t, e)[3:]), np.float32)


def plan(horizon, win, idx, last):
    """The action rows of the steps at rows idx..last, (last - idx + 1, 4) float32.  Horizon 0 is one backward pass: every step's
    known rows end at `last`, so the walk from there passes through every step's coefficients."""
    out = np.zeros((max(last - idx + 1, 0), 4), np.float32)
    if horizon == 0:
        for j, _, _, _, c0, c1 in walk(win, idx, last):
            out[j - idx] = _row(c0, c1)
    else:
        for t in range(idx, last + 1):
            out[t - idx] = action(horizon, win, t, last)
    return out


def play(matrix, start, horizon, steps, state=None):
    """One env of oracle/ticker.py under `horizon` for `steps` steps (no TimeLimit; the caller keeps idx + steps <= 1023) from a
    reset at `start`, or from `state` (a one-env state dict of oracle/ticker.py, left untouched).  Returns actions (steps, 4)
    float32, rewards and assets after each step (steps,) float64, and the bound of the start:
    log(cash A + q0 B0 + q1 B1 + 1e-4) - log(assets + 1e-4) with the whole-episode coefficients."""
    if state is None:
        st, _ = TK.ticker_reset(matrix, [start])
    else:
        st = {k: np.array(v) for k, v in state.items()}
        start = int(st["start"][0])
    win = matrix[start:start + TK.WINDOW]
    idx = int(st["idx"][0])
    last = idx + steps - 1
    assert last <= TK.WINDOW - 2
    A, B0, B1 = coefficients(win, idx, last)[:3]
    vc = st["cash"][0] * A
    v0 = st["qty"][0, 0] * B0
    v1 = st["qty"][0, 1] * B1
    vs = vc + v0
    v = vs + v1
    bound = np.log(v + 1e-4) - np.log(st["assets"][0] + 1e-4)
    acts = plan(horizon, win, idx, last)
    rewards, assets = np.zeros(steps), np.zeros(steps)
    for t in range(steps):
        _, r, _ = TK.ticker_step(matrix, st, acts[t:t + 1, :2].astype(np.int64), acts[t:t + 1, 2:].astype(np.float64))
        rewards[t], assets[t] = r[0], st["assets"][0]
    return acts, rewards, assets, float(bound)


BRUTE_MOVES = ((0, 0.0), (1, 0.5), (1, 1.0), (2, 1.0))       # hold, buy 1/2, buy all, sell all


def brute_force(matrix, steps=4):
    """The largest final assets over all 16 ** steps sequences of BRUTE_MOVES x BRUTE_MOVES from a reset at row 0, the sequences
    as the batch of oracle/ticker.py.  matrix needs steps + 1 rows (the env shows the row after the last step)."""
    per_step = list(itertools.product(range(4), repeat=2))
    seqs = np.array(list(itertools.product(range(16), repeat=steps)), np.int64)        # (16 ** steps, steps)
    st, _ = TK.ticker_reset(matrix, np.zeros(len(seqs), np.int64))
    moves = np.array(BRUTE_MOVES)
    for t in range(steps):
        pair = np.array(per_step)[seqs[:, t]]                                           # (N, 2) move indices
        disc = moves[pair, 0].astype(np.int64)
        cont = moves[pair, 1].astype(np.float64)
        TK.ticker_step(matrix, st, disc, cont)
    best = int(np.argmax(st["assets"]))
    return float(st["assets"][best]), [per_step[k] for k in seqs[best]]
