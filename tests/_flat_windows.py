"""The TRUE history window of the flat PAAC policy (include/goldsrl_flatwindow.h) restated in numpy: per env the last
L = min(k + 1, rnn) processed states of the current episode, oldest first, the current state last, zero rows behind; k = steps
since the episode's reset.  A step that ends the episode is followed by the reset observation alone; a window never spans two
episodes.  This is the rule of SolowPolicyMonitor.eval_once (window_rows[-rnn:]) and of _gauss_oracle.replay_windows; unlike the
latter, `replay` carries the rows of an unfinished episode from one rollout into the next.

Scenarios of tests/test_gpu_flat_true_window.py (shapes of _async_scenarios: E = 200, T = 20): name -> env kind, rnn R, TimeLimit
cap, steps per rollout, rollouts in a row."""
import numpy as np

import _async_scenarios as SC

SCENARIOS = {
    "solow": dict(kind="solow", R=5, cap=SC.CAP, T=SC.T, rollouts=2),              # staggered TimeLimit
    "trade3": dict(kind="trade", n=3, R=4, cap=16, T=SC.T, rollouts=2),             # depletion; the window fills and slides
    "trade16": dict(kind="trade", n=16, R=20, cap=16, T=SC.T, rollouts=2),          # the window never fills: zero rows always
    "solow_short": dict(kind="solow", R=5, cap=SC.CAP, T=3, rollouts=4),            # T < R - 1: the carry is a shift
}


def replay(states, dones, rnn, prev_rows=None, prev_len=None):
    """Windows of one rollout.  states (T,E,D): the state each step was entered with, as recorded; dones (T,E): the step ended
    the episode (the NEXT recorded state is then the reset observation).  prev_rows (E,rnn,D) / prev_len (E,): the rows of each
    env's running episode behind the previous rollout, oldest first (what the previous call returned; None or length 0: the
    episode starts with this rollout's first state -- fresh handles, and envs the host reset in between).
    Returns windows (T,E,rnn,D) float32, lengths (T,E) int32, and the (rows, lengths) to hand to the next rollout's call."""
    states = np.asarray(states, np.float32)
    T, E, D = states.shape
    win = np.zeros((T, E, rnn, D), np.float32)
    length = np.zeros((T, E), np.int32)
    next_rows = np.zeros((E, rnn, D), np.float32)
    next_len = np.zeros(E, np.int32)
    for e in range(E):
        n0 = 0 if prev_len is None else int(prev_len[e])
        rows = [] if n0 == 0 else [np.array(r) for r in prev_rows[e][:n0]]
        for t in range(T):
            rows.append(states[t, e])
            del rows[:-rnn]                      # the window slides: k + 1 > rnn
            win[t, e, :len(rows)] = rows
            length[t, e] = len(rows)
            if dones[t, e]:
                rows = []
        keep = rows[-(rnn - 1):] if rnn > 1 else []
        next_len[e] = len(keep)
        if keep:
            next_rows[e, :len(keep)] = keep
    return win, length, (next_rows, next_len)


def replay_chain(states_list, dones_list, rnn, reset_between=()):
    """`replay` over consecutive rollouts; reset_between[i]: env indices the host reset between rollout i and i + 1."""
    out, carry = [], (None, None)
    for i, (s, d) in enumerate(zip(states_list, dones_list)):
        w, l, carry = replay(s, d, rnn, *carry)
        out.append((w, l))
        if i < len(reset_between) and len(reset_between[i]):
            carry[1][np.asarray(reset_between[i])] = 0
    return out


def edges(lengths_list, dones_list, rnn):
    """Which edges a chain of rollouts exercises: the set of window lengths, whether a window slides (a length-rnn window follows a
    length-rnn window of the same episode), whether rows are carried over a rollout boundary (a first-step window longer than 1),
    whether a done falls on the last step of a rollout."""
    seen = set()
    slides = carried = last_done = False
    for i, (l, d) in enumerate(zip(lengths_list, dones_list)):
        d = np.asarray(d).astype(bool)
        seen |= set(np.unique(l).tolist())
        if rnn > 1:
            slides = slides or bool(((l[1:] == rnn) & (l[:-1] == rnn) & ~d[:-1]).any())
        if i > 0:
            carried = carried or bool((l[0] > 1).any())
            if rnn > 1:
                slides = slides or bool(((l[0] == rnn) & (lengths_list[i - 1][-1] == rnn) & ~np.asarray(dones_list[i - 1][-1]).astype(bool)).any())
        last_done = last_done or bool(d[-1].any())
    return dict(lengths=seen, slides=slides, carried=carried, last_done=last_done)


def oracle_dones(name):
    """(rollouts) x (T,E) done masks of the scenario under the oracle envs alone: the staggered TimeLimit for Solow; TimeLimit(cap)
    plus depletion under the fixed tanh(N(0,1)) actions of _async_scenarios for TradeAR1."""
    c = SCENARIOS[name]
    steps = c["T"] * c["rollouts"]
    if c["kind"] == "solow":
        d = SC.timelimit_dones(SC.staggered_elapsed(SC.E, c["cap"]), steps, c["cap"])
    else:
        n = c["n"]
        kw = SC.TRADE_DEPLETION[n]
        acts, nrm = SC.trade_inputs(n, SC.TRADE_INPUT_SEED[n], steps=steps)
        d = SC.trade_oracle(n, kw["trade_starting_balance"], kw["trade_std_p"], acts, nrm, cap=c["cap"])["done"]
    return [d[i * c["T"]:(i + 1) * c["T"]] for i in range(c["rollouts"])]
