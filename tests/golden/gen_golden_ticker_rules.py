#!/usr/bin/env python3
"""Golden fixture for the scripted rule baseline of the Ticker env (goldsrl/baselines.py:TickerRuleBaseline), made as
gen_golden_ticker.py makes its own: the UNMODIFIED reference TickerEnv (fed_gym/envs/fed_env.py:89-158) is created without __init__
under the stand-ins of _ref_stubs.py, with the _Windows stand-in for the sampler.  Build container only:
    python tests/golden/gen_golden_ticker_rules.py

The reference has no scripted baseline; what it pins here is the env the rules are played on.  The rule (include/goldsrl_tickersweep.h)
is written out below in numpy float64, one operation per line, on what the env shows before the step: cash_balance, quantities, the
prices of the row the trade executes at and the price `lookback` rows before.  Each action is handed to the env as the float64 copy
of its float32 fraction: the device account takes float32 actions.

The table is a synthetic one of gen_golden_ticker.py's kind (700 days, 1 400 rows through the reference's open_close_to_sequence)
with a daily log drift of 6e-4.  Recorded for the window starts 0 / 123 / 376 and the 12 default rules: the table, the starts, the
rules; per rule the actions, the rewards and the assets after every step over 256 steps, the length and the total; the same for
buy-and-hold and the 0.05-band mix over the full 1 023 steps; and the L = 2 trend rule until it is depleted.  Asserted: holding cash
totals exactly 0, buy-and-hold trades exactly once, the depletion case ends before the window does, and the best and second-best
mean totals are further apart than twice the device test's bound (256 steps x 2e-7)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden_ticker as G  # noqa: E402  (installs _ref_stubs and imports the reference)

STEPS, FULL = 256, 1023
STARTS = (0, 123, 376)
RULES = np.array([(0, 0, 0, 0, 1, 0), (1, 0, 1, 0, 0.5, 0), (0, 1, 0, 1, 0.5, 0)]
                 + [(0.5, 0.5, 0.5, 0.5, b, 0) for b in (0.25, 0.05, 0.01)]
                 + [(1, 0, 0, 1, 0.5, L) for L in (2, 8, 32, 128)]
                 + [(1, 0, 0, 0, 0.5, L) for L in (8, 32)], np.float32)
FULL_RULES = (1, 4)       # buy and hold, the 0.05-band mix
DEP_RULE = 6              # the L = 2 switch


def drifting_table(days, seed, drift):
    rng = np.random.RandomState(seed)
    opens, closes = [], []
    p = 100.0
    for _ in range(days):
        o = p * np.exp(rng.normal(0.5 * drift, 0.004))
        c = o * np.exp(rng.normal(0.5 * drift, 0.006))
        opens.append(o); closes.append(c)
        p = c
    vol = rng.uniform(1e5, 5e5, size=days).round()
    return np.array(opens), np.array(closes), vol


def rule_action(rule, cash, q, p, back):
    """(choices (2,) int64, fractions (2,) float32) of `rule` (float64 copies of the float32 parameters)"""
    up0, up1, dn0, dn1, band, lb = (np.float64(v) for v in rule)
    L = int(lb)
    up = L == 0 or p[0] >= back
    t = (up0, up1) if up else (dn0, dn1)
    v0 = q[0] * p[0]
    v1 = q[1] * p[1]
    hold = v0 + v1
    total = cash + hold
    disc, frac = np.zeros(2, np.int64), np.zeros(2, np.float32)
    for a, v in enumerate((v0, v1)):
        s = v / total
        lo = t[a] - band
        hi = t[a] + band
        if s < lo:
            d = t[a] - s
            w = d * total
            c = max(cash, 1e-12)
            f = w / c
            f = min(f, 1.0)
            disc[a] = 1
        elif s > hi:
            d = s - t[a]
            f = d / s
            f = min(f, 1.0)
            disc[a] = 2
        else:
            f = 0.0
        frac[a] = np.float32(f)
    return disc, frac


def play(matrix, start, rule, steps):
    """One episode of the reference env under `rule`, `steps` steps or until done.  Returns actions (steps,4) float32, rewards and
    assets after each step (steps,) float64, zero past the length, and the length."""
    env = G.make_env(matrix, [start])
    env.reset()
    L = int(rule[5])
    actions, rewards, assets = np.zeros((steps, 4), np.float32), np.zeros(steps), np.zeros(steps)
    length = 0
    for t in range(steps):
        i = env.data_idx
        back = env.price_vol_data[max(i - L, 0), 0]
        disc, frac = rule_action(rule, env.cash_balance, env.quantities, env.prices, back)
        assert (frac >= 0).all() and (frac <= 1).all()
        actions[t, :2], actions[t, 2:] = disc, frac
        _, r, done, _ = env.step([disc, frac.astype(np.float64)])       # _step rescales the buy fractions it is handed in place
        rewards[t], assets[t] = r, env.assets
        length = t + 1
        if done:
            break
    assert np.isfinite(rewards).all() and np.isfinite(assets).all()
    return actions, rewards, assets, length


def play_all(matrix, rules, steps):
    S, R = len(STARTS), len(rules)
    out = (np.zeros((S, R, steps, 4), np.float32), np.zeros((S, R, steps)), np.zeros((S, R, steps)), np.zeros((S, R), np.int32))
    for s, st in enumerate(STARTS):
        for r, rule in enumerate(rules):
            out[0][s, r], out[1][s, r], out[2][s, r], out[3][s, r] = play(matrix, st, rule, steps)
    return out


def main():
    s = object.__new__(G.ref_sampler.OpenCloseSampler)
    opens, closes, vol = drifting_table(700, 2, 6e-4)      # a seed whose table passes the sampler's exact-zero self-check (sampler.py:36)
    frame = {"Open": G._col(opens), "Close": G._col(closes), "Volume": G._col(vol)}
    matrix = s.open_close_to_sequence(frame, inverse_asset=True)
    assert matrix.shape == (1400, 4) and max(STARTS) + 1024 <= len(matrix)
    out = {"tbl_open": opens, "tbl_close": closes, "tbl_volume": vol, "matrix": matrix, "starts": np.array(STARTS, np.int32), "rules": RULES}
    # ---- the 12 default rules over 256 steps
    actions, rewards, assets, length = play_all(matrix, RULES, STEPS)
    assert (length == STEPS).all(), length
    total = rewards.sum(axis=2)
    assert (rewards[:, 0] == 0.0).all() and (assets[:, 0] == 10.0).all() and (actions[:, 0] == 0).all()          # hold cash
    mean = total.mean(axis=0)
    order = np.argsort(-mean, kind="stable")
    assert mean[order[0]] - mean[order[1]] > 2 * STEPS * 2e-7, mean
    out["actions"], out["rewards"], out["assets"], out["length"], out["total"] = actions, rewards, assets, length, total
    out["best_index"] = np.array(int(order[0]))
    print("mean totals over 256 steps", mean, "best", int(order[0]))
    # ---- two rules over the whole window
    fa, fr, fas, fl = play_all(matrix, RULES[list(FULL_RULES)], FULL)
    assert (fl == FULL).all(), fl
    assert (((fa[:, 0, :, :2] != 0).any(axis=2)).sum(axis=1) == 1).all()                                         # buy and hold trades once
    out["full_rules"], out["full_actions"], out["full_rewards"], out["full_assets"] = np.array(FULL_RULES, np.int32), fa, fr, fas
    out["full_length"], out["full_total"] = fl, fr.sum(axis=2)
    print("totals over 1023 steps", out["full_total"])
    # ---- the L = 2 switch until the spread has eaten the account
    da, dr, das, dl = play_all(matrix, RULES[[DEP_RULE]], FULL)
    assert (dl[:, 0] < FULL).all(), dl
    n = int(dl.max())
    for i, st in enumerate(STARTS):
        assert das[i, 0, dl[i, 0] - 1] < 1.0 and (das[i, 0, :dl[i, 0] - 1] >= 1.0).all()
    out["dep_rule"], out["dep_actions"], out["dep_rewards"], out["dep_assets"] = np.array(DEP_RULE, np.int32), da[:, 0, :n], dr[:, 0, :n], das[:, 0, :n]
    out["dep_length"], out["dep_total"] = dl[:, 0], dr[:, 0].sum(axis=1)
    out["dep_trades"] = (da[:, 0, :, :2] != 0).any(axis=2).sum(axis=1).astype(np.int32)
    print("depletion lengths", dl[:, 0], "trades", out["dep_trades"])
    path = os.path.join(HERE, "ticker_rules.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
