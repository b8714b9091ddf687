#!/usr/bin/env python3
"""Golden fixture for the scripted trading-rule baseline of TradeAR1 (goldsrl/baselines.py:TradingRuleBaseline), made by playing the
UNMODIFIED reference TradeAR1Env (fed_gym/envs/fed_env.py:268-334) under the stand-ins of _ref_stubs.py.  Build container only:
    python tests/golden/gen_golden_trade_rules.py

The reference has no scripted baseline; what it pins here is the env the rules are played on.  For n_assets in (2, 3, 16) the env
is played 256 steps under each of the nine default rules, with np.random.normal replaced by a recorded sequence (as gen_golden.py
does for trade.npz) so every rule sees the same price path.  The recorded normals are float32 values (the device tape's format)
handed to the env as float64.  The action is the rule on the env's current prices, clip(bias - gain * (p - 1), -1, 1) in float64,
rounded to float32 and handed to the env as the float64 copy of that float32: the env's arithmetic follows its action's dtype, and
the device account is the float64 one that trade.npz pins.  Recorded: the normals, per rule the step rewards, the assets after every
step and the total, and the best rule; the best and the second-best total must be further apart than the device test's bound.

A depletion case: n_assets in (2, 3), normals -|N| * 60 from seed 3, rules (0,1), (0,0.5), (5,0), (0,0), 16 steps at most: the first
three end with assets below 1, hold-cash never ends."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_stubs  # noqa: E402

_ref_stubs.install()
from fed_gym.envs import fed_env  # noqa: E402

STEPS, DEP_STEPS = 256, 16
RULES = np.array([(0, 0), (1, 0), (2, 0), (5, 0), (10, 0), (20, 0), (50, 0), (100, 0), (0, 1)], np.float32)
DEP_RULES = np.array([(0, 1), (0, 0.5), (5, 0), (0, 0)], np.float32)


def play(n, rule, normals):
    """One episode of TradeAR1Env(n_assets=n) under `rule` over the recorded normals, until done or the normals run out.
    Returns rewards, assets after each step (zero past the length) and the length."""
    env = fed_env.TradeAR1Env(n_assets=n)
    env.reset()
    g, b = np.float64(rule[0]), np.float64(rule[1])
    rewards, assets = np.zeros(len(normals)), np.zeros(len(normals))
    it = iter(normals.astype(np.float64))
    orig = np.random.normal
    np.random.normal = lambda size=None: next(it)
    length = 0
    try:
        for t in range(len(normals)):
            action = np.clip(b - g * (env.prices - 1.0), -1.0, 1.0).astype(np.float32)
            _, r, done, _ = env.step(action.astype(np.float64))
            rewards[t], assets[t] = r, env.assets
            length = t + 1
            if done:
                break
    finally:
        np.random.normal = orig
    return rewards, assets, length


def main():
    out = {"rules": RULES, "dep_rules": DEP_RULES}
    for n in (2, 3, 16):
        normals = np.random.RandomState(100 + n).normal(size=(STEPS, n)).astype(np.float32)
        rewards, assets = np.zeros((len(RULES), STEPS)), np.zeros((len(RULES), STEPS))
        for i, rule in enumerate(RULES):
            rewards[i], assets[i], length = play(n, rule, normals)
            assert length == STEPS, (n, i, length)
        total = rewards.sum(axis=1)
        order = np.argsort(-total, kind="stable")
        bound = 1e-5 * max(1.0, abs(total[order[0]])) + STEPS * 1e-9
        assert total[order[0]] - total[order[1]] > 2 * bound, (n, total)
        assert (rewards[0] == 0.0).all() and (assets[0] == 10.0).all()          # hold cash
        pre = "n%d_" % n
        out[pre + "normals"], out[pre + "rewards"], out[pre + "assets"] = normals, rewards, assets
        out[pre + "total"], out[pre + "best_index"] = total, np.array(int(order[0]))
        print(n, "totals", total, "best", int(order[0]))
    for n in (2, 3):
        normals = (-np.abs(np.random.RandomState(3).normal(size=(DEP_STEPS, n))) * 60.0).astype(np.float32)
        rewards, assets = np.zeros((len(DEP_RULES), DEP_STEPS)), np.zeros((len(DEP_RULES), DEP_STEPS))
        length = np.zeros(len(DEP_RULES), np.int32)
        for i, rule in enumerate(DEP_RULES):
            rewards[i], assets[i], length[i] = play(n, rule, normals)
        assert (length[:3] < DEP_STEPS).all() and length[3] == DEP_STEPS, length
        assert all(assets[i, length[i] - 1] < 1.0 for i in range(3)) and (rewards[3] == 0.0).all()
        pre = "dep_n%d_" % n
        out[pre + "normals"], out[pre + "rewards"], out[pre + "assets"], out[pre + "length"] = normals, rewards, assets, length
        print(n, "depletion lengths", length)
    path = os.path.join(HERE, "trade_rules.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
