#!/usr/bin/env python3
"""Golden fixture for the foresight ceiling of the TradeAR1 env (include/goldsrl_tradeforesight.h), made as gen_golden_trade_rules.py
makes its own: the UNMODIFIED reference TradeAR1Env (fed_gym/envs/fed_env.py:268-334) under the stand-ins of _ref_stubs.py, with
np.random.normal replaced by the recorded normals of trade_rules.npz (n2_ / n3_ / n16_normals, float32 values handed to the env as
float64).  Build container only:
    python tests/golden/gen_golden_trade_foresight.py

The reference has no ceiling; what it pins here is the env the foresight actions are played on.  For n_assets in (2, 3, 16) the env
is first played 256 steps holding cash to record its own price path (row t: the prices step t trades at), then once per horizon of
(1, 2, 4, 16, 64, 0) under the actions of the plain-loop recurrence of tests/_trade_foresight_oracle.py on that path.  Each action is
handed to the env as the float64 copy of its float32 value.  Recorded per n: the path, and per horizon the actions, the rewards, the
assets after every step and the total; the bound of horizon 0; and the totals when 1 / 2 / 4 / 16 rows are known (the same columns).
Asserted: nothing depletes, the env's path under the actions is the recorded one, and the horizon-0 total equals the bound within
length * 2**-24 * max(|min|, |max|) + 1e-10, the allowance of the device test (whose rewards are float32)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _ref_stubs  # noqa: E402

_ref_stubs.install()
from fed_gym.envs import fed_env  # noqa: E402
import _trade_foresight_oracle as FO  # noqa: E402

STEPS = 256


def play(n, normals, acts):
    """One episode of TradeAR1Env(n_assets=n) under the action rows `acts` over the recorded normals.  Returns the prices every
    step traded at, the rewards and the assets after each step."""
    env = fed_env.TradeAR1Env(n_assets=n)
    env.reset()
    path, rewards, assets = np.zeros((len(acts), n)), np.zeros(len(acts)), np.zeros(len(acts))
    it = iter(normals.astype(np.float64))
    orig = np.random.normal
    np.random.normal = lambda size=None: next(it)
    try:
        for t, a in enumerate(acts):
            path[t] = env.prices
            _, r, done, _ = env.step(np.asarray(a, np.float32).astype(np.float64))
            assert not done, (n, t)
            rewards[t], assets[t] = r, env.assets
    finally:
        np.random.normal = orig
    return path, rewards, assets


def main():
    rules = np.load(os.path.join(HERE, "trade_rules.npz"))
    out = {"horizons": np.array(FO.HORIZONS, np.int32)}
    for n in (2, 3, 16):
        pre = "n%d_" % n
        normals = rules[pre + "normals"]
        assert normals.shape == (STEPS, n) and normals.dtype == np.float32
        path = play(n, normals, np.zeros((STEPS, n), np.float32))[0]
        Hn = len(FO.HORIZONS)
        actions = np.zeros((Hn, STEPS, n), np.float32)
        rewards, assets = np.zeros((Hn, STEPS)), np.zeros((Hn, STEPS))
        for k, H in enumerate(FO.HORIZONS):
            actions[k] = FO.plan(H, path, STEPS - 1)
            played, rewards[k], assets[k] = play(n, normals, actions[k])
            assert np.array_equal(played, path)
        total = rewards.sum(axis=1)
        bound = FO.bound(path, STEPS - 1, 10.0, np.zeros(n), 10.0)
        whole = FO.HORIZONS.index(0)
        allowance = STEPS * 2.0 ** -24 * np.abs(rewards[whole]).max() + 1e-10
        assert abs(total[whole] - bound) <= allowance, (n, total[whole], bound, allowance)
        assert (total <= bound + allowance).all() and (rules[pre + "total"] <= bound + allowance).all()
        assert np.isfinite(rewards).all() and (assets >= 1.0).all()
        out[pre + "path"], out[pre + "actions"], out[pre + "rewards"], out[pre + "assets"] = path, actions, rewards, assets
        out[pre + "total"], out[pre + "bound"] = total, np.array(bound)
        print("n = %d: whole-episode total %.10f, bound %.10f (difference %.3g, allowance %.3g); by rows known %s; best rule %.4f"
              % (n, total[whole], bound, total[whole] - bound, allowance,
                 " / ".join("%d: %.4f" % (H, total[k]) for k, H in enumerate(FO.HORIZONS) if H), rules[pre + "total"].max()))
    path = os.path.join(HERE, "trade_foresight.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
