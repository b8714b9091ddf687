#!/usr/bin/env python3
"""Golden fixture for the foresight ceiling of the Ticker env (include/goldsrl_tickerforesight.h), made as
gen_golden_ticker_rules.py makes its own: the UNMODIFIED reference TickerEnv (fed_gym/envs/fed_env.py:89-158) is created without
__init__ under the stand-ins of _ref_stubs.py, with the _Windows stand-in for the sampler.  Build container only:
    python tests/golden/gen_golden_ticker_foresight.py

The reference has no ceiling; what it pins here is the env the foresight actions are played on.  The actions are those of the
plain-loop recurrence of tests/_ticker_foresight_oracle.py on the table of ticker_rules.npz, for the window starts 0 / 123 / 376, 256
steps, horizon 0 (every row of the episode known) and horizon 4.  Each action is handed to the env as the float64 copy of its float32
fraction.  Recorded: the starts, the horizons, per (start, horizon) the actions, the rewards and the assets after every step, and the
bound of horizon 0.  Asserted: nothing depletes, horizon 0 ends above horizon 4, and its total is within 1e-12 of its bound."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import gen_golden_ticker as G  # noqa: E402  (installs _ref_stubs and imports the reference)
import _ticker_foresight_oracle as FO  # noqa: E402

STEPS = 256
HORIZONS = (0, 4)


def play(matrix, start, acts):
    env = G.make_env(matrix, [start])
    env.reset()
    rewards, assets = np.zeros(len(acts)), np.zeros(len(acts))
    for t, a in enumerate(acts):
        assert env.data_idx == t
        _, r, done, _ = env.step([a[:2].astype(np.int64), a[2:].astype(np.float64)])
        assert not done
        rewards[t], assets[t] = r, env.assets
    return rewards, assets


def main():
    rules = np.load(os.path.join(HERE, "ticker_rules.npz"))
    matrix, starts = rules["matrix"], rules["starts"]
    S, Hn = len(starts), len(HORIZONS)
    actions = np.zeros((S, Hn, STEPS, 4), np.float32)
    rewards, assets, bound = np.zeros((S, Hn, STEPS)), np.zeros((S, Hn, STEPS)), np.zeros(S)
    for s, st in enumerate(starts):
        win = matrix[st:st + 1024]
        for k, H in enumerate(HORIZONS):
            actions[s, k] = FO.plan(H, win, 0, STEPS - 1)
            rewards[s, k], assets[s, k] = play(matrix, int(st), actions[s, k])
        A, B0, B1 = FO.coefficients(win, 0, STEPS - 1)[:3]
        bound[s] = np.log(10.0 * A + 1e-4) - np.log(10.0 + 1e-4)
        assert abs(rewards[s, 0].sum() - bound[s]) <= 1e-12, (rewards[s, 0].sum(), bound[s])
    assert np.isfinite(rewards).all() and (assets >= 1.0).all()
    assert (assets[:, 0, -1] > assets[:, 1, -1]).all()
    print("totals (start, horizon)", rewards.sum(axis=2), "bound", bound)
    path = os.path.join(HERE, "ticker_foresight.npz")
    np.savez_compressed(path, starts=starts, horizons=np.array(HORIZONS, np.int32), actions=actions, rewards=rewards, assets=assets,
                        bound=bound)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
