#!/usr/bin/env python3
"""Golden vectors of the Ticker gated trader's acting and window rules, captured from the UNMODIFIED reference
(read-only) under the gym/tensorflow stand-ins of _ref_stubs.py:

  * GaussianWorker.get_random_discrete_action         (fed_gym/agents/a3c/worker.py:223-227)
  * TickerGatedTraderWorker.get_random_action         (worker.py:460-464)
  * TickerGatedTraderWorker.transform_raw_action      (worker.py:491-494)
  * TickerTraderStateProcessor.process_temporal_states (fed_gym/agents/state_processors.py:65-66)

The uniforms and normals the reference draws from numpy's global generator are handed in (np.random.rand / normal answer the
recorded arrays for the duration of one call), so the rule is captured independently of the generator.  Some uniforms are
placed at or above the last float32 cumsum value (the all-False row: argmax gives 0).

Run in the build container only:   python tests/golden/gen_golden_gated.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _ref_stubs  # noqa: E402

_ref_stubs.install()

from fed_gym.agents.state_processors import TickerTraderStateProcessor  # noqa: E402
from fed_gym.agents.a3c import worker as a3c_worker  # noqa: E402


def main():
    rng = np.random.RandomState(20261016)
    K = 64
    logits = rng.normal(size=(K, 3)) * 2.0
    probs = (np.exp(logits) / np.exp(logits).sum(1, keepdims=True)).astype(np.float32)
    probs[0] = np.float32(1.0 / 3.0)                       # cumsum ends at 0.99999994 in float32
    probs[1] = [0.1, 0.2, 0.3]                             # sums to 0.6 (not normalised): u in [0.6, 1) hits no entry
    u = rng.uniform(size=(K, 1))
    u[0, 0] = 0.99999997                                   # >= the last cumsum value of row 0
    u[1, 0] = 0.75
    u[2, 0] = float(np.cumsum(probs[2])[-1])               # exactly the last cumsum value: no entry is larger
    saved = np.random.rand, np.random.normal
    try:
        np.random.rand = lambda *shape: u.reshape(shape)
        choices = np.asarray(a3c_worker.TickerGatedTraderWorker.get_random_discrete_action(probs))
        mu = rng.normal(size=(K, 3)).astype(np.float32)
        sigma = (np.abs(rng.normal(size=(K, 3))) + 0.1).astype(np.float32)
        nz = rng.normal(size=K)
        raw = []
        for k in range(0, K, 2):      # one env = two assets: rows (k, k+1)
            np.random.normal = lambda size=None, _n=nz[k:k + 2]: _n.reshape(size)
            raw.append(a3c_worker.TickerGatedTraderWorker.get_random_action(None, mu[k:k + 2], sigma[k:k + 2], choices[k:k + 2]))
        raw = np.concatenate(raw)
    finally:
        np.random.rand, np.random.normal = saved
    disc, frac = a3c_worker.TickerGatedTraderWorker.transform_raw_action(None, choices, raw)
    sp = TickerTraderStateProcessor(2)
    hist = [rng.normal(size=7) for _ in range(9)]
    temporal = sp.process_temporal_states(hist)
    np.savez_compressed(os.path.join(HERE, "gated_worker.npz"), probs=probs, u=u[:, 0], choices=np.asarray(choices), mu=mu,
                        sigma=sigma, normals=nz, raw=np.asarray(raw, np.float64), disc=np.asarray(disc), frac=np.asarray(frac, np.float64),
                        history=np.stack(hist), temporal=np.asarray(temporal, np.float64))
    print("wrote gated_worker.npz", choices[:4], raw[:4])


if __name__ == "__main__":
    main()
