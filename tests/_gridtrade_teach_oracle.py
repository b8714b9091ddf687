"""float64 statement of the grid trader's supervised update (include/goldsrl_gridtradeteach.h): the cross-entropy of each output's
softmax to a soft label on the grid -- mass 1 - w on point lo, w on lo + 1 -- and its analytic gradient, on the forward, the tower
and trunk backward, the value loss and the entropy of tests/_gridtrade_oracle.py, used from there."""
import numpy as np

import _gated_oracle as G
import _gauss_oracle as A
import _gridtrade_oracle as GT

EPS = GT.EPS
RS_GRIDTRADE_COIN = 22


def _labels(probs, label_lo, label_w):
    """lo (n,O), then per (sample, output) the two target masses and the two probabilities they sit on.  y_lo = 1 - w is taken in
    float32, as the device takes it."""
    n, O, _ = probs.shape
    lo = np.asarray(label_lo).reshape(n, O).astype(int)
    w32 = np.asarray(label_w, np.float32).reshape(n, O)
    i, o = np.arange(n)[:, None], np.arange(O)[None]
    return lo, (np.float32(1.0) - w32).astype(np.float64), w32.astype(np.float64), probs[i, o, lo], probs[i, o, lo + 1]


def losses(p, states, windows, label_lo, label_w, targets, weights=None, mult=1.0, scale=1.0, O=2):
    """cross-entropy, value loss, entropy mean, agreement.  A term with mass 0 is skipped: it adds exactly nothing."""
    probs, values = GT.forward(p, states, windows, scale, O)
    n = len(values)
    wt = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    lo, ylo, yhi, plo, phi = _labels(probs, label_lo, label_w)
    ce = -(np.where(ylo > 0, ylo * np.log(plo + EPS), 0.0) + np.where(yhi > 0, yhi * np.log(phi + EPS), 0.0))
    zero = np.zeros(n)
    _, vl, ent = GT.losses(p, states, windows, np.zeros((n, O), int), zero, targets, weights, mult, scale, O)
    heavy = np.where(yhi > 0.5, lo + 1, lo)
    agree = np.sum(wt[:, None] * (probs.argmax(axis=2) == heavy)) / (O * np.sum(wt)) if np.sum(wt) > 0 else 0.0
    return np.sum(mult * wt * ce.sum(axis=1)), vl, ent, agree


def grads(p, states, windows, label_lo, label_w, targets, weights=None, mult=1.0, scale=1.0, O=2):
    """(the four of losses), policy gradient, value gradient: r_k = y_k p_k / (p_k + eps), dz[o][j] = c (p[o][j] (r_lo + r_hi) - r_j);
    the value gradient is _gridtrade_oracle's, which no label reaches."""
    probs, values, c = GT.forward(p, states, windows, scale, O, keep=True)
    n, _, K = probs.shape
    wt = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    lo, ylo, yhi, plo, phi = _labels(probs, label_lo, label_w)
    rlo, rhi = ylo * plo / (plo + EPS), yhi * phi / (phi + EPS)
    r = rlo[:, :, None] * np.eye(K)[lo] + rhi[:, :, None] * np.eye(K)[lo + 1]
    dz = ((mult * wt)[:, None, None] * (probs * (rlo + rhi)[:, :, None] - r)).reshape(n, O * K)
    gp = {}
    d2 = G._dense_bwd(p, gp, "probs3", c["h2"], dz) * (c["h2"] > 0)
    d1 = G._dense_bwd(p, gp, "probs2", c["h1"], d2) * (c["h1"] > 0)
    A._trunk_bwd(p, c, G._dense_bwd(p, gp, "probs1", c["x"], d1), gp)
    gp = {k: np.asarray(gp.get(k, np.zeros(p[k].shape)), np.float64).reshape(p[k].shape) for k in p}
    gv = GT.grads(p, states, windows, np.zeros((n, O), int), np.zeros(n), targets, weights, mult, scale, O)[2]
    return losses(p, states, windows, label_lo, label_w, targets, weights, mult, scale, O), gp, gv


def coin(seed, env_ids, counter):
    """the teach rollout's uniform per (env, step): the first of the block of stream 22"""
    return GT.O_.u01_pair(GT.O_.rng_block(seed, np.asarray(env_ids, np.uint64), counter, RS_GRIDTRADE_COIN, 0))[0]
