"""float64 restatement of the A3C grid trader (include/goldsrl_gridtradenet.h): the reference's DiscretePolicyEstimator with
num_outputs = O (a3c/estimators.py:155-238: logits O * K, reshaped (-1, O, K), one softmax per output) + ValueEstimator on the shared
rnn_graph_lstm trunk, both losses and their analytic gradients, and GridSolowWorker's acting per output (a3c/worker.py:223-227,
343-391).  Generic in the state width D and in O, both read off the parameter shapes with K; at D = 2, O = 1 it is
tests/_grid_oracle.py.  The trunk and its backward, the optimiser, the windows and the GAE are tests/_gauss_oracle.py's and
tests/_grid_oracle.py's, used from there, not restated."""
import numpy as np

import _gated_oracle as G
import _gauss_oracle as A
import _grid_oracle as D1
from oracle import nets as NN
from oracle import oracle as O_

H, S, EPS = G.H, G.S, D1.EPS
RS_GRIDTRADE_ACTION = 21
LB, UB, K_DEFAULT = -1.0, 1.0, 17

lr_at, replay_windows, gae_segments = G.lr_at, A.replay_windows, A.gae_segments
choose, greedy = D1.choose, D1.greedy          # per output, on that output's K float32 probabilities


def param_shapes(K=K_DEFAULT, D=5, O=2):
    """_grid_oracle's blocks with the trunk at width D and O * K columns in probs3"""
    return NN.flat_param_shapes(static_size=D, temporal_size=D)[:10] + D1.param_shapes(O * K)[10:]


def num_params(K=K_DEFAULT, D=5, O=2):
    return sum(int(np.prod(s)) for _, s in param_shapes(K, D, O))       # D = 5, O = 2: 91 041 + 258 K


def unflatten(flat, K=K_DEFAULT, D=5, O=2):
    return NN.unflatten_params(np.asarray(flat, np.float64), param_shapes(K, D, O))


def flatten(p):
    return np.concatenate([np.asarray(p[n], np.float64).reshape(-1) for n in D1.names()])


def block_ranges(K=K_DEFAULT, D=5, O=2):
    out, o = {}, 0
    for n, s in param_shapes(K, D, O):
        out[n] = (o, o + int(np.prod(s)))
        o = out[n][1]
    return out


def init(seed=3, K=K_DEFAULT, D=5, O=2):
    """default_init_gridtrade's rule: glorot-uniform kernels, zero biases, GRU gate bias 1."""
    rng = np.random.RandomState(seed)
    return {n: NN.glorot_uniform(rng, s) if n.endswith("_w") else (np.ones(s) if n == "gru_gates_b" else np.zeros(s))
            for n, s in param_shapes(K, D, O)}


def forward(p, states, windows, scale=1.0, O=2, keep=False):
    """probs (n,O,K), values (n,): column o * K + j of probs3 is output o, choice j (the row-major reshape)."""
    states = np.asarray(states, np.float64); windows = np.asarray(windows, np.float64)
    x, tc = G._trunk(p, states, windows)
    h1 = np.maximum(x @ p["probs1_w"] + p["probs1_b"], 0); h2 = np.maximum(h1 @ p["probs2_w"] + p["probs2_b"], 0)
    logits = h2 @ p["probs3_w"] + p["probs3_b"]
    probs = G._softmax(logits.reshape(len(x), O, -1))
    v1 = np.tanh(x @ p["value1_w"] + p["value1_b"])
    values = scale * (v1 @ p["value2_w"] + p["value2_b"])[:, 0]
    if not keep:
        return probs, values
    return probs, values, dict(tc, x=x, h1=h1, h2=h2, v1=v1, windows=windows, states=states)


def _picked(probs, choices):
    n, O, _ = probs.shape
    ch = np.asarray(choices).reshape(n, O).astype(int)
    return ch, probs[np.arange(n)[:, None], np.arange(O)[None], ch]


def losses(p, states, windows, choices, adv, targets, weights=None, mult=1.0, scale=1.0, O=2):
    """policy loss (the sum over the outputs of -log(p_choice + eps)), value loss, entropy mean (per sample the mean over the
    outputs, estimators.py:206; weighted over the samples) -- the quantities the device reports."""
    probs, values = forward(p, states, windows, scale, O)
    w = np.ones(len(values)) if weights is None else np.asarray(weights, np.float64)
    pc = _picked(probs, choices)[1]
    pl = np.sum(mult * w * np.asarray(adv, np.float64) * np.sum(-np.log(pc + EPS), axis=1))
    vl = np.sum(mult * w * 0.5 * (values - np.asarray(targets, np.float64)) ** 2 / scale)
    ent = np.mean(-np.sum(probs * np.log(probs + EPS), axis=2), axis=1)
    return pl, vl, (np.sum(w * ent) / np.sum(w) if np.sum(w) > 0 else 0.0)


def grads(p, states, windows, choices, adv, targets, weights=None, mult=1.0, scale=1.0, O=2):
    """(policy loss, value loss, entropy mean), policy gradient, value gradient (dicts over the block names; blocks a loss does not
    reach are 0).  dz[o][j] = cp * p_c / (p_c + eps) * (p[o][j] - [j == c_o]) with c_o output o's OWN choice."""
    probs, values, c = forward(p, states, windows, scale, O, keep=True)
    n, _, K = probs.shape
    w = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    ch, pc = _picked(probs, choices)
    cp = mult * w * np.asarray(adv, np.float64)
    gp, gv = {}, {}
    dz = ((cp[:, None] * pc / (pc + EPS))[:, :, None] * (probs - np.eye(K)[ch])).reshape(n, O * K)
    d2 = G._dense_bwd(p, gp, "probs3", c["h2"], dz) * (c["h2"] > 0)
    d1 = G._dense_bwd(p, gp, "probs2", c["h1"], d2) * (c["h1"] > 0)
    A._trunk_bwd(p, c, G._dense_bwd(p, gp, "probs1", c["x"], d1), gp)
    dzv = (mult * w * (values - np.asarray(targets, np.float64)))[:, None]
    dv1 = G._dense_bwd(p, gv, "value2", c["v1"], dzv) * (1 - c["v1"] ** 2)
    A._trunk_bwd(p, c, G._dense_bwd(p, gv, "value1", c["x"], dv1), gv)
    for g in (gp, gv):
        for k in p:
            g[k] = np.asarray(g.get(k, np.zeros(p[k].shape)), np.float64).reshape(p[k].shape)
    return losses(p, states, windows, choices, adv, targets, weights, mult, scale, O), gp, gv


def apply_update(params, gp_flat, gv_flat, msp, msv, global_step, lr0, K=K_DEFAULT, D=5, O=2, **kw):
    """_gauss_oracle.apply_update (clip each gradient on its own, two RMSProp steps from the same pre-update parameters) under this
    net's masks, swapped in for the call as _grid_oracle.apply_update swaps its own: the policy gradient covers everything before
    the value head, the value gradient the trunk and the value head."""
    r = block_ranges(K, D, O)
    idx = np.arange(r["value2_b"][1])
    saved = A.policy_mask, A.value_mask
    A.policy_mask = lambda **_: idx < r["value1_w"][0]
    A.value_mask = lambda **_: (idx < r["probs1_w"][0]) | (idx >= r["value1_w"][0])
    try:
        return A.apply_update(params, gp_flat, gv_flat, msp, msv, global_step, lr0, {}, **kw)
    finally:
        A.policy_mask, A.value_mask = saved


def grid(K=K_DEFAULT, lb=LB, ub=UB):
    """idx_to_grid's values (worker.py:349), float64"""
    return np.linspace(lb, ub, K)


def draws(seed, env_ids, counter):
    """(u_0, u_1), each (len(env_ids),): ONE Philox block per env and step, its first uniform for output 0, its second for output 1."""
    return O_.u01_pair(O_.rng_block(seed, np.asarray(env_ids, np.uint64), counter, RS_GRIDTRADE_ACTION, 0))
