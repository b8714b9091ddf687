"""float64 restatement of the A3C discrete savings-grid agent (include/goldsrl_discretenet.h): the reference's
DiscretePolicyEstimator + ValueEstimator on the shared rnn_graph_lstm trunk (a3c/estimators.py:18-28, 155-238, 338-417) with one
output of K choices, both losses and their gradients, and GridSolowWorker's acting (a3c/worker.py:223-227, 343-391).  The trunk and
its backward, the optimiser, the windows and the GAE are tests/_gauss_oracle.py's (apply_update, replay_windows, gae_segments are
used from there, not restated); K is read off the parameter shapes."""
import numpy as np

import _gated_oracle as G
import _gauss_oracle as A
from oracle import nets as NN
from oracle import oracle as O

H, S = G.H, G.S
RS_GRID_ACTION = 20
EPS = 1e-7                      # tf.keras.backend.epsilon()
LB, UB, K_DEFAULT = 0.01, 0.99, 51

lr_at, rmsprop = G.lr_at, G.rmsprop
replay_windows, gae_segments, window = A.replay_windows, A.gae_segments, A.window


def param_shapes(K=K_DEFAULT):
    trunk = NN.flat_param_shapes(static_size=2, temporal_size=2)[:10]
    X = 3 * H
    return trunk + [
        ("probs1_w", (X, 2 * S)), ("probs1_b", (2 * S,)), ("probs2_w", (2 * S, S)), ("probs2_b", (S,)), ("probs3_w", (S, K)), ("probs3_b", (K,)),
        ("value1_w", (X, 2 * S)), ("value1_b", (2 * S,)), ("value2_w", (2 * S, 1)), ("value2_b", (1,)),
    ]


def num_params(K=K_DEFAULT):
    return sum(int(np.prod(s)) for _, s in param_shapes(K))       # 90 561 + 129 K


def names(K=K_DEFAULT):
    return [n for n, _ in param_shapes(K)]


POLICY_BLOCKS = [n for n in names() if not n.startswith("value")]
VALUE_BLOCKS = names()[:10] + ["value1_w", "value1_b", "value2_w", "value2_b"]


def K_of(p):
    return p["probs3_b"].shape[0]


def unflatten(flat, K=K_DEFAULT):
    return NN.unflatten_params(np.asarray(flat, np.float64), param_shapes(K))


def flatten(p):
    return np.concatenate([np.asarray(p[n], np.float64).reshape(-1) for n, _ in param_shapes(K_of(p))])


def block_ranges(K=K_DEFAULT):
    out, o = {}, 0
    for n, s in param_shapes(K):
        k = int(np.prod(s))
        out[n] = (o, o + k)
        o += k
    return out


def init(seed=3, K=K_DEFAULT):
    """default_init_discrete's rule: glorot-uniform kernels, zero biases, GRU gate bias 1."""
    rng = np.random.RandomState(seed)
    p = {}
    for n, s in param_shapes(K):
        if n.endswith("_w"):
            p[n] = NN.glorot_uniform(rng, s)
        else:
            p[n] = np.ones(s) if n == "gru_gates_b" else np.zeros(s)
    return p


def forward(p, states, windows, scale=1.0, keep=False):
    """probs (n,K), values (n,)."""
    states = np.asarray(states, np.float64); windows = np.asarray(windows, np.float64)
    x, tc = G._trunk(p, states, windows)
    h1 = np.maximum(x @ p["probs1_w"] + p["probs1_b"], 0); h2 = np.maximum(h1 @ p["probs2_w"] + p["probs2_b"], 0)
    probs = G._softmax(h2 @ p["probs3_w"] + p["probs3_b"])
    v1 = np.tanh(x @ p["value1_w"] + p["value1_b"])
    values = scale * (v1 @ p["value2_w"] + p["value2_b"])[:, 0]
    if not keep:
        return probs, values
    return probs, values, dict(tc, x=x, h1=h1, h2=h2, v1=v1, windows=windows, states=states)


def losses(p, states, windows, choices, adv, targets, weights=None, mult=1.0, scale=1.0):
    """policy loss, value loss, entropy mean (weighted) -- the quantities the device reports."""
    probs, values = forward(p, states, windows, scale)
    n = probs.shape[0]
    w = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    ch = np.asarray(choices).reshape(-1).astype(int)
    pc = probs[np.arange(n), ch]
    pl = np.sum(mult * w * np.asarray(adv, np.float64) * -np.log(pc + EPS))
    vl = np.sum(mult * w * 0.5 * (values - np.asarray(targets, np.float64)) ** 2 / scale)
    ent = -np.sum(probs * np.log(probs + EPS), axis=1)
    ent_mean = np.sum(w * ent) / np.sum(w) if np.sum(w) > 0 else 0.0
    return pl, vl, ent_mean


def grads(p, states, windows, choices, adv, targets, weights=None, mult=1.0, scale=1.0):
    """(policy loss, value loss, entropy mean), policy gradient, value gradient (dicts over the block names; blocks a loss does not
    reach are 0).  d/dlogit_j of -log(p_c + eps) = p_c / (p_c + eps) * (p_j - [j == c]): the epsilon stays in the gradient."""
    probs, values, c = forward(p, states, windows, scale, keep=True)
    n, K = probs.shape
    w = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    ch = np.asarray(choices).reshape(-1).astype(int)
    cp = mult * w * np.asarray(adv, np.float64)
    pc = probs[np.arange(n), ch]
    gp, gv = {}, {}
    dz = (cp * pc / (pc + EPS))[:, None] * (probs - np.eye(K)[ch])
    d2 = G._dense_bwd(p, gp, "probs3", c["h2"], dz) * (c["h2"] > 0)
    d1 = G._dense_bwd(p, gp, "probs2", c["h1"], d2) * (c["h1"] > 0)
    dx = G._dense_bwd(p, gp, "probs1", c["x"], d1)
    A._trunk_bwd(p, c, dx, gp)
    dzv = (mult * w * (values - np.asarray(targets, np.float64)))[:, None]
    dv1 = G._dense_bwd(p, gv, "value2", c["v1"], dzv) * (1 - c["v1"] ** 2)
    dxv = G._dense_bwd(p, gv, "value1", c["x"], dv1)
    A._trunk_bwd(p, c, dxv, gv)
    for g in (gp, gv):
        for k, s in param_shapes(K):
            g[k] = np.asarray(g.get(k, np.zeros(s)), np.float64).reshape(s)
    return losses(p, states, windows, choices, adv, targets, weights, mult, scale), gp, gv


# ------------------------------------------------------------------------------------------ optimiser
def policy_mask(K=K_DEFAULT):
    m = np.zeros(num_params(K), bool)
    m[:block_ranges(K)["value1_w"][0]] = True
    return m


def value_mask(K=K_DEFAULT):
    r = block_ranges(K)
    m = np.zeros(num_params(K), bool)
    m[:r["probs1_w"][0]] = True
    m[r["value1_w"][0]:] = True
    return m


def apply_update(params, gp_flat, gv_flat, msp, msv, global_step, lr0, K=K_DEFAULT, **kw):
    """_gauss_oracle.apply_update (clip each gradient on its own, two RMSProp steps from the same pre-update parameters) under this
    net's masks: it looks its two masks up by the Gaussian block names, which this net does not have, so they are swapped for the
    call."""
    saved = A.policy_mask, A.value_mask
    A.policy_mask, A.value_mask = (lambda **_: policy_mask(K)), (lambda **_: value_mask(K))
    try:
        return A.apply_update(params, gp_flat, gv_flat, msp, msv, global_step, lr0, {}, **kw)
    finally:
        A.policy_mask, A.value_mask = saved


# ------------------------------------------------------------------------------------------ acting
def grid(K=K_DEFAULT, lb=LB, ub=UB):
    """idx_to_grid's values (worker.py:349), float64"""
    return np.linspace(lb, ub, K)


def draws(seed, env_ids, counter):
    """u of shape (len(env_ids),): the Philox draws of include/goldsrl_discretenet.h."""
    return O.u01_pair(O.rng_block(seed, np.asarray(env_ids, np.uint64), counter, RS_GRID_ACTION, 0))[0]


def choose(probs32, u):
    """get_random_discrete_action (worker.py:223-227) for one sample: the first i with u < the float32 cumulative sum in index
    order; 0 if none (argmax of an all-False row)."""
    cum = np.cumsum(np.asarray(probs32, np.float32).reshape(-1), dtype=np.float32)
    return int((u < cum.astype(np.float64)).argmax())


def greedy(probs32):
    """the evident intention of GridSolowWorker.get_greedy_action: np.argmax, the first index of the largest float32 probability"""
    return int(np.argmax(np.asarray(probs32, np.float32).reshape(-1)))


def update_feed(states, windows, choices, rewards, values, boot, gamma=0.99, lam=0.96, scale=1.0):
    """_gauss_oracle.update_feed with the int choices in the actions' place (GridSolowWorker.fill_feed_dict_for_update)."""
    f = A.update_feed(states, windows, np.asarray(choices).reshape(-1, 1), rewards, values, boot, gamma, lam, scale)
    f["actions"] = f["actions"].astype(np.int64)
    return f


def worker_update(params_flat, K, msp, msv, global_step, states, windows, choices, rewards, boot, lr0, gamma=0.99, lam=0.96, scale=1.0,
                  clip=40.0):
    """GaussianWorker.update (worker.py:241-325) as GridSolowWorker runs it on one worker's recorded transitions."""
    p = unflatten(params_flat, K)
    _, V = forward(p, states, windows, scale)
    feed = update_feed(states, windows, choices, rewards, V, boot, gamma, lam, scale)
    (pl, vl, ent), gp, gv = grads(p, feed["states"], feed["history"], feed["actions"], feed["advantages"], feed["targets"], None, 1.0, scale)
    out = apply_update(params_flat, flatten(gp), flatten(gv), msp, msv, global_step, lr0, K, clip=clip)
    return out, flatten(gp), flatten(gv), (pl, vl, ent)
