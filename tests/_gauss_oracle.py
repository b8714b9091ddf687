"""float64 restatement of the A3C Gaussian agent (include/goldsrl_gaussnet.h): the reference's GaussianPolicyEstimator +
ValueEstimator on the shared rnn_graph_lstm trunk (a3c/estimators.py:18-28, 241-417), both losses and their gradients, clip +
TF 1.x RMSProp + the lr decay, and the GaussianWorker's acting / window / GAE / update as SolowWorker and TradeWorker run it
(a3c/worker.py:69-341, 394-442).  The trunk forward, the optimiser and the lr decay are tests/_gated_oracle.py's; the sizes
(static = temporal width D, actions A) are read off the parameter shapes."""
import numpy as np

import _gated_oracle as G
from oracle import nets as NN
from oracle import oracle as O

H, S = G.H, G.S
RS_GAUSS_ACTION = 19
LOG_SQRT_2PI = G.LOG_SQRT_2PI
SOLOW = dict(static_size=2, temporal_size=2, num_actions=1)
TRADE = dict(static_size=5, temporal_size=5, num_actions=2)
LB, UB, SIGMA_EPS = -5.0, 5.0, 1e-3

lr_at, rmsprop = G.lr_at, G.rmsprop


def param_shapes(static_size=2, temporal_size=2, num_actions=1):
    trunk = NN.flat_param_shapes(static_size=static_size, temporal_size=temporal_size)[:10]
    X, A = 3 * H, num_actions
    return trunk + [
        ("mu1_w", (X, 2 * S)), ("mu1_b", (2 * S,)), ("mu2_w", (2 * S, S)), ("mu2_b", (S,)), ("mu3_w", (S, A)), ("mu3_b", (A,)),
        ("sigma1_w", (X, 2 * S)), ("sigma1_b", (2 * S,)), ("sigma2_w", (2 * S, S)), ("sigma2_b", (S,)), ("sigma3_w", (S, A)), ("sigma3_b", (A,)),
        ("value1_w", (X, 2 * S)), ("value1_b", (2 * S,)), ("value2_w", (2 * S, 1)), ("value2_b", (1,)),
    ]


def num_params(**sizes):
    return sum(int(np.prod(s)) for _, s in param_shapes(**sizes))       # Solow 148 547, TradeAR1 (2 assets) 149 285


def names(**sizes):
    return [n for n, _ in param_shapes(**sizes)]


POLICY_BLOCKS = [n for n in names() if not n.startswith("value")]
VALUE_BLOCKS = names()[:10] + ["value1_w", "value1_b", "value2_w", "value2_b"]


def sizes_of(p):
    return dict(static_size=p["static1_w"].shape[0], temporal_size=p["gru_gates_w"].shape[0] - H, num_actions=p["mu3_b"].shape[0])


def unflatten(flat, **sizes):
    return NN.unflatten_params(np.asarray(flat, np.float64), param_shapes(**sizes))


def flatten(p):
    return np.concatenate([np.asarray(p[n], np.float64).reshape(-1) for n, _ in param_shapes(**sizes_of(p))])


def block_ranges(**sizes):
    out, o = {}, 0
    for n, s in param_shapes(**sizes):
        k = int(np.prod(s))
        out[n] = (o, o + k)
        o += k
    return out


def init(seed=3, **sizes):
    """default_init_gauss's rule: glorot-uniform kernels, zero biases, GRU gate bias 1, sigma3 bias -1 (estimators.py:289)."""
    rng = np.random.RandomState(seed)
    p = {}
    for n, s in param_shapes(**sizes):
        if n.endswith("_w"):
            p[n] = NN.glorot_uniform(rng, s)
        else:
            p[n] = np.ones(s) if n == "gru_gates_b" else (-np.ones(s) if n == "sigma3_b" else np.zeros(s))
    return p


_sigmoid = G._sigmoid


def forward(p, states, windows, scale=1.0, keep=False):
    """mu, sigma (n,A), values (n,)."""
    states = np.asarray(states, np.float64); windows = np.asarray(windows, np.float64)
    x, tc = G._trunk(p, states, windows)
    m1 = np.maximum(x @ p["mu1_w"] + p["mu1_b"], 0); m2 = np.tanh(m1 @ p["mu2_w"] + p["mu2_b"])
    th = np.tanh(m2 @ p["mu3_w"] + p["mu3_b"])
    mu = (UB - LB) / 2.0 * th + (LB + UB) / 2.0
    g1 = np.maximum(x @ p["sigma1_w"] + p["sigma1_b"], 0); g2 = np.tanh(g1 @ p["sigma2_w"] + p["sigma2_b"])
    sg = _sigmoid(g2 @ p["sigma3_w"] + p["sigma3_b"])
    sigma = sg + SIGMA_EPS
    v1 = np.tanh(x @ p["value1_w"] + p["value1_b"])
    values = scale * (v1 @ p["value2_w"] + p["value2_b"])[:, 0]
    if not keep:
        return mu, sigma, values
    return mu, sigma, values, dict(tc, x=x, m1=m1, m2=m2, th=th, g1=g1, g2=g2, sg=sg, v1=v1, windows=windows, states=states)


def losses(p, states, windows, raw, adv, targets, weights=None, mult=1.0, scale=1.0):
    """policy loss, value loss, entropy mean (weighted) -- the quantities the device reports."""
    mu, sigma, values = forward(p, states, windows, scale)
    n = mu.shape[0]
    w = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    z = (np.asarray(raw, np.float64) - mu) / sigma
    nll = 0.5 * z ** 2 + np.log(sigma) + LOG_SQRT_2PI
    cp = mult * w * np.asarray(adv, np.float64)
    pl = np.sum(nll * cp[:, None])
    vl = np.sum(mult * w * 0.5 * (values - np.asarray(targets, np.float64)) ** 2 / scale)
    ent = 0.5 + LOG_SQRT_2PI + np.log(sigma)
    ent_mean = np.sum(w[:, None] * ent) / (mu.shape[1] * np.sum(w)) if np.sum(w) > 0 else 0.0
    return pl, vl, ent_mean


def _trunk_bwd(p, c, dx, g):
    """_gated_oracle._trunk_bwd with the temporal width read off the window."""
    D = c["windows"].shape[2]
    ddt, ds2 = dx[:, :2 * H] * (c["dt"] > 0), dx[:, 2 * H:] * (c["s2"] > 0)
    ds1 = G._dense_bwd(p, g, "static2", c["s1"], ds2) * (c["s1"] > 0)
    G._dense_bwd(p, g, "static1", c["states"], ds1)
    dh = G._dense_bwd(p, g, "temporal", c["h"], ddt)
    for k in ("gru_gates_w", "gru_gates_b", "gru_cand_w", "gru_cand_b"):
        g[k] = np.zeros_like(p[k])
    win, length = c["windows"], c["length"]
    for t in reversed(range(win.shape[1])):
        act = (t < length)[:, None]
        hp, r, u, cc = c["hs"][t], c["rs"][t], c["us"][t], c["cs"][t]
        x = win[:, t]
        dhn = np.where(act, dh, 0.0)
        du, dcand, dh_keep = dhn * (hp - cc), dhn * (1 - u), dhn * u
        dzc = dcand * (1 - cc ** 2)
        g["gru_cand_w"] += np.concatenate([x, r * hp], 1).T @ dzc; g["gru_cand_b"] += dzc.sum(0)
        drh = (dzc @ p["gru_cand_w"].T)[:, D:]
        dzg = np.concatenate([drh * hp * r * (1 - r), du * u * (1 - u)], 1)
        g["gru_gates_w"] += np.concatenate([x, hp], 1).T @ dzg; g["gru_gates_b"] += dzg.sum(0)
        dh_prev = dh_keep + drh * r + (dzg @ p["gru_gates_w"].T)[:, D:]
        dh = np.where(act, dh_prev, dh)


def grads(p, states, windows, raw, adv, targets, weights=None, mult=1.0, scale=1.0):
    """(policy loss, value loss, entropy mean), policy gradient, value gradient (dicts over the block names; blocks a loss does not
    reach are 0)."""
    mu, sigma, values, c = forward(p, states, windows, scale, keep=True)
    n = mu.shape[0]
    w = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    raw = np.asarray(raw, np.float64)
    cp = (mult * w * np.asarray(adv, np.float64))[:, None]
    d = raw - mu
    gp, gv = {}, {}
    # mu tower: d nll / d mu = -(a - mu) / sigma^2, through mu = 5 tanh(z)
    dzm = cp * (-d / sigma ** 2) * ((UB - LB) / 2.0) * (1 - c["th"] ** 2)
    d2 = G._dense_bwd(p, gp, "mu3", c["m2"], dzm) * (1 - c["m2"] ** 2)
    d1 = G._dense_bwd(p, gp, "mu2", c["m1"], d2) * (c["m1"] > 0)
    dx = G._dense_bwd(p, gp, "mu1", c["x"], d1)
    # sigma tower: d nll / d sigma = 1 / sigma - (a - mu)^2 / sigma^3, through sigma = sigmoid(z) + 1e-3
    dzs = cp * (1.0 / sigma - d ** 2 / sigma ** 3) * c["sg"] * (1 - c["sg"])
    d2 = G._dense_bwd(p, gp, "sigma3", c["g2"], dzs) * (1 - c["g2"] ** 2)
    d1 = G._dense_bwd(p, gp, "sigma2", c["g1"], d2) * (c["g1"] > 0)
    dx = dx + G._dense_bwd(p, gp, "sigma1", c["x"], d1)
    _trunk_bwd(p, c, dx, gp)
    # value head
    dz = (mult * w * (values - np.asarray(targets, np.float64)))[:, None]
    dv1 = G._dense_bwd(p, gv, "value2", c["v1"], dz) * (1 - c["v1"] ** 2)
    dxv = G._dense_bwd(p, gv, "value1", c["x"], dv1)
    _trunk_bwd(p, c, dxv, gv)
    for g in (gp, gv):
        for k, s in param_shapes(**sizes_of(p)):
            g[k] = np.asarray(g.get(k, np.zeros(s)), np.float64).reshape(s)
    return losses(p, states, windows, raw, adv, targets, weights, mult, scale), gp, gv


# ------------------------------------------------------------------------------------------ optimiser
def policy_mask(**sizes):
    r = block_ranges(**sizes)
    m = np.zeros(num_params(**sizes), bool)
    m[:r["value1_w"][0]] = True
    return m


def value_mask(**sizes):
    r = block_ranges(**sizes)
    m = np.zeros(num_params(**sizes), bool)
    m[:r["mu1_w"][0]] = True
    m[r["value1_w"][0]:] = True
    return m


def apply_update(params, gp_flat, gv_flat, msp, msv, global_step, lr0, sizes, clip=40.0, rho=0.99, eps=0.1, rate=0.96, steps=100000):
    """clip each gradient to `clip` on its own, two RMSProp steps from the same pre-update parameters: (w - step_p) - step_v."""
    gpc, normp = NN.clip_by_global_norm(gp_flat, clip)
    gvc, normv = NN.clip_by_global_norm(gv_flat, clip)
    lr = lr_at(lr0, global_step, rate, steps)
    pm, vm = policy_mask(**sizes), value_mask(**sizes)
    w = np.array(params, np.float64)
    msp, msv = np.array(msp, np.float64), np.array(msv, np.float64)
    wp, msp_n = rmsprop(w, gpc, msp, lr, rho, eps)
    w = np.where(pm, wp, w); msp = np.where(pm, msp_n, msp)
    wv, msv_n = rmsprop(w, gvc, msv, lr, rho, eps)
    w = np.where(vm, wv, w); msv = np.where(vm, msv_n, msv)
    return w, msp, msv, global_step + 2, lr, normp, normv


# ------------------------------------------------------------------------------------------ acting, window, returns
def draws(seed, env_ids, counter, num_actions):
    """normals of shape (len(env_ids), A): the Philox draws of include/goldsrl_gaussnet.h."""
    env_ids = np.asarray(env_ids, np.uint64)
    return np.stack([O.normal_pair(O.rng_block(seed, env_ids, counter, RS_GAUSS_ACTION, a))[0] for a in range(num_actions)], 1)


def act(mu32, sigma32, n, tanh_action=False):
    """raw (A,) float32 and the env's action (A,) float32 for one env: SolowWorker.get_random_action + the worker's sigmoid
    (worker.py:17-34, 410-415) in the device's float32 form, TradeWorker's tanh (:440-442)."""
    mu32, sigma32 = np.asarray(mu32, np.float32).reshape(-1), np.asarray(sigma32, np.float32).reshape(-1)
    raw = (mu32.astype(np.float64) + sigma32.astype(np.float64) * np.asarray(n, np.float64).reshape(-1)).astype(np.float32)
    if tanh_action:
        return raw, np.tanh(raw)
    z = np.exp(-np.abs(raw))
    one = np.float32(1.0)
    return raw, np.where(raw >= 0, one / (one + z), z / (one + z)).astype(np.float32)


def window(rows, R):
    """pad_sequences(padding='post', maxlen=R) of the episode's last min(k+1, R) processed states (rows: (k+1, D), current last)."""
    rows = np.asarray(rows)[-R:]
    w = np.zeros((R, rows.shape[1]), rows.dtype)
    w[:len(rows)] = rows
    return w


def replay_windows(states, dones, R, term_states=None):
    """Windows and weights of a rollout whose first step starts fresh episodes: states (T,E,D) as recorded, dones (T,E).
    With term_states (T,E,D) also the window each finished episode ends in (its terminal state last; zero where none ended)."""
    T, E = dones.shape
    D = states.shape[2]
    win = np.zeros((T, E, R, D), np.float32)
    wts = np.zeros((T, E), np.float32)
    twin = np.zeros((T, E, R, D), np.float32)
    for e in range(E):
        rows = []
        for t in range(T):
            rows.append(states[t, e])
            win[t, e] = window(rows, R)
            wts[t, e] = 1.0 if len(rows) >= R else 0.0
            if dones[t, e]:
                if term_states is not None:
                    twin[t, e] = window(rows + [term_states[t, e]], R)
                rows = []
    return (win, wts) if term_states is None else (win, wts, twin)


def gae_segments(rewards, values, boot, dones, term_values=None, always_bootstrap=False, gamma=0.99, lam=0.96, scale=1.0):
    """The worker's GAE per env column, cut at episode ends (worker.py:241-294): behind a finished episode the next value is
    term_values[t] (always_bootstrap) or done_penalty = 0, and the running advantage restarts.  (T,E) inputs, boot (E,): the value
    behind the last step where it ended no episode.  Returns adv / scale and the value targets."""
    T = rewards.shape[0]
    dn = np.asarray(dones) != 0
    run = np.zeros(rewards.shape[1:])
    vnext = np.array(boot, np.float64)
    adv = np.zeros(rewards.shape); tgt = np.zeros(rewards.shape)
    for t in reversed(range(T)):
        vt = np.asarray(values[t], np.float64)
        behind = np.asarray(term_values[t], np.float64) if always_bootstrap else np.zeros_like(vt)
        vnext = np.where(dn[t], behind, vnext)
        delta = np.asarray(rewards[t], np.float64) + gamma * vnext - vt
        run = delta + np.where(dn[t], 0.0, gamma * lam * run)
        tgt[t] = run + vt
        adv[t] = run / scale
        vnext = vt
    return adv, tgt


def update_feed(states, windows, raw, rewards, values, boot, gamma=0.99, lam=0.96, scale=1.0):
    """What GaussianWorker.update feeds both train ops for one worker's transitions (oldest first) whose values are `values` and
    whose bootstrap value is `boot`: everything reversed in time (worker.py:282, 294-300), advantages / scale (:332)."""
    rewards = np.asarray(rewards, np.float64); values = np.asarray(values, np.float64)
    adv, tgt = O.gae(rewards[:, None], values[:, None], np.array([boot], np.float64), gamma, lam)
    return dict(states=np.asarray(states)[::-1], history=np.asarray(windows)[::-1], actions=np.asarray(raw)[::-1],
                advantages=adv[::-1, 0] / scale, targets=tgt[::-1, 0])


def worker_update(params_flat, sizes, msp, msv, global_step, states, windows, raw, rewards, boot, lr0, gamma=0.99, lam=0.96, scale=1.0,
                  clip=40.0):
    """GaussianWorker.update (worker.py:241-325) on one worker's recorded transitions: V of the recorded states, the bootstrap value
    appended, GAE, advantages / scale to the policy, targets to the value head, both train ops.  Returns the new params, ms vectors,
    global step, the gradients and the losses."""
    p = unflatten(params_flat, **sizes)
    _, _, V = forward(p, states, windows, scale)
    feed = update_feed(states, windows, raw, rewards, V, boot, gamma, lam, scale)
    (pl, vl, ent), gp, gv = grads(p, feed["states"], feed["history"], feed["actions"], feed["advantages"], feed["targets"], None, 1.0, scale)
    out = apply_update(params_flat, flatten(gp), flatten(gv), msp, msv, global_step, lr0, sizes, clip)
    return out, flatten(gp), flatten(gv), (pl, vl, ent)
