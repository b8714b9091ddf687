"""float64 restatement of the Ticker gated trader (include/goldsrl_gatednet.h): the reference's DiscreteAndContPolicyEstimator +
ValueEstimator on the shared rnn_graph_lstm trunk (a3c/estimators.py:18-152, 338-417), both losses and their gradients, clip +
TF 1.x RMSProp + the lr decay, and the TickerGatedTraderWorker's acting / window / GAE / update (a3c/worker.py:191-294, 445-494).
The GRU trunk is oracle/nets.py's (gru_last_state); its back-propagation through time is the one of nets.flat_loss_and_grads."""
import numpy as np

from oracle import nets as NN
from oracle import oracle as O

N_ASSETS, N_CHOICES, S0, D, H, S = 2, 3, 7, 4, 32, 128
RS_GATED_ACTION = 18
LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)


def param_shapes():
    trunk = NN.flat_param_shapes(static_size=S0, temporal_size=D)[:10]
    X = 3 * H
    return trunk + [
        ("class1_w", (X, 2 * S)), ("class1_b", (2 * S,)), ("class2_w", (2 * S, S)), ("class2_b", (S,)),
        ("class3_w", (S, 6)), ("class3_b", (6,)),
        ("normal1_w", (X, 2 * S)), ("normal1_b", (2 * S,)), ("normal2_w", (2 * S, S)), ("normal2_b", (S,)),
        ("normal3_w", (S, 12)), ("normal3_b", (12,)),
        ("value1_w", (X, 2 * S)), ("value1_b", (2 * S,)), ("value2_w", (2 * S, 1)), ("value2_b", (1,)),
    ]


SHAPES = param_shapes()
NUM_PARAMS = sum(int(np.prod(s)) for _, s in SHAPES)          # 151 123
POLICY_BLOCKS = [n for n, _ in SHAPES if not n.startswith("value")]
VALUE_BLOCKS = [n for n, _ in SHAPES[:10]] + ["value1_w", "value1_b", "value2_w", "value2_b"]


def unflatten(flat):
    return NN.unflatten_params(np.asarray(flat, np.float64), SHAPES)


def flatten(p):
    return np.concatenate([np.asarray(p[n], np.float64).reshape(-1) for n, _ in SHAPES])


def block_ranges():
    out, o = {}, 0
    for n, s in SHAPES:
        k = int(np.prod(s))
        out[n] = (o, o + k)
        o += k
    return out


def init(seed=3):
    """flat_init's rule: glorot-uniform kernels, zero biases, GRU gate bias 1."""
    rng = np.random.RandomState(seed)
    p = {}
    for n, s in SHAPES:
        p[n] = NN.glorot_uniform(rng, s) if n.endswith("_w") else (np.ones(s) if n == "gru_gates_b" else np.zeros(s))
    return p


def _sigmoid(x):
    with np.errstate(over="ignore"):          # exp(-x) = inf far below 0: 1 / inf = 0 is the limit, the same bits without the warning
        return 1.0 / (1.0 + np.exp(-x))


def _softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def _softmax(l):
    e = np.exp(l - l.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def _trunk(p, states, windows):
    N, T, _ = windows.shape
    length = np.sign(np.max(np.abs(windows), axis=2)).sum(axis=1).astype(int)
    hs, rs, us, cs = [np.zeros((N, H))], [], [], []
    h = hs[0]
    for t in range(T):
        x = windows[:, t]
        gates = _sigmoid(np.concatenate([x, h], 1) @ p["gru_gates_w"] + p["gru_gates_b"])
        r, u = gates[:, :H], gates[:, H:]
        c = np.tanh(np.concatenate([x, r * h], 1) @ p["gru_cand_w"] + p["gru_cand_b"])
        h = np.where((t < length)[:, None], u * h + (1 - u) * c, h)
        rs.append(r); us.append(u); cs.append(c); hs.append(h)
    dt_ = np.maximum(h @ p["temporal_w"] + p["temporal_b"], 0)
    s1 = np.maximum(states @ p["static1_w"] + p["static1_b"], 0)
    s2 = np.maximum(s1 @ p["static2_w"] + p["static2_b"], 0)
    return np.concatenate([dt_, s2], axis=1), dict(length=length, hs=hs, rs=rs, us=us, cs=cs, h=h, dt=dt_, s1=s1, s2=s2)


def forward(p, states, windows, scale=1.0, keep=False):
    """probs, mu, sigma (n,2,3), values (n,)."""
    states = np.asarray(states, np.float64); windows = np.asarray(windows, np.float64)
    x, tc = _trunk(p, states, windows)
    h = NN.gru_last_state(p, windows)
    assert np.allclose(h, tc["h"], rtol=0, atol=1e-12)       # the trunk is oracle/nets.py's (up to BLAS summation order)
    c1 = np.maximum(x @ p["class1_w"] + p["class1_b"], 0); c2 = np.maximum(c1 @ p["class2_w"] + p["class2_b"], 0)
    logits = (c2 @ p["class3_w"] + p["class3_b"]).reshape(-1, N_ASSETS, N_CHOICES)
    probs = _softmax(logits)
    n1 = np.maximum(x @ p["normal1_w"] + p["normal1_b"], 0); n2 = np.maximum(n1 @ p["normal2_w"] + p["normal2_b"], 0)
    nout = (n2 @ p["normal3_w"] + p["normal3_b"]).reshape(-1, N_ASSETS, N_CHOICES, 2)
    mu, rs = nout[..., 0], nout[..., 1]
    sigma = _softplus(rs) + 1e-7
    v1 = np.tanh(x @ p["value1_w"] + p["value1_b"])
    values = scale * (v1 @ p["value2_w"] + p["value2_b"])[:, 0]
    if not keep:
        return probs, mu, sigma, values
    return probs, mu, sigma, values, dict(tc, x=x, c1=c1, c2=c2, n1=n1, n2=n2, rsig=rs, v1=v1, windows=windows, states=states)


def losses(p, states, windows, choices, raw, adv, targets, weights=None, mult=1.0, scale=1.0):
    """policy loss, value loss, entropy mean (weighted) -- the quantities the device reports."""
    probs, mu, sigma, values = forward(p, states, windows, scale)
    n = probs.shape[0]
    w = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    ch = np.asarray(choices, int)
    idx = np.arange(n)[:, None], np.arange(N_ASSETS)[None, :]
    pc, mc, sc = probs[idx + (ch,)], mu[idx + (ch,)], sigma[idx + (ch,)]
    z = (np.asarray(raw, np.float64) - mc) / sc
    nll = -np.log(pc) + 0.5 * z ** 2 + np.log(sc) + LOG_SQRT_2PI
    cp = mult * w * np.asarray(adv, np.float64)
    pl = np.sum(nll * cp[:, None])
    vl = np.sum(mult * w * 0.5 * (values - np.asarray(targets, np.float64)) ** 2 / scale)
    plogp = np.where(probs > 0, probs * np.log(np.where(probs > 0, probs, 1.0)), 0.0)      # 0 log 0 = 0 (a float64 softmax can underflow)
    ent = -plogp.sum(-1) + 0.5 + LOG_SQRT_2PI + np.log(sc)
    ent_mean = np.sum(w[:, None] * ent) / (2.0 * np.sum(w)) if np.sum(w) > 0 else 0.0
    return pl, vl, ent_mean


def _dense_bwd(p, g, name, x, dz):
    g[name + "_w"] = g.get(name + "_w", 0) + x.T @ dz
    g[name + "_b"] = g.get(name + "_b", 0) + dz.sum(0)
    return dz @ p[name + "_w"].T


def _trunk_bwd(p, c, dx, g):
    ddt, ds2 = dx[:, :2 * H] * (c["dt"] > 0), dx[:, 2 * H:] * (c["s2"] > 0)
    ds1 = _dense_bwd(p, g, "static2", c["s1"], ds2) * (c["s1"] > 0)
    _dense_bwd(p, g, "static1", c["states"], ds1)
    dh = _dense_bwd(p, g, "temporal", c["h"], ddt)
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


def grads(p, states, windows, choices, raw, adv, targets, weights=None, mult=1.0, scale=1.0):
    """(policy loss, value loss, entropy mean), policy gradient, value gradient (dicts over SHAPES' names; blocks a loss does not reach are 0)."""
    probs, mu, sigma, values, c = forward(p, states, windows, scale, keep=True)
    n = probs.shape[0]
    w = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    ch = np.asarray(choices, int)
    raw = np.asarray(raw, np.float64)
    cp = mult * w * np.asarray(adv, np.float64)
    onehot = np.eye(N_CHOICES)[ch]                                        # (n,2,3)
    gp, gv = {}, {}
    # class tower
    dl = (cp[:, None, None] * (probs - onehot)).reshape(n, 6)
    d2 = _dense_bwd(p, gp, "class3", c["c2"], dl) * (c["c2"] > 0)
    d1 = _dense_bwd(p, gp, "class2", c["c1"], d2) * (c["c1"] > 0)
    dx = _dense_bwd(p, gp, "class1", c["x"], d1)
    # normal tower: only the chosen (mu, sigma)
    sig = sigma; d = raw[:, :, None] - mu
    dmu = onehot * cp[:, None, None] * (-d / sig ** 2)
    dsg = onehot * cp[:, None, None] * (1.0 / sig - d ** 2 / sig ** 3)
    dn = np.stack([dmu, dsg * _sigmoid(c["rsig"])], axis=-1).reshape(n, 12)
    d2 = _dense_bwd(p, gp, "normal3", c["n2"], dn) * (c["n2"] > 0)
    d1 = _dense_bwd(p, gp, "normal2", c["n1"], d2) * (c["n1"] > 0)
    dx = dx + _dense_bwd(p, gp, "normal1", c["x"], d1)
    _trunk_bwd(p, c, dx, gp)
    # value head
    dz = (mult * w * (values - np.asarray(targets, np.float64)))[:, None]
    dv1 = _dense_bwd(p, gv, "value2", c["v1"], dz) * (1 - c["v1"] ** 2)
    dxv = _dense_bwd(p, gv, "value1", c["x"], dv1)
    _trunk_bwd(p, c, dxv, gv)
    for g in (gp, gv):
        for k, s in SHAPES:
            g[k] = np.asarray(g.get(k, np.zeros(s)), np.float64).reshape(s)
    return losses(p, states, windows, choices, raw, adv, targets, weights, mult, scale), gp, gv


# ------------------------------------------------------------------------------------------ optimiser
def lr_at(lr0, global_step, rate=0.96, steps=100000):
    """tf.train.exponential_decay(staircase=False) at the global step before the update."""
    return lr0 * rate ** (global_step / steps)


def rmsprop(w, g, ms, lr, rho=0.99, eps=0.1):
    """TF 1.x RMSPropOptimizer, momentum 0 (ms starts at 1)."""
    ms = rho * ms + (1 - rho) * g * g
    return w - lr * g / np.sqrt(ms + eps), ms


def policy_mask():
    r = block_ranges()
    m = np.zeros(NUM_PARAMS, bool)
    m[:r["value1_w"][0]] = True
    return m


def value_mask():
    r = block_ranges()
    m = np.zeros(NUM_PARAMS, bool)
    m[:r["class1_w"][0]] = True
    m[r["value1_w"][0]:] = True
    return m


def apply_update(params, gp_flat, gv_flat, msp, msv, global_step, lr0, clip=40.0, rho=0.99, eps=0.1, rate=0.96, steps=100000):
    """clip each gradient to `clip` on its own, two RMSProp steps from the same pre-update parameters: (w - step_p) - step_v."""
    gpc, normp = NN.clip_by_global_norm(gp_flat, clip)
    gvc, normv = NN.clip_by_global_norm(gv_flat, clip)
    lr = lr_at(lr0, global_step, rate, steps)
    pm, vm = policy_mask(), value_mask()
    w = np.array(params, np.float64)
    msp, msv = np.array(msp, np.float64), np.array(msv, np.float64)
    wp, msp_n = rmsprop(w, gpc, msp, lr, rho, eps)
    w = np.where(pm, wp, w); msp = np.where(pm, msp_n, msp)
    wv, msv_n = rmsprop(w, gvc, msv, lr, rho, eps)
    w = np.where(vm, wv, w); msv = np.where(vm, msv_n, msv)
    return w, msp, msv, global_step + 2, lr, normp, normv


# ------------------------------------------------------------------------------------------ acting, window, returns
def discrete_choice(probs32, u):
    """get_random_discrete_action for one asset: the first c with u < float32 cumsum; 0 if none (argmax of an all-False row)."""
    cum = np.cumsum(np.asarray(probs32, np.float32))          # float32 accumulation in index order
    hits = u < cum
    return int(np.argmax(hits))


def draws(seed, env_ids, counter):
    """(u, n) of shape (len(env_ids), 2): the Philox draws of include/goldsrl_gatednet.h."""
    env_ids = np.asarray(env_ids, np.uint64)
    u = np.stack([O.u01_pair(O.rng_block(seed, env_ids, counter, RS_GATED_ACTION, 2 * a))[0] for a in range(N_ASSETS)], 1)
    n = np.stack([O.normal_pair(O.rng_block(seed, env_ids, counter, RS_GATED_ACTION, 2 * a + 1))[0] for a in range(N_ASSETS)], 1)
    return u, n


def act(probs32, mu32, sigma32, u, n):
    """choice (2,), raw (2,) float32, env fraction (2,) float32 for one env."""
    ch = np.array([discrete_choice(probs32[a], u[a]) for a in range(N_ASSETS)])
    raw = np.array([np.float32(float(mu32[a, ch[a]]) + float(sigma32[a, ch[a]]) * n[a]) for a in range(N_ASSETS)], np.float32)
    frac = (1.0 / (1.0 + np.exp(-raw.astype(np.float64)))).astype(np.float32)
    return ch, raw, frac


def window(rows, R):
    """pad_sequences(padding='post', maxlen=R) of the episode's last min(k+1, R) temporal rows (rows: (k+1, 4), current last)."""
    rows = np.asarray(rows)[-R:]
    w = np.zeros((R, D), rows.dtype)
    w[:len(rows)] = rows
    return w


def replay_windows(states, dones, R):
    """Windows and weights of a rollout whose first step starts fresh episodes: states (T,E,7) as recorded, dones (T,E)."""
    T, E = dones.shape
    win = np.zeros((T, E, R, D), np.float32)
    wts = np.zeros((T, E), np.float32)
    for e in range(E):
        rows = []
        for t in range(T):
            rows.append(states[t, e, 3:])
            win[t, e] = window(rows, R)
            wts[t, e] = 1.0 if len(rows) >= R else 0.0
            if dones[t, e]:
                rows = []
    return win, wts


def gae_masked(rewards, values, boot, dones, gamma=0.99, lam=0.96, scale=1.0):
    """The worker's GAE per env column with a done mask: delta = r + g V' m - V, A = delta + g lam m A'; targets A + V, adv A / scale."""
    T = rewards.shape[0]
    m = 1.0 - np.asarray(dones, np.float64)
    run = np.zeros(rewards.shape[1:])
    vnext = np.asarray(boot, np.float64)
    adv = np.zeros(rewards.shape); tgt = np.zeros(rewards.shape)
    for t in reversed(range(T)):
        vt = np.asarray(values[t], np.float64)
        delta = np.asarray(rewards[t], np.float64) + gamma * vnext * m[t] - vt
        run = delta + gamma * lam * m[t] * run
        tgt[t] = run + vt
        adv[t] = run / scale
        vnext = vt
    return adv, tgt


def worker_update(params_flat, msp, msv, global_step, states, windows, choices, raw, rewards, boot, lr0, gamma=0.99, lam=0.96,
                  scale=1.0, clip=40.0):
    """TickerGatedTraderWorker.update (worker.py:241-294 + :478-489) on a list of recorded transitions: V of the recorded states,
    the bootstrap value appended, GAE (lfilter over reversed deltas), advantages / scale to the policy, targets to the value head,
    both train ops.  Returns the new params, ms vectors, global step and the gradients."""
    p = unflatten(params_flat)
    _, _, _, V = forward(p, states, windows, scale)
    v_all = np.concatenate([V, [boot]])
    adv, tgt = O.gae(np.asarray(rewards, np.float64)[:, None], V[:, None], np.array([boot]), gamma, lam)
    adv, tgt = adv[:, 0], tgt[:, 0]
    assert np.allclose(tgt - adv, v_all[:-1])
    (pl, vl, ent), gp, gv = grads(p, states, windows, choices, raw, adv / scale, tgt, None, 1.0, scale)
    out = apply_update(params_flat, flatten(gp), flatten(gv), msp, msv, global_step, lr0, clip)
    return out, flatten(gp), flatten(gv), (pl, vl, ent)
