"""Helpers of tests/test_gpu_field_rollout.py: the geometries, biased parameters, engines and nets of the field policy on Swarm,
the float64 oracle's samples from a recorded rollout, and the step-by-step replay of a rollout on a twin engine."""
import numpy as np

import _async_scenarios as SC
from oracle import nets as NN
from oracle import oracle as O

GEOMS = {
    "G8_L2_F3": dict(height=8, width=8, channels=2, filters=3, conv_layers=2, num_actions=2),
    "G20_L2_F5": dict(height=20, width=20, channels=2, filters=5, conv_layers=2, num_actions=2),
    "G12_L1_F4": dict(height=12, width=12, channels=2, filters=4, conv_layers=1, num_actions=2),
}
SCALE, BETA, GAMMA = 10.0, 0.02, 0.99
SEED, OFFSET = 77, 3            # generator seed and env_id_offset of the engines
E, T, CAP, COUNTER0 = 5, 4, 3, 1000
ACT_RTOL, ACT_ATOL = 1e-6, 1e-7      # tests/test_gpu_conv_rollout_replay.py
OBS = (("lb", "locust_bins"), ("ab", "agent_bins"), ("ps", "positions"))

_params = {}


def params(geom):
    """glorot weights with small random NON-ZERO biases (so that no pre-activation is exactly zero): (dict float64, shapes, flat float32)"""
    if geom not in _params:
        from goldsrl import _ffi_field
        g = GEOMS[geom]
        shapes = NN.field_param_shapes(**g)
        rng = np.random.RandomState(11)
        p = NN.unflatten_params(_ffi_field.glorot_uniform_flat(3, **g).astype(np.float64), shapes)
        for k in p:
            if k.endswith("_b"):
                b = rng.normal(size=p[k].shape) * 0.05
                p[k] = np.where(np.abs(b) < 1e-3, 1e-3, b)
        flat = NN.flatten_params(p, shapes).astype(np.float32)
        _params[geom] = (NN.unflatten_params(flat.astype(np.float64), shapes), shapes, flat)
    return _params[geom]


def set_fused(monkeypatch, fused):
    """before the net is created: the switch is read at the net's first rollout call"""
    monkeypatch.delenv("GRL_FIELD_HEADT", raising=False)
    if fused:
        monkeypatch.delenv("GRL_FIELD_FUSED", raising=False)
    else:
        monkeypatch.setenv("GRL_FIELD_FUSED", "off")


def engine(geom, n_envs=E, offset=OFFSET, cap=CAP, elapsed=None, seed=SEED):
    from goldsrl import _ffi
    eng = _ffi.Engine(_ffi.ENV_SWARM, n_envs, seed=seed, env_id_offset=offset, max_episode_steps=cap, grid_size=GEOMS[geom]["height"])
    eng.reset()
    if elapsed is not None:
        eng.set_state("ELAPSED", elapsed)
    eng.episodes_enable()
    return eng


def net(eng, geom, max_samples=64, clip_norm=40.0, flat=None, counter=None):
    from goldsrl import _ffi_field
    n = _ffi_field.FieldNet(eng, max_samples=max_samples, scale=SCALE, entropy_beta=BETA, clip_norm=clip_norm, **GEOMS[geom])
    n.set_params(params(geom)[2] if flat is None else flat)
    n.rollout_bind(GAMMA)
    if counter is not None:
        n.set_action_counter(counter)
    return n


def share_cells(eng):
    """Agent 0 of envs 0, 1 and 2 onto agent 0 of env 0's offset from its env's swarm, and one agent and one locust of env 1 outside
    the box (y < 0): the same state on every engine it is applied to.  Observes."""
    x, xa = eng.get_state("SWARM_X"), eng.get_state("SWARM_XA")
    rel = xa[0, 0] - np.array([np.mean(np.vstack([x[0], xa[0]])[:, 0]), 0.0])
    for e in range(1, min(3, eng.E)):
        xa[e, 0] = rel + np.array([np.mean(np.vstack([x[e], xa[e]])[:, 0]), 0.0])
    if eng.E > 1:
        xa[1, 9, 1] = -0.7
        x[1, 5, 1] = -0.3
    eng.set_state("SWARM_X", x)
    eng.set_state("SWARM_XA", xa)
    eng.observe()


def field_inputs(lb, ab, ps, G):
    """the oracle's (n * 10, G, G, 2) float64 states -- an env's image repeated for its ten agents -- and (n * 10, 2) positions"""
    from goldsrl.agents.state_processors import swarm_field_inputs
    states, pos = swarm_field_inputs(lb, ab, ps, G)
    return np.repeat(states, 10, axis=0), pos.reshape(-1, 2)


def read_rollout(n, steps):
    ro = {k: n.read_rollout(name, steps) for k, name in OBS}
    for k in ("actions", "env_actions", "mu", "sigma", "values", "rewards", "dones", "y", "adv"):
        ro[k] = n.read_rollout(k, steps)
    ro["boot"] = n.read_rollout("boot")
    return ro


def replay(ro, twin, tnet, layout, counter0, schedule, figures):
    """Steps the twin with the recorded env_actions and compares; returns None or the first mismatch (t, field)."""
    steps, n_envs = ro["dones"].shape
    env, agent = np.arange(n_envs), np.arange(10)
    for t in range(steps):
        for k, name in OBS:
            if not np.array_equal(twin.read(name), ro[k][t]):
                return t, name
        pred = tnet.predict_swarm()
        for k, want in (("mu", pred["mu"]), ("sigma", pred["sigma"]), ("values", pred["vs"])):
            if not np.array_equal(ro[k][t], want):
                return t, k
        e0, e1 = O.normal_pair(O.rng_block(SEED, env[:, None] + OFFSET, counter0 + t, 16, agent[None]))
        eps = np.stack([e0, e1], axis=-1).reshape(n_envs * 10, 2)
        want = pred["mu"].astype(np.float64) + pred["sigma"].astype(np.float64) * eps
        err, bound = np.abs(ro["actions"][t] - want), ACT_ATOL + ACT_RTOL * np.abs(want)
        figures["action_err_of_bound"] = max(figures.get("action_err_of_bound", 0.0), float((err / bound).max()))
        if not (err <= bound).all():
            return t, "actions"
        if not np.array_equal(ro["env_actions"][t], twin.transform_actions(ro["actions"][t])):
            return t, "env_actions"
        twin.step(ro["env_actions"][t].reshape(n_envs, 10, 2))
        rew = twin.read("reward")
        if layout == 0:
            ok = np.array_equal(ro["rewards"][t].reshape(n_envs, 10), np.repeat(rew[:, None], 10, axis=1))
        else:
            ok = np.array_equal(ro["rewards"][t, :n_envs], rew) and not ro["rewards"][t, n_envs:].any()
        if not ok:
            return t, "rewards"
        if not np.array_equal(twin.read("done"), ro["dones"][t]):
            return t, "dones"
        if not np.array_equal(ro["dones"][t].astype(bool), schedule[t]):
            return t, "dones_schedule"
    if not np.array_equal(tnet.predict_swarm()["vs"], ro["boot"]):
        return steps, "boot"
    return None


_scenario = {}


def scenario(geom, fused, layout, monkeypatch):
    """The rollout of tests 3 and 5 -- 5 envs, 4 steps, TimeLimit(3) with staggered counters, three agents moved onto one cell,
    action counter from 1000 -- with its engine, net and twin left open: computed once per (geometry, path, layout)."""
    key = (geom, fused, layout)
    if key not in _scenario:
        set_fused(monkeypatch, fused)
        el = SC.staggered_elapsed(E, CAP)
        eng, twin = engine(geom, elapsed=el), engine(geom, elapsed=el)
        share_cells(eng); share_cells(twin)
        n, tn = net(eng, geom, counter=COUNTER0), net(twin, geom)
        n.rollout(T, layout)
        eng.wait()
        _scenario[key] = dict(eng=eng, twin=twin, net=n, tnet=tn, ro=read_rollout(n, T), schedule=SC.timelimit_dones(el, T, CAP))
    return _scenario[key]


def oracle_samples(ro, geom):
    """states (T*B,G,G,2) float64, positions, actions, adv, y of a recorded rollout in (t, env, agent) order"""
    G = GEOMS[geom]["height"]
    steps = ro["dones"].shape[0]
    parts = [field_inputs(ro["lb"][t], ro["ab"][t], ro["ps"][t], G) for t in range(steps)]
    states = np.concatenate([s for s, _ in parts]).astype(np.float64)
    pos = np.concatenate([p for _, p in parts])
    return states, pos, ro["actions"].reshape(-1, 2), ro["adv"].reshape(-1), ro["y"].reshape(-1)


def oracle_grads(ro, geom):
    p, shapes, _ = params(geom)
    states, pos, act, adv, y = oracle_samples(ro, geom)
    loss, pl, cl, g, _ = NN.field_loss_and_grads(p, states, pos, act.astype(np.float64), adv.astype(np.float64), y.astype(np.float64), BETA, SCALE,
                                                 GEOMS[geom]["conv_layers"])
    return (loss, pl, cl), g


def block_errors(flat_grads, g, shapes):
    """per parameter block: max |got - want| over the block's largest |want|"""
    got = NN.unflatten_params(np.asarray(flat_grads, np.float64), shapes)
    return {name: float(np.abs(got[name] - g[name]).max() / (np.abs(g[name]).max() + 1e-12)) for name, _ in shapes}
