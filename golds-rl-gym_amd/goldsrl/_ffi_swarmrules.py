"""ctypes binding of the feedback-rule baseline of the Swarm env (C ABI: include/goldsrl_swarmrules.h): every (env, rule) pair
plays a whole episode in one kernel launch, each step's action computed on the device from the positions the step before left.
swarm_rule_actions is the host form of the rule, device-free."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_episode import read_outputs, steps_and_trace

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t

# include/goldsrl_swarmrules.h: a dict of its own, as the header is a file of its own (tests/test_swarm_rules_header.py pins both)
SWARMRULES_SIGNATURES = {
    "grl_swarm_rules": (C.c_int, [_P, _P, _P, _I, _I, _I, _I]),
    "grl_swarm_rules_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}

RULE_FIELDS = ("cancel", "gain", "anchor", "off_x", "off_y", "radius")
N_LOCUSTS, N_AGENTS = 80, 10
MAX_RULES = 4096


def check_swarm_rules(rules):
    """rules as the (n_rules, 6) float64 array of (cancel, gain, anchor, off_x, off_y, radius) rows, or ValueError naming the
    offending rule and field: the checks of grl_swarm_rules, device-free."""
    r = np.asarray(rules, np.float64)
    if r.ndim != 2 or r.shape[1] != 6 or r.shape[0] < 1 or r.shape[0] > MAX_RULES:
        raise ValueError("rules must be (n_rules, 6) of (cancel, gain, anchor, off_x, off_y, radius) with 1..%d rows, got shape %s"
                         % (MAX_RULES, r.shape))
    for i, u in enumerate(r):
        for k, name in enumerate(RULE_FIELDS):
            if not np.isfinite(u[k]):
                raise ValueError("rule %d: %s is not finite" % (i, name))
        if u[2] != 0.0 and u[2] != 1.0:
            raise ValueError("rule %d: anchor must be 0 (the centroid) or 1 (the agent's nearest locust), got %r" % (i, float(u[2])))
    return np.ascontiguousarray(r)


def swarm_rule_offsets(rules):
    """The per-agent offset tables the device is handed: off[a] = (off_x + radius * cos(2 pi a / 10), off_y + radius * sin(2 pi a / 10)),
    float64, computed once on the host.  Returns (n_rules, 10, 2)."""
    r = check_swarm_rules(rules)
    ang = 2.0 * np.pi * np.arange(N_AGENTS, dtype=np.float64) / N_AGENTS
    off = np.empty((r.shape[0], N_AGENTS, 2), np.float64)
    off[:, :, 0] = r[:, 3:4] + r[:, 5:6] * np.cos(ang)[None]
    off[:, :, 1] = r[:, 4:5] + r[:, 5:6] * np.sin(ang)[None]
    return off


def swarm_rule_actions(x, xa, rule_row, offsets):
    """The host form of the rule (include/goldsrl_swarmrules.h), one IEEE float64 operation after the other -- the device's bits.
    x (..., 80, 2) and xa (..., 10, 2): the positions before the step; rule_row: (cancel, gain, anchor, ...) -- the first three
    numbers of a rule; offsets (10, 2): that rule's row of swarm_rule_offsets.  Returns the action rows (..., 10, 2) float64."""
    x, xa = np.asarray(x, np.float64), np.asarray(xa, np.float64)
    off = np.asarray(offsets, np.float64)
    cancel, gain, anchor = (np.float64(v) for v in tuple(rule_row)[:3])
    if anchor != 0.0 and anchor != 1.0:
        raise ValueError("anchor must be 0 or 1")
    ax_x, ax_y = xa[..., 0], xa[..., 1]                       # (..., 10)
    if anchor == 0.0:
        cx = np.zeros(x.shape[:-2], np.float64)
        cy = np.zeros(x.shape[:-2], np.float64)
        for j in range(N_LOCUSTS):                            # sequential, index order: the order is part of the contract
            cx = cx + x[..., j, 0]
            cy = cy + x[..., j, 1]
        cx = cx / 80.0
        cy = cy / 80.0
        cx = np.broadcast_to(cx[..., None], ax_x.shape)
        cy = np.broadcast_to(cy[..., None], ax_y.shape)
    else:
        qx = x[..., 0, 0][..., None]
        qy = x[..., 0, 1][..., None]
        dx = qx - ax_x
        dy = qy - ax_y
        sx = dx * dx
        sy = dy * dy
        best = sx + sy
        cx = np.broadcast_to(qx, ax_x.shape).copy()
        cy = np.broadcast_to(qy, ax_y.shape).copy()
        for j in range(1, N_LOCUSTS):
            qx = x[..., j, 0][..., None]
            qy = x[..., j, 1][..., None]
            dx = qx - ax_x
            dy = qy - ax_y
            sx = dx * dx
            sy = dy * dy
            d2 = sx + sy
            nearer = d2 < best                                # strict: the first index wins a tie
            best = np.where(nearer, d2, best)
            cx = np.where(nearer, qx, cx)
            cy = np.where(nearer, qy, cy)
    tx = cx + off[:, 0]
    ty = cy + off[:, 1]
    ex = tx - ax_x
    ey = ty - ax_y
    gx = gain * ex
    ax = gx - cancel
    ay = gain * ey
    qx = ax * ax
    qy = ay * ay
    s = qx + qy
    d = np.sqrt(s)
    clip = d >= 1.0
    safe = np.where(clip, d, 1.0)
    nx = ax / safe
    ny = ay / safe
    return np.stack([np.where(clip, nx, ax), np.where(clip, ny, ay)], axis=-1)


def swarm_rules(engine, rules, max_steps=None, keep_actions=False, trace_env=None):
    """Play every (env, rule) pair from the engine's CURRENT state (reset it first) for up to max_steps steps (default: the
    engine's max_episode_steps); the engine's state is left as it was.  rules: (n_rules, 6) rows (cancel, gain, anchor, off_x,
    off_y, radius).  A pair ends after the step whose reward is >= 0 or that reaches the engine's TimeLimit (finished = 1), or
    after max_steps.

    Returns rules and offsets as played, rewards (E, n_rules, T) float64, zero past the pair's length, totals (E, n_rules) =
    rewards.sum(-1), length (E, n_rules) int32, finished (E, n_rules) uint8; with keep_actions the action rows actions
    (E, n_rules, T, 10, 2); with trace_env the positions after every step of that env: trace_x (n_rules, T, 80, 2), trace_xa
    (n_rules, T, 10, 2)."""
    if engine.kind != _ffi.ENV_SWARM:
        raise ValueError("swarm_rules: the engine is not a Swarm engine")
    r = check_swarm_rules(rules)
    off = np.ascontiguousarray(swarm_rule_offsets(r))
    head = np.ascontiguousarray(r[:, :3])
    T, t_env = steps_and_trace(engine, "swarm_rules", max_steps, trace_env)
    n = r.shape[0]
    lib = _ffi.load_library(extra_signatures=SWARMRULES_SIGNATURES)
    engine._check(lib.grl_swarm_rules(engine.h, _ffi._ptr(head), _ffi._ptr(off), n, T, 1 if keep_actions else 0, t_env))
    pair = [("rewards", np.float64, (T,)), ("length", np.int32, ()), ("finished", np.uint8, ())]
    if keep_actions:
        pair += [("actions", np.float64, (T, N_AGENTS, 2))]
    out = {"rules": r, "offsets": off}
    out.update(read_outputs(engine, lib.grl_swarm_rules_read, pair, (engine.E, n)))
    if t_env >= 0:
        out.update(read_outputs(engine, lib.grl_swarm_rules_read,
                                (("trace_x", np.float64, (N_LOCUSTS, 2)), ("trace_xa", np.float64, (N_AGENTS, 2))), (n, T)))
    out["totals"] = out["rewards"].sum(-1)
    return out
