"""ctypes binding of the receding-horizon rule planner of the Swarm env (C ABI: include/goldsrl_swarmplan.h): at every decision each
env plays every rule of the table `horizon` steps ahead, commits the best for `replan` steps and plans again, the whole planned
episode enqueued in one call.  swarm_plan_host is the same computation composed on the host from grl_swarm_rules and
grl_swarm_step_f64: the documented slow path, and the oracle the device is held to."""
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi_episode import read_outputs, steps_and_trace
from ._ffi_swarmrules import N_AGENTS, N_LOCUSTS, check_swarm_rules, swarm_rule_offsets, swarm_rules

_P, _I, _SZ = C.c_void_p, C.c_int32, C.c_size_t

# include/goldsrl_swarmplan.h: a dict of its own, as the header is a file of its own (tests/test_swarm_plan_header.py pins both)
SWARMPLAN_SIGNATURES = {
    "grl_swarm_plan": (C.c_int, [_P, _P, _P, _I, _I, _I, _I, _I, _I]),
    "grl_swarm_plan_read": (C.c_int, [_P, C.c_char_p, _P, _SZ]),
}


def _check_plan(engine, fn_name, rules, horizon, replan, max_steps, trace_env):
    if engine.kind != _ffi.ENV_SWARM:
        raise ValueError("%s: the engine is not a Swarm engine" % fn_name)
    r = check_swarm_rules(rules)
    H, K = int(horizon), int(replan)
    if H < 1 or K < 1 or K > H:
        raise ValueError("%s: 1 <= replan <= horizon is required, got horizon %d, replan %d" % (fn_name, H, K))
    T, t_env = steps_and_trace(engine, fn_name, max_steps, trace_env)
    return r, H, K, T, t_env, (T + K - 1) // K


def swarm_plan(engine, rules, horizon, replan, max_steps=None, keep_actions=False, trace_env=None):
    """Plan every env from the engine's CURRENT state (reset it first) for up to max_steps steps (default: the engine's
    max_episode_steps); the engine's state is left as it was.  rules: (n_rules, 6) rows (cancel, gain, anchor, off_x, off_y, radius).
    At each of the D = ceil(max_steps / replan) decisions every rule plays min(horizon, steps to the TimeLimit) steps ahead, the
    first rule with the largest float64 sum of rewards is committed for replan steps.  An env ends after the step whose reward is
    >= 0 or that reaches the engine's TimeLimit (finished = 1), or after max_steps.

    Returns rules and offsets as played, rewards (E, T) float64, zero past the env's length, totals (E,) = rewards.sum(-1), length
    (E,) int32, finished (E,) uint8, choices (E, D) int32, -1 past the env's last decision, scores (E, D, n_rules) float64, zero past
    it; with keep_actions the committed action rows actions (E, T, 10, 2); with trace_env the positions after every committed step
    of that env: trace_x (T, 80, 2), trace_xa (T, 10, 2)."""
    r, H, K, T, t_env, D = _check_plan(engine, "swarm_plan", rules, horizon, replan, max_steps, trace_env)
    off = np.ascontiguousarray(swarm_rule_offsets(r))
    head = np.ascontiguousarray(r[:, :3])
    n = r.shape[0]
    lib = _ffi.load_library(extra_signatures=SWARMPLAN_SIGNATURES)
    engine._check(lib.grl_swarm_plan(engine.h, _ffi._ptr(head), _ffi._ptr(off), n, H, K, T, 1 if keep_actions else 0, t_env))
    per_env = [("rewards", np.float64, (T,)), ("length", np.int32, ()), ("finished", np.uint8, ()), ("choices", np.int32, (D,)),
               ("scores", np.float64, (D, n))]
    if keep_actions:
        per_env += [("actions", np.float64, (T, N_AGENTS, 2))]
    out = {"rules": r, "offsets": off}
    out.update(read_outputs(engine, lib.grl_swarm_plan_read, per_env, (engine.E,)))
    if t_env >= 0:
        out.update(read_outputs(engine, lib.grl_swarm_plan_read,
                                (("trace_x", np.float64, (N_LOCUSTS, 2)), ("trace_xa", np.float64, (N_AGENTS, 2))), (T,)))
    out["totals"] = out["rewards"].sum(-1)
    return out


def swarm_plan_host(engine, rules, horizon, replan, max_steps=None, keep_actions=False, trace_env=None):
    """swarm_plan composed on the host, several round trips per decision: grl_swarm_rules(max_steps=horizon) from the engine's
    current state, the scores as a Python loop of float64 adds over t < length, np.argmax, and replan calls of
    grl_swarm_step_f64 with the chosen rule's kept action rows.  Same arguments and outputs as swarm_plan.  It ADVANCES the engine
    (and the engine auto-resets an env whose episode ends; such an env takes no further part here and is stepped with zero
    actions; the trace row of the step that ends the traced env's episode stays zero, as its positions are gone by then)."""
    r, H, K, T, t_env, D = _check_plan(engine, "swarm_plan_host", rules, horizon, replan, max_steps, trace_env)
    E, n = engine.E, r.shape[0]
    out = {"rules": r, "offsets": np.ascontiguousarray(swarm_rule_offsets(r)),
           "rewards": np.zeros((E, T), np.float64), "length": np.zeros(E, np.int32), "finished": np.zeros(E, np.uint8),
           "choices": np.full((E, D), -1, np.int32), "scores": np.zeros((E, D, n), np.float64)}
    if keep_actions:
        out["actions"] = np.zeros((E, T, N_AGENTS, 2), np.float64)
    if t_env >= 0:
        out["trace_x"] = np.zeros((T, N_LOCUSTS, 2), np.float64)
        out["trace_xa"] = np.zeros((T, N_AGENTS, 2), np.float64)
    alive = np.ones(E, bool)
    t = 0
    for d in range(D):
        if not alive.any():
            break
        look = swarm_rules(engine, r, H, keep_actions=True)
        for e in np.flatnonzero(alive):
            for i in range(n):
                s = np.float64(0.0)
                for k in range(int(look["length"][e, i])):
                    s = s + look["rewards"][e, i, k]
                out["scores"][e, d, i] = s
            out["choices"][e, d] = int(np.argmax(out["scores"][e, d]))
        for k in range(min(K, T - t)):
            act = np.zeros((E, N_AGENTS, 2), np.float64)
            for e in np.flatnonzero(alive):
                act[e] = look["actions"][e, out["choices"][e, d], k]
            engine.swarm_step_f64(act)
            rew, done = engine.read("reward_f64"), engine.read("done")
            if t_env >= 0 and alive[t_env]:
                # the env's positions after the step: its own unless the step ended the episode and the engine reset it
                if not done[t_env]:
                    out["trace_x"][t] = engine.get_state("SWARM_X")[t_env]
                    out["trace_xa"][t] = engine.get_state("SWARM_XA")[t_env]
            for e in np.flatnonzero(alive):
                out["rewards"][e, t] = rew[e]
                if keep_actions:
                    out["actions"][e, t] = act[e]
                out["length"][e] = t + 1
                if done[e]:
                    out["finished"][e] = 1
                    alive[e] = False
            t += 1
    out["totals"] = out["rewards"].sum(-1)
    return out
