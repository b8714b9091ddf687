"""Scenarios in which the envs of one batch end their episodes on DIFFERENT steps, shared by tests/test_async_scenarios.py
(CPU: the scenarios really are asynchronous, oracle alone), tests/test_gpu_async_dones.py (GPU: the kernels against them) and
tests/test_gpu_conv_rollout_replay.py (GPU: the conv rollout's chunks and lanes, REPLAY_* and chunk_end_stats below).

Two ways to desynchronise a batch:
  * staggered TimeLimit -- after reset(), ELAPSED is set to (7 * env + env // 64) % CAP, so with CAP = 9 every wave of 64 envs
    ends about 7 scattered envs on every step and the set differs from wave to wave;
  * TradeAR1 depletion -- a starting balance just above MIN_CASH = 1 and noisy prices: `assets < 1` ends envs one by one.
"""
import numpy as np

from oracle import oracle as O

E, T, CAP, WAVE = 200, 20, 9, 64          # three waves and a partial one of 8 lanes
SWARM_E = 70
RESET_IDX = [197, 3, 64, 63, 130, 5, 199]
GEN_SEED, GEN_OFFSET = 77, 1000           # device generator: engine seed and env_id_offset

# n_assets -> engine kwargs of the depletion configuration, RandomState seed of the fixed actions / injected normals
TRADE_DEPLETION = {
    2: dict(trade_starting_balance=1.05, trade_std_p=0.3),
    3: dict(trade_starting_balance=1.05, trade_std_p=0.3),
    16: dict(trade_starting_balance=1.02, trade_std_p=0.5),
}
TRADE_INPUT_SEED = {2: 1, 3: 1, 16: 1}
# Rollouts whose actions the device net chooses (it trades less than tanh(N(0,1)) does): the GPU test asserts >= E / 4 depletion
# dones and a mixed share >= 0.25 on the recorded dones.  n = 3 at 1.05 gave 43 depletion dones in 20 steps, so its starting
# balance sits closer to MIN_CASH.
TRADE_POLICY_DEPLETION = {
    2: dict(trade_starting_balance=1.05, trade_std_p=0.3),
    3: dict(trade_starting_balance=1.02, trade_std_p=0.3),
    16: dict(trade_starting_balance=1.02, trade_std_p=0.5),
}
MIN_GAP = 1e-6                            # condition 3: the oracle's assets never come closer to MIN_CASH than this

# The conv rollout replayed step by step (tests/test_gpu_conv_rollout_replay.py): 37 Swarm envs in chunks of 7 envs (70 samples) are
# six chunks of 7, 7, 7, 7, 7 and 2 envs at bases 0, 7, 14, 21, 28, 35 -- four bases are no multiple of the step kernel's 4 envs per
# block, the last chunk is smaller than one workgroup, and over four lanes chunks 4 and 5 share lanes 0 and 1 with chunks 0 and 1.
REPLAY_E, REPLAY_CHUNK_SAMPLES, REPLAY_LANES = 37, 70, 4
REPLAY_CHUNK_ENVS = REPLAY_CHUNK_SAMPLES // 10
REPLAY_COUNTER0 = 1000                    # action counter the first rollout starts at
REPLAY_ROLLOUTS, REPLAY_GRAD_T = 2, 4     # two chained rollouts of T steps, then one of 4 steps for the gradient leg
REPLAY_NEG_ENV = 23                       # negative control: the twin's ELAPSED is off by one for this env only


def staggered_elapsed(n_env, cap=CAP):
    env = np.arange(n_env)
    return ((7 * env + env // WAVE) % cap).astype(np.int32)


def timelimit_dones(elapsed0, steps, cap=CAP):
    """(steps, E) bool: TimeLimit(cap) ends of envs whose counter started at elapsed0 (the counter restarts at 0 behind a done,
    so the same expression holds after the first end)."""
    t = np.arange(steps)[:, None]
    return (elapsed0[None].astype(np.int64) + t + 1) % cap == 0


def mixed_share(dones, wave=WAVE):
    """Share of (step, wave) pairs whose done mask is mixed: some lanes done, not all of the lanes the wave has."""
    dones = np.asarray(dones).astype(bool)
    steps, n_env = dones.shape
    mixed = total = 0
    for w0 in range(0, n_env, wave):
        d = dones[:, w0:w0 + wave]
        s = d.sum(axis=1)
        mixed += int(((s > 0) & (s < d.shape[1])).sum())
        total += steps
    return mixed / total


def chunk_end_stats(dones, chunk_envs, lanes):
    """What a rollout that steps its envs in chunks of chunk_envs, chunk c on lane c % lanes, sees of a (steps, E) done mask:
    mixed      per FULL chunk, the share of steps on which some of its envs are done and not all
    per_step   ends per step, per_env  ends per env
    shared     number of steps on which two chunks of one lane (c and c + lanes) both hold an end"""
    dones = np.asarray(dones).astype(bool)
    steps, n_env = dones.shape
    bases = list(range(0, n_env, chunk_envs))
    per_chunk = np.stack([dones[:, b:b + chunk_envs].sum(axis=1) for b in bases], axis=1)      # (steps, chunks)
    full = [c for c, b in enumerate(bases) if b + chunk_envs <= n_env]
    mixed = [float(((per_chunk[:, c] > 0) & (per_chunk[:, c] < chunk_envs)).mean()) for c in full]
    held = per_chunk > 0
    shared = np.zeros(steps, bool)
    for c in range(len(bases) - lanes):
        shared |= held[:, c] & held[:, c + lanes]
    return dict(mixed=mixed, per_step=dones.sum(axis=1), per_env=dones.sum(axis=0), shared=int(shared.sum()))


def trade_inputs(n, seed, n_env=E, steps=T):
    """Fixed actions tanh(N(0,1)) and injected normals, both rounded to float32: (steps, E, n) each."""
    rng = np.random.RandomState(seed)
    acts = np.empty((steps, n_env, n), np.float32)
    nrm = np.empty((steps, n_env, n), np.float32)
    for t in range(steps):
        acts[t] = np.tanh(rng.normal(size=(n_env, n))).astype(np.float32)
        nrm[t] = rng.normal(size=(n_env, n)).astype(np.float32)
    return acts, nrm


def trade_generator_normals(seed, env_off, n_env, steps, n, nstep0=0):
    """The device price generator's draws: asset a of env e at the env's nstep-th step since CREATION (the counter runs on
    across resets) is normal number a % 2 of block (seed, e + env_off, episode 0, stream 12, nstep * pairs + a // 2),
    pairs = (n + 1) // 2.  (steps, E, n) float64."""
    pairs = (n + 1) // 2
    a = np.arange(n)
    nstep = nstep0 + np.arange(steps)
    ctr = nstep[:, None, None] * pairs + (a // 2)[None, None, :]
    env = (np.arange(n_env) + env_off)[None, :, None]
    n0, n1 = O.normal_pair(O.rng_block(seed, env, 0, 12, ctr))
    return np.where((a % 2 == 0)[None, None, :], n0, n1)


def trade_reset_obs(n_env, n, start):
    return np.concatenate([np.full((n_env, 1), start), np.zeros((n_env, n)), np.ones((n_env, n))], axis=1)


def trade_oracle(n, start, std_p, actions, normals, elapsed0=None, cap=0):
    """O.trade_step plus the worker's per-env auto-reset (emulator_runner.py:50-52) over actions/normals (steps, E, n).
    An env is done when it depletes or, with cap > 0, when its TimeLimit counter reaches cap.  Returns a dict:
    obs (steps, E, 1+2n) -- the RESET observation behind a done (quirk Q6) --, reward, done, own_done (steps, E), gap =
    min |assets' - 1| over the trajectory, and the final account (cash, assets, q, p, elapsed, episodes)."""
    steps, n_env = actions.shape[:2]
    std_e = O.trade_std_e(std_p)
    cash, assets = np.full(n_env, float(start)), np.full(n_env, float(start))
    q, p = np.zeros((n_env, n)), np.ones((n_env, n))
    elapsed = np.zeros(n_env, np.int64) if elapsed0 is None else np.asarray(elapsed0, np.int64).copy()
    episodes = np.zeros(n_env, np.int64)
    out = dict(obs=np.empty((steps, n_env, 1 + 2 * n)), reward=np.empty((steps, n_env)), done=np.zeros((steps, n_env), bool),
               own_done=np.zeros((steps, n_env), bool))
    gap = np.inf
    robs = trade_reset_obs(n_env, n, start)
    for t in range(steps):
        cash, assets, q, p, obs, rew, own = O.trade_step(cash, assets, q, p, actions[t].astype(np.float64),
                                                         np.asarray(normals[t], np.float64), std_e)
        gap = min(gap, float(np.abs(assets - 1.0).min()))
        elapsed = elapsed + 1
        done = own | ((elapsed >= cap) if cap > 0 else False)
        cash = np.where(done, start, cash); assets = np.where(done, start, assets)
        q = np.where(done[:, None], 0.0, q); p = np.where(done[:, None], 1.0, p)
        elapsed = np.where(done, 0, elapsed); episodes = episodes + done
        out["obs"][t] = np.where(done[:, None], robs, obs)
        out["reward"][t], out["done"][t], out["own_done"][t] = rew, done, own
    out.update(gap=gap, cash=cash, assets=assets, q=q, p=p, elapsed=elapsed, episodes=episodes)
    return out


# ------------------------------------------------------------------------------------------ device generator restatements
def solow_reset_z(seed, env_global, episode, p, sigma=0.1):
    """z after a Solow reset: lag i is normal i % 2 of block (seed, env, episode, RS_SOLOW_Z0 = 8, i // 2), times sigma in float64,
    rounded to float32.  env_global, episode: (N,) -> (N, p) float32."""
    i = np.arange(p)
    n0, n1 = O.normal_pair(O.rng_block(seed, np.asarray(env_global)[:, None], np.asarray(episode)[:, None], 8, (i // 2)[None]))
    return (np.where((i % 2 == 0)[None], n0, n1) * sigma).astype(np.float32)


def solow_reset_tape(seed, env_global, episode, tape_len, sigma=0.1):
    """The shock tape drawn at a Solow reset (stream RS_SOLOW_TAPE = 9): (N, tape_len) float32."""
    n0, n1 = O.normal_pair(O.rng_block(seed, np.asarray(env_global)[:, None], np.asarray(episode)[:, None], 9,
                                       np.arange(tape_len // 2)[None]))
    return (np.stack([n0, n1], axis=-1).reshape(len(env_global), tape_len) * sigma).astype(np.float32)


def swarm_reset_state(seed, env_global, episode):
    """O.swarm_burn_in of the oracle generator's draws: x (N,80,2), xa (N,10,2), pnoise row 10 (N,80,2), anoise row 10 (N,10,2)."""
    env = np.asarray(env_global)[:, None]
    ep = np.asarray(episode)[:, None]
    N = len(env)
    x0 = np.stack(O.u01_pair(O.rng_block(seed, env, ep, 0, np.arange(80)[None])), axis=-1)
    xa0 = np.stack(O.u01_pair(O.rng_block(seed, env, ep, 1, np.arange(10)[None])), axis=-1)
    ra = np.stack(O.normal_pair(O.rng_block(seed, env, ep, 2, np.arange(100)[None])), axis=-1).reshape(N, 10, 10, 2)
    an = np.stack(O.normal_pair(O.rng_block(seed, env, ep, 3, np.arange(110)[None])), axis=-1).reshape(N, 11, 10, 2)
    pn = np.stack(O.normal_pair(O.rng_block(seed, env, ep, 4, np.arange(880)[None])), axis=-1).reshape(N, 11, 80, 2)
    x, xa = O.swarm_burn_in(x0, xa0, ra, an, pn)
    return x, xa, pn[:, 10], an[:, 10]


def ticker_reset_start(seed, env_global, episode, rows):
    """Window start drawn at a Ticker reset (stream RS_TICKER_START = 16): int(u0 * (rows - 1024 + 1))."""
    u0 = O.u01_pair(O.rng_block(seed, np.asarray(env_global), np.asarray(episode), 16, 0))[0]
    return np.clip((u0 * float(rows - 1024 + 1)).astype(np.int64), 0, rows - 1024)
