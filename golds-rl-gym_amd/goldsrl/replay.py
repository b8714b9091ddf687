"""Replay recorded Swarm episodes on the device and draw them (reference scripts/make_swarm_gif.py).

`SwarmPolicyMonitor` keeps the best eval episode's actions in swarm-eval.json ({'score', 'actions'}); the reference steps them
through `Swarm-eval-v0` one `env.step` at a time and scatter-plots every state with matplotlib.  Here the whole episode is one
kernel launch (include/goldsrl_replay.h), and the frames are drawn with numpy alone: `frames` restates the script's plot
(window x in (0, 9), y in (0, 4), locusts shaded by index with cmap='Reds', agents in dodgerblue on top) as filled squares on a
white canvas.  matplotlib is not used."""
import json

import numpy as np

# matplotlib's 'Reds' is the ColorBrewer 9-class sequential Reds scheme, interpolated linearly; 'dodgerblue' is the CSS colour
_REDS = np.array([(255, 245, 240), (254, 224, 210), (252, 187, 161), (252, 146, 114), (251, 106, 74), (239, 59, 44),
                  (203, 24, 29), (165, 15, 21), (103, 0, 13)], np.float64)
DODGERBLUE = (30, 144, 255)
BACKGROUND = (255, 255, 255)


def load_actions(path):
    """swarm-eval.json as SwarmPolicyMonitor._save_actions writes it -> (score, actions (T, 10, 2) float64)"""
    with open(path) as f:
        record = json.load(f)
    actions = np.asarray(record["actions"], np.float64)
    if actions.ndim != 3 or actions.shape[1:] != (10, 2):
        raise ValueError("%s: 'actions' must be (T, 10, 2), got %s" % (path, actions.shape))
    return float(record["score"]), actions


def episode_totals(rewards, length):
    """np.sum over each pair's first `length` rewards -- the monitor's total_reward, in numpy's own summation order (a sum over
    the zero tail as well would pair the terms differently)."""
    rewards, length = np.asarray(rewards), np.asarray(length)
    flat = rewards.reshape(-1, rewards.shape[-1])
    return np.array([np.sum(row[:n]) for row, n in zip(flat, length.reshape(-1))], np.float64).reshape(length.shape)


class SwarmReplay(object):
    """Scripted episodes on a Swarm engine, or on the engine of a SwarmEnv facade, from its CURRENT state (reset it first); the
    state is left as it was."""

    def __init__(self, env_or_engine):
        self.eng = getattr(env_or_engine, "_eng", env_or_engine)

    def play(self, actions, seq_len=None, trace_env=None, dtype=None):
        """actions: (T, 10, 2) -- one script --, (n_seq, T, 10, 2), or (E, n_seq, T, 10, 2) rows of each env's own; float64 rows
        are stepped as SwarmEnv.step steps a direct caller's, float32 rows as the worker's shared array is (quirk Q7); `dtype`
        converts first.  Returns rewards (E, n_seq, T), totals, length and finished (E, n_seq), and with trace_env the positions
        after every step of that env: x_traj (n_seq, T, 80, 2) and xa_traj (n_seq, T, 10, 2), zero past the pair's length."""
        from . import _ffi_replay
        a = np.asarray(actions)
        if dtype is not None:
            a = a.astype(dtype)
        if a.ndim == 3:
            a = a[None]
        out = _ffi_replay.swarm_replay(self.eng, a, seq_len, -1 if trace_env is None else trace_env)
        res = {"rewards": out["rewards"], "length": out["length"], "finished": out["finished"],
               "totals": episode_totals(out["rewards"], out["length"])}
        if "trace_x" in out:
            res["x_traj"], res["xa_traj"] = out["trace_x"], out["trace_xa"]
        return res


def reds(n):
    """cmap='Reds' over np.arange(n) (make_swarm_gif.py:46): (n, 3) uint8"""
    u = np.linspace(0.0, 1.0, n) * (len(_REDS) - 1) if n > 1 else np.zeros(1)
    lo = np.minimum(u.astype(np.int64), len(_REDS) - 2)
    w = (u - lo)[:, None]
    return np.rint(_REDS[lo] * (1.0 - w) + _REDS[lo + 1] * w).astype(np.uint8)


def _paint(canvas, pts, colour, half, xlim, ylim):
    """One point per frame: pts (T, 2) -> a (2*half+1)-pixel square of `colour` around its pixel, cut at the canvas' edge.  A point
    outside the window is dropped, not clamped."""
    T, height, width = canvas.shape[:3]
    px, py = pts[:, 0], pts[:, 1]
    with np.errstate(invalid="ignore"):
        inside = (px >= xlim[0]) & (px < xlim[1]) & (py >= ylim[0]) & (py < ylim[1])
    t = np.flatnonzero(inside)
    if t.size == 0:
        return
    col = np.minimum(((px[t] - xlim[0]) / (xlim[1] - xlim[0]) * width).astype(np.int64), width - 1)
    row = height - 1 - np.minimum(((py[t] - ylim[0]) / (ylim[1] - ylim[0]) * height).astype(np.int64), height - 1)      # y points up
    for dr in range(-half, half + 1):
        for dc in range(-half, half + 1):
            r, c = row + dr, col + dc
            ok = (r >= 0) & (r < height) & (c >= 0) & (c < width)
            canvas[t[ok], r[ok], c[ok]] = colour


def frames(x_traj, xa_traj, width=720, height=320, xlim=(0, 9), ylim=(0, 4), locust_half=2, agent_half=3):
    """make_plot (make_swarm_gif.py:44-51) per step, in numpy: x_traj (T, 80, 2), xa_traj (T, 10, 2) -> (T, height, width, 3) uint8.
    The window is the reference's; y points up; a locust is a (2*locust_half+1)-pixel square shaded red by its index, an agent a
    (2*agent_half+1)-pixel dodgerblue square drawn over the locusts; a point outside the window is not drawn."""
    x, xa = np.asarray(x_traj, np.float64), np.asarray(xa_traj, np.float64)
    if x.ndim != 3 or xa.ndim != 3 or x.shape[2] != 2 or xa.shape[2] != 2 or x.shape[0] != xa.shape[0]:
        raise ValueError("frames: expected (T, n, 2) and (T, m, 2), got %s and %s" % (x.shape, xa.shape))
    canvas = np.empty((x.shape[0], int(height), int(width), 3), np.uint8)
    canvas[:] = BACKGROUND
    shades = reds(x.shape[1])
    for i in range(x.shape[1]):
        _paint(canvas, x[:, i], shades[i], int(locust_half), xlim, ylim)
    for i in range(xa.shape[1]):
        _paint(canvas, xa[:, i], DODGERBLUE, int(agent_half), xlim, ylim)
    return canvas


def save_gif(frames, path, interval_ms=50):
    """Write (T, H, W, 3) uint8 frames as a looping GIF (FuncAnimation's interval=50, make_swarm_gif.py:81).  Needs PIL."""
    try:
        from PIL import Image
    except ImportError:
        raise RuntimeError("save_gif needs PIL, which cannot be imported; keep the frames with np.save(path, frames) instead")
    images = [Image.fromarray(np.ascontiguousarray(f, np.uint8), "RGB") for f in frames]
    if not images:
        raise ValueError("save_gif: no frames")
    images[0].save(path, format="GIF", save_all=True, append_images=images[1:], duration=int(interval_ms), loop=0)
