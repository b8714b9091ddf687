"""CPU: goldsrl/replay.py without a device -- frames() paints exactly the pixels the window maps a point to (y up, points outside
dropped, agents over locusts), save_gif() writes what PIL reads back, load_actions() reads SwarmPolicyMonitor._save_actions's file."""
import json

import numpy as np
import pytest

from goldsrl import replay

W, H = 720, 320        # 80 pixels per unit in both directions over the reference's window (0, 9) x (0, 4)


def _only(x, xa):
    return replay.frames(np.asarray(x, np.float64).reshape(1, -1, 2), np.asarray(xa, np.float64).reshape(1, -1, 2))


def _block(frame, colour):
    rows, cols = np.nonzero((frame == np.asarray(colour, np.uint8)).all(axis=2))
    return set(zip(rows.tolist(), cols.tolist()))


def test_shape_dtype_and_background():
    f = replay.frames(np.full((3, 80, 2), -1.0), np.full((3, 10, 2), -1.0))
    assert f.shape == (3, H, W, 3) and f.dtype == np.uint8
    assert (f == 255).all()                      # every point is outside the window: nothing is painted
    g = replay.frames(np.zeros((2, 4, 2)), np.zeros((2, 1, 2)), width=90, height=40)
    assert g.shape == (2, 40, 90, 3)


def test_one_locust_paints_its_block_with_y_flipped():
    # (2.5, 1.0): column floor(2.5 / 9 * 720) = 200, row from the top 319 - floor(1.0 / 4 * 320) = 239; a 5 x 5 square around it
    f = _only([[2.5, 1.0]], [[-1.0, -1.0]])[0]
    shade = tuple(replay.reds(1)[0])
    want = {(r, c) for r in range(237, 242) for c in range(198, 203)}
    assert _block(f, shade) == want
    painted = (f != 255).any(axis=2)
    assert int(painted.sum()) == 25
    # a higher point is drawn nearer the top
    g = _only([[2.5, 3.0]], [[-1.0, -1.0]])[0]
    assert _block(g, shade) == {(r, c) for r in range(77, 82) for c in range(198, 203)}


def test_points_outside_the_window_are_dropped_not_clamped():
    outside = [[-0.01, 1.0], [9.0, 1.0], [4.0, -0.01], [4.0, 4.0], [np.nan, 1.0], [100.0, 100.0]]
    f = _only(outside, [[9.5, 2.0]])[0]
    assert (f == 255).all()
    # a point inside but next to the edge keeps the part of its square that is on the canvas
    g = _only([[0.0, 0.0]], [[-1.0, -1.0]])[0]
    assert _block(g, tuple(replay.reds(1)[0])) == {(r, c) for r in range(317, 320) for c in range(0, 3)}


def test_agent_is_drawn_over_a_locust_at_the_same_spot():
    f = _only([[4.5, 2.0]], [[4.5, 2.0]])[0]
    blue = _block(f, replay.DODGERBLUE)
    assert blue == {(r, c) for r in range(156, 163) for c in range(357, 364)}       # 7 x 7 around (159, 360)
    assert int((f != 255).any(axis=2).sum()) == 49                                 # the locust's 5 x 5 lies under it


def test_locusts_are_shaded_red_by_index():
    shades = replay.reds(80).astype(int)
    assert tuple(shades[0]) == (255, 245, 240) and tuple(shades[-1]) == (103, 0, 13)      # the ends of 'Reds'
    assert (np.diff(shades.sum(axis=1)) < 0).all()                                        # darker with the index
    x = np.stack([np.linspace(0.5, 8.5, 80), np.full(80, 2.0)], axis=1)
    f = _only(x, [[-1.0, -1.0]])[0]
    cols = np.floor(x[:, 0] / 9 * W).astype(int)
    assert (f[159, cols[-1]] == shades[-1]).all() and (f[159, cols[40]] == shades[40]).all()


def test_save_gif_reads_back():
    Image = pytest.importorskip("PIL.Image")
    import tempfile, os
    rng = np.random.RandomState(0)
    f = replay.frames(rng.uniform(0, 4, size=(5, 80, 2)), rng.uniform(0, 4, size=(5, 10, 2)), width=180, height=80)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "swarm.gif")
        replay.save_gif(f, path, interval_ms=50)
        with Image.open(path) as im:
            assert im.n_frames == 5 and im.size == (180, 80)
            assert im.info.get("duration") == 50


def test_load_actions_round_trips_the_monitors_file(tmp_path):
    from goldsrl.agents.paac.policy_monitor import SwarmPolicyMonitor
    rng = np.random.RandomState(1)
    taken = [rng.normal(size=(10, 2)) for _ in range(7)]
    mon = SwarmPolicyMonitor.__new__(SwarmPolicyMonitor)      # _save_actions needs the path only
    mon.actions_path = str(tmp_path / "swarm-eval.json")
    mon._save_actions(-123.4567890123, [np.asarray(a).tolist() for a in taken])
    score, actions = replay.load_actions(mon.actions_path)
    assert score == -123.4567890123
    assert actions.dtype == np.float64 and actions.shape == (7, 10, 2)
    assert actions.tobytes() == np.asarray(taken).tobytes()
    with open(mon.actions_path, "w") as f:
        json.dump({"score": 0.0, "actions": [[1.0, 2.0]]}, f)
    with pytest.raises(ValueError):
        replay.load_actions(mon.actions_path)


def test_episode_totals_sum_the_played_part_only():
    rng = np.random.RandomState(2)
    r = np.zeros((2, 3, 130))
    n = np.array([[128, 1, 130], [5, 129, 64]], np.int32)
    for e in range(2):
        for s in range(3):
            r[e, s, :n[e, s]] = -rng.uniform(1, 2, size=n[e, s])
    tot = replay.episode_totals(r, n)
    for e in range(2):
        for s in range(3):
            assert tot[e, s] == np.sum(r[e, s, :n[e, s]])
