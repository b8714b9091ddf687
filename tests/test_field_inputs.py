"""CPU: goldsrl.agents.state_processors.swarm_field_inputs -- the numpy restatement of the two inputs of ConvPolicyVFieldNetwork on
Swarm (the reference's SwarmStateProcessor.process_state, fed_gym/agents/state_processors.py:15-44) from the handle's compact
observation: bins 255 are not counted, image axis 0 is the x bin, the float32 values are float32(count / 80.0) and
float32(count / 10.0), and on drawn positions it is process_state's np.histogram2d image (restated here) cast to float32."""
import numpy as np

from goldsrl.agents.state_processors import swarm_field_inputs

G = 20


def _empty(E=1):
    lb = np.full((E, 80, 2), 255, np.uint8)
    ab = np.full((E, 10, 2), 255, np.uint8)
    pos = np.zeros((E, 10, 2), np.uint8)
    return lb, ab, pos


def test_outside_bins_are_not_counted_and_axis_0_is_the_x_bin():
    lb, ab, pos = _empty(2)
    lb[0, 0] = (3, 7)                   # bx = 3, by = 7
    lb[0, 1] = (255, 255)               # outside the box
    ab[0, 4] = ab[0, 9] = (5, 2)        # two agents in one cell
    ab[1, 0] = (G - 1, 0)
    pos[0, 4] = (5, 2); pos[1, 0] = (G - 1, 0)
    states, positions = swarm_field_inputs(lb, ab, pos, G)
    assert states.shape == (2, G, G, 2) and states.dtype == np.float32
    assert positions.shape == (2, 10, 2) and positions.dtype == np.int32 and np.array_equal(positions, pos)
    want = np.zeros((2, G, G, 2), np.float32)
    want[0, 3, 7, 0] = np.float32(1 / 80.0)
    want[0, 5, 2, 1] = np.float32(0.2)
    want[1, G - 1, 0, 1] = np.float32(0.1)
    assert np.array_equal(states, want)
    assert states[0, 7, 3, 0] == 0 and states[0, 5, 2, 1] == np.float32(2 / 10.0)
    assert states[..., 0].sum() * 80 == 1      # the locust at (255, 255) is nowhere


def test_every_count_gives_the_float32_of_the_float64_quotient():
    for c in range(81):
        lb, ab, pos = _empty()
        lb[0, :c] = (1, 2)
        ab[0, :min(c, 10)] = (4, 4)
        states, _ = swarm_field_inputs(lb, ab, pos, G)
        assert states[0, 1, 2, 0] == np.float32(c / 80.0), c
        assert states[0, 4, 4, 1] == np.float32(min(c, 10) / 10.0), c
        assert np.count_nonzero(states) == (2 if c else 0)


def _bin(p, edges):
    """np.histogram2d's bin of a coordinate along one axis: half-open cells, the last one closed; -1 outside"""
    b = np.searchsorted(edges, p, side='right') - 1
    b[p == edges[-1]] = len(edges) - 2
    b[(p < edges[0]) | (p > edges[-1])] = -1
    return b


def _compact(points, x_edges, y_edges):
    bx, by = _bin(points[:, 0], x_edges), _bin(points[:, 1], y_edges)
    out = (bx < 0) | (by < 0)
    return np.where(out[:, None], 255, np.stack([bx, by], axis=-1)).astype(np.uint8)


def test_equals_the_histogram2d_form_of_process_state():
    rng = np.random.RandomState(7)
    WIDTH = HEIGHT = 3.
    E = 6
    lb, ab, want = [], [], []
    for e in range(E):
        x = rng.uniform(0.0, 1.0, size=(80, 2)) * (4.0, 7.0) + (rng.uniform(-2, 2), -0.5)      # some points outside the box
        xa = rng.uniform(0.0, 1.0, size=(10, 2)) * (4.0, 7.0) + (x[:, 0].mean() - 2.0, -0.5)
        # process_state (state_processors.py:26-33,35-44)
        mean_x = np.mean(np.vstack([x, xa]), axis=0)[0]
        bounding_box = [[mean_x - WIDTH / 2., mean_x + WIDTH / 2.], [0, 2 * HEIGHT]]
        x_grid, x_edges, y_edges = np.histogram2d(x[:, 0], x[:, 1], G, bounding_box)
        xa_grid, _, _ = np.histogram2d(xa[:, 0], xa[:, 1], bins=[x_edges, y_edges])
        want.append(np.stack([x_grid / len(x), xa_grid / len(xa)], axis=-1))
        lb.append(_compact(x, x_edges, y_edges)); ab.append(_compact(xa, x_edges, y_edges))
    lb, ab = np.stack(lb), np.stack(ab)
    assert (lb == 255).any() and (ab == 255).any() and (lb != 255).sum() > 100
    states, _ = swarm_field_inputs(lb, ab, np.zeros((E, 10, 2), np.uint8), G)
    for e in range(E):
        assert np.array_equal(states[e], want[e].astype(np.float32)), e
