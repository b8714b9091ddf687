"""What the ctypes bindings of the two softmax-grid A3C nets share (DiscreteNet in _ffi_discrete.py: one output on Solow;
GridTradeNet in _ffi_gridtrade.py: one output per asset on TradeAR1): DiscretePolicyEstimator's parameter layout and default
initialisation for any num_outputs, and the net's calls with O = num_outputs in the shapes -- the axis is absent where O == 1."""
import numpy as np

from ._ffi_a3c import A3cNet


def grid_param_shapes(K, static_size, temporal_size, num_outputs, H=32, S=128):
    """tf.trainable_variables() order: the trunk (the Gaussian net's first ten blocks), the probs tower whose last layer has
    num_outputs * K columns (column o * K + j: output o, choice j), the value head."""
    X = 3 * H
    return [
        ("gru_gates_w", (temporal_size + H, 2 * H)), ("gru_gates_b", (2 * H,)), ("gru_cand_w", (temporal_size + H, H)), ("gru_cand_b", (H,)),
        ("temporal_w", (H, 2 * H)), ("temporal_b", (2 * H,)), ("static1_w", (static_size, 2 * H)), ("static1_b", (2 * H,)),
        ("static2_w", (2 * H, H)), ("static2_b", (H,)),
        ("probs1_w", (X, 2 * S)), ("probs1_b", (2 * S,)), ("probs2_w", (2 * S, S)), ("probs2_b", (S,)),
        ("probs3_w", (S, num_outputs * K)), ("probs3_b", (num_outputs * K,)),
        ("value1_w", (X, 2 * S)), ("value1_b", (2 * S,)), ("value2_w", (2 * S, 1)), ("value2_b", (1,)),
    ]


def default_init_grid(seed, K, static_size, temporal_size, num_outputs):
    """TF's defaults: glorot-uniform kernels, zero biases; the GRU as default_init_gated does it (gate bias 1)."""
    rng = np.random.RandomState(seed)
    parts = []
    for name, shape in grid_param_shapes(K, static_size, temporal_size, num_outputs):
        if name.endswith("_w"):
            lim = np.sqrt(6.0 / (shape[0] + shape[1]))
            parts.append(rng.uniform(-lim, lim, size=shape).reshape(-1))
        elif name == "gru_gates_b":
            parts.append(np.ones(shape))
        else:
            parts.append(np.zeros(shape))
    return np.concatenate(parts).astype(np.float32)


class GridNet(A3cNet):
    """A softmax-grid net on its Engine: predict / train on host samples, device-resident rollout + update, one-launch greedy
    evaluation.  A choice is, per output, an index into grid = np.linspace(grid_lb, grid_ub, num_choices); the env is stepped with
    the grid values.  Greedy: per output the first index of the largest probability.  The subclass sets PREFIX, SIGNATURES, CONFIG,
    SIZES (static_size = temporal_size and num_outputs) and TERM: whether the rollout keeps the terminal-pass buffers."""
    EVAL_TRACE = ("states", "choices", "actions", "rewards", "dones")

    def __init__(self, engine, **kw):
        self._create(engine, self.SIGNATURES, self.CONFIG(), kw)
        self.sizes = dict(self.SIZES)
        self.S0 = self.D = self.SIZES["static_size"]
        self.O, self.K = self.SIZES["num_outputs"], int(self.cfg.num_choices)
        self.tail = () if self.O == 1 else (self.O,)
        self.grid = np.linspace(self.cfg.grid_lb, self.cfg.grid_ub, self.K)

    def predict(self, states, windows):
        return self._predict(states, windows, (("probs", self.tail + (self.K,)),))

    def train(self, states, windows, choices, adv, targets, weights=None, grad_mult=1.0, lr=1e-4, apply_update=True):
        if not self.tail:
            choices = np.asarray(choices).reshape(-1)
        return self._train(states, windows, [(choices, np.int32, self.tail)], adv, targets, weights, grad_mult, lr, apply_update)

    def read_rollout(self, which):
        T, E, R, D = self.T, self.eng.E, self.R, self.D
        shapes = {"states": (T, E, self.S0), "windows": (T, E, R, D), "probs": (T, E) + self.tail + (self.K,), "choices": (T, E) + self.tail,
                  "actions": (T, E) + self.tail, "values": (T, E), "rewards": (T, E), "dones": (T, E), "weights": (T, E), "adv": (T, E),
                  "targets": (T, E), "boot": (E,)}
        if self.TERM:
            shapes.update({"term_values": (T, E), "term_states": (T, E, self.S0), "term_windows": (T, E, R, D)})
        return self._read("read_rollout", which, shapes[which])

    def eval(self, max_steps, trace_steps=0, trace_fields=EVAL_TRACE):
        """Greedy episodes of every env from the engine's current state (reset it first), one kernel launch; the engine is reset
        afterwards.  Returns total_reward (E) float64, length (E) int32, finished (E) uint8 and, with trace_steps > 0, states
        (S,E,S0), choices int32 and actions (S,E) or (S,E,O), rewards, dones (S,E) of the first S = min(trace_steps, steps played)
        steps, each defined up to its env's own end (trace_fields: the ones to read back)."""
        tails = {"states": (self.S0,), "choices": self.tail, "actions": self.tail, "rewards": (), "dones": ()}
        return self._eval(max_steps, trace_steps, trace_fields, tails)
