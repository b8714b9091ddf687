"""fed_gym/agents/a3c/estimators.py on the device: DiscreteAndContPolicyEstimator (:40-152), DiscretePolicyEstimator (:155-238),
GaussianPolicyEstimator (:241-334) and ValueEstimator (:338-417) on the shared rnn_graph_lstm trunk (:18-28), as facades over ONE device net (both estimators own the same
parameters, as the reference's two graphs share the "shared" variable scope).  The gated trader (goldsrl._ffi_gated.GatedNet)
exists for the Ticker sizes only: 2 assets x 3 choices, static input 7, temporal rows 4; the Gaussian agent
(goldsrl._ffi_gauss.GaussNet) for the Solow sizes (2, 2, 1 action) and the 2-asset TradeAR1 sizes (5, 5, 2 actions); the discrete
savings-grid agent (goldsrl._ffi_discrete.DiscreteNet) for the Solow sizes with one output of 2..64 choices; hidden sizes 32 / 128."""
import numpy as np

from ..._ffi_discrete import DiscreteNet
from ..._ffi_gauss import GaussNet


def _check_sizes(static_size, temporal_size, static_hidden_size, num_assets=2):
    if (num_assets, static_size, temporal_size, static_hidden_size) != (2, 7, 4, 128):
        raise ValueError("the device net exists for the Ticker sizes only: num_assets=2, static_size=7, temporal_size=4, "
                         "static_hidden_size=128 (got %r)" % ((num_assets, static_size, temporal_size, static_hidden_size),))


def _window(history, R):
    """pad_sequences(padding='post', maxlen=R) of the history rows (..., n, D): the last R rows, zero rows after"""
    h = np.asarray(history, np.float32)
    out = np.zeros(h.shape[:-2] + (R, h.shape[-1]), np.float32)
    n = min(R, h.shape[-2])
    out[..., :n, :] = h[..., -n:, :] if h.shape[-2] > R else h[..., :n, :]
    return out


def _batch(state, history, batch):
    s = np.asarray(state, np.float32)
    h = np.asarray(history, np.float32)
    if not batch:
        s, h = s[None], h[None]
    return s, h


class DiscreteAndContPolicyEstimator(object):
    """predict() returns the reference's keys: mu, sigma, probs, each (n, num_assets, 3)."""
    num_actions = 3
    BUY_IDX = 1
    SELL_IDX = 2

    def __init__(self, num_assets, static_size, temporal_size, shared_layer=None, static_hidden_size=128, trainable=True,
                 learning_rate=1e-4, seed=None, reuse=False, net=None):
        _check_sizes(static_size, temporal_size, static_hidden_size, num_assets)
        if net is None:
            raise ValueError("pass net=GatedNet(ticker_engine, ...): the estimators are facades over one device net")
        self.net, self.num_assets, self.static_size, self.temporal_size = net, num_assets, static_size, temporal_size
        self.learning_rate = learning_rate

    def predict(self, state, history, sess=None, batch=False):
        s, h = _batch(state, _window(history, self.net.R), batch)
        out = self.net.predict(s, h)
        return {"mu": out["mu"], "sigma": out["sigma"], "probs": out["probs"]}


def _is_gauss(net):
    return isinstance(net, GaussNet)


def _check_discrete_sizes(net, static_size, temporal_size, static_hidden_size, num_outputs=None, num_choices=None):
    got = (static_size, temporal_size, static_hidden_size)
    want = (net.S0, net.D, 128)
    if got != want or (num_outputs is not None and num_outputs != 1) or (num_choices is not None and num_choices != net.K):
        raise ValueError("the net was built for static_size=%d, temporal_size=%d, static_hidden_size=%d, num_outputs=1, num_choices=%d "
                         "(got %r, num_outputs=%r, num_choices=%r)" % (want + (net.K, got, num_outputs, num_choices)))


class DiscretePolicyEstimator(object):
    """predict() returns the reference's key: probs, (n, num_outputs = 1, num_choices).  lb and ub are accepted as the reference's
    constructor accepts them; it does not use them either (the grid is the worker's, the net's grid_lb / grid_ub here)."""

    def __init__(self, num_outputs, num_choices, static_size, temporal_size, shared_layer=None, static_hidden_size=128, reuse=False,
                 trainable=True, learning_rate=1e-4, seed=None, lb=-5., ub=5., net=None):
        if not isinstance(net, DiscreteNet):
            raise ValueError("pass net=DiscreteNet(solow_engine, num_choices=...): the estimators are facades over one device net")
        _check_discrete_sizes(net, static_size, temporal_size, static_hidden_size, num_outputs, num_choices)
        self.net, self.num_outputs, self.num_choices = net, num_outputs, num_choices
        self.static_size, self.temporal_size, self.learning_rate = static_size, temporal_size, learning_rate

    def predict(self, state, history, sess=None, batch=False):
        s, h = _batch(state, _window(history, self.net.R), batch)
        return {"probs": self.net.predict(s, h)["probs"][:, None, :]}


def _check_gauss_sizes(net, static_size, temporal_size, static_hidden_size, num_actions=None):
    got = (static_size, temporal_size, static_hidden_size)
    want = (net.sizes["static_size"], net.sizes["temporal_size"], 128)
    if got != want or (num_actions is not None and num_actions != net.sizes["num_actions"]):
        raise ValueError("the net was built for static_size=%d, temporal_size=%d, static_hidden_size=%d, num_actions=%d (got %r, "
                         "num_actions=%r)" % (want + (net.sizes["num_actions"], got, num_actions)))


class GaussianPolicyEstimator(object):
    """predict() returns the reference's keys: mu, sigma, each (n, num_actions)."""

    def __init__(self, num_actions, static_size, temporal_size, shared_layer=None, static_hidden_size=128, reuse=False, trainable=True,
                 learning_rate=1e-4, seed=None, lb=-5., ub=5., net=None):
        if not _is_gauss(net):
            raise ValueError("pass net=GaussNet(solow_or_trade_engine, ...): the estimators are facades over one device net")
        if (lb, ub) != (-5., 5.):
            raise ValueError("the device net has the reference's bounds lb=-5, ub=5 only")
        _check_gauss_sizes(net, static_size, temporal_size, static_hidden_size, num_actions)
        self.net, self.num_actions, self.static_size, self.temporal_size = net, num_actions, static_size, temporal_size
        self.learning_rate = learning_rate

    def predict(self, state, history, sess=None, batch=False):
        s, h = _batch(state, _window(history, self.net.R), batch)
        out = self.net.predict(s, h)
        return {"mu": out["mu"], "sigma": out["sigma"]}


class ValueEstimator(object):
    """predict() returns {'logits': (n,)}: scale times the value head, as the reference."""

    def __init__(self, static_size, temporal_size, shared_layer=None, static_hidden_size=128, reuse=False, trainable=True,
                 learning_rate=1e-4, num_actions=2, scale=1., net=None):
        if _is_gauss(net):
            _check_gauss_sizes(net, static_size, temporal_size, static_hidden_size)
        elif isinstance(net, DiscreteNet):
            _check_discrete_sizes(net, static_size, temporal_size, static_hidden_size)
        else:
            _check_sizes(static_size, temporal_size, static_hidden_size)
        if net is None:
            raise ValueError("pass net=GatedNet(ticker_engine, scale=...): the estimators are facades over one device net")
        if abs(net.cfg.scale - scale) > 1e-12 * max(1.0, abs(scale)):
            raise ValueError("scale %r differs from the net's %r" % (scale, net.cfg.scale))
        self.net, self.static_size, self.temporal_size, self.scale = net, static_size, temporal_size, scale
        self.learning_rate = learning_rate

    def predict(self, state, history, sess=None, batch=False):
        s, h = _batch(state, _window(history, self.net.R), batch)
        return {"logits": self.net.predict(s, h)["values"]}

