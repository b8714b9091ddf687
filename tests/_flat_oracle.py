"""The float64 oracle of FlatPolicyVNetwork (oracle/nets.py) over rollouts of bench size: NN.flat_loss_and_grads on chunks of
samples, combined as weighted means, and the contribution of a single 64-sample group (the unit the HIP kernels loop over) to the
mean gradient of the whole batch."""
import numpy as np

from oracle import nets as NN

CHUNK = 16384      # samples per oracle call: a TradeAR1-16 window of this many samples is 86 MB of float64


def dense_windows(hist):
    """Windows given as a (N, rnn, D) array (explicit histories; Solow's recorded ones)."""
    return lambda lo, hi: np.asarray(hist[lo:hi], np.float64)


def repeated_state_windows(states, nhist, rnn):
    """The PAAC worker's window (quirk Q11): the current state in rows < max(nhist, 1), capped at rnn, zeros after."""
    rows = np.minimum(np.maximum(np.asarray(nhist).reshape(-1), 1), rnn)

    def win(lo, hi):
        s = np.asarray(states[lo:hi], np.float64)
        keep = np.arange(rnn)[None, :] < rows[lo:hi, None]
        return np.where(keep[:, :, None], s[:, None, :], 0.0)
    return win


def loss_and_grads(p, states, windows, actions, adv, y, scale=100.0, lo=0, hi=None, chunk=CHUNK):
    """NN.flat_loss_and_grads over samples [lo, hi) (all by default) as chunks of `chunk` samples; every loss term and every gradient
    block is the mean over the range, i.e. the chunks' values times n_chunk / n.  Returns loss, policy_loss, critic_loss_mean,
    grads (dict), (mu, sigma, vs) of every sample."""
    hi = len(states) if hi is None else hi
    n = hi - lo
    terms, grads, outs = np.zeros(3), None, []
    for c0 in range(lo, hi, chunk):
        c1 = min(c0 + chunk, hi)
        f64 = lambda x: np.asarray(x[c0:c1], np.float64)      # noqa: E731
        loss, pl, cl, g, out = NN.flat_loss_and_grads(p, f64(states), windows(c0, c1), f64(actions), f64(adv), f64(y), scale)
        w = (c1 - c0) / n
        terms += w * np.array([loss, pl, cl])
        grads = {k: w * v for k, v in g.items()} if grads is None else {k: grads[k] + w * v for k, v in g.items()}
        outs.append(out)
    return terms[0], terms[1], terms[2], grads, tuple(np.concatenate(o) for o in zip(*outs))


def group_contribution(p, states, windows, actions, adv, y, group, scale=100.0):
    """What 64-sample group `group` adds to the mean gradient of all len(states) samples (its own mean times n_group / n)."""
    n = len(states)
    lo, hi = 64 * group, min(64 * group + 64, n)
    assert lo < hi, (group, n)
    g = loss_and_grads(p, states, windows, actions, adv, y, scale, lo, hi)[3]
    return {k: v * ((hi - lo) / n) for k, v in g.items()}


def block_errors(got, ref):
    """Per parameter block: max |got - ref| / max |ref| (the suite's gradient measure)."""
    return {k: float(np.abs(got[k] - ref[k]).max() / (np.abs(ref[k]).max() + 1e-12)) for k in ref}


def altered(ref, contributions):
    """The gradient with single groups left out (weight -1) or counted twice (+1): {label: (weight, contribution)} -> {label: grads}."""
    return {label: {k: ref[k] + w * c[k] for k in ref} for label, (w, c) in contributions.items()}


def sensitivity(ref, alterations):
    """For each altered gradient {label: grads}: its largest per-block distance from ref (block_errors), and that block."""
    out = {}
    for label, alt in alterations.items():
        e = block_errors(alt, ref)
        k = max(e, key=e.get)
        out[label] = (e[k], k)
    return out
