"""The numpy statements of a cross-entropy search that know nothing of the env whose rule is searched (the numbering is that of
include/goldsrl_swarmsearch.h and include/goldsrl_tickersearch.h), and the argument checks every such search makes, device-free.
One copy for _ffi_swarmsearch, _ffi_swarmcemplan and _ffi_tickersearch, as csrc/search_dev.h is for their kernels: a tie rule, a
message or the refit is changed here, and the searches cannot drift apart."""
import numpy as np

MAX_CANDIDATES = 1024
BOX_NAMES = ("spread", "floor", "lo", "hi")          # the four per-parameter vectors every search takes


def first_max(a, b):
    return np.where(a >= b, a, b)                   # the first operand wins a tie, as the device's select


def first_min(a, b):
    return np.where(a <= b, a, b)


def search_clamp(v, lo, hi):
    """Statement 1: into the box."""
    return first_min(first_max(v, lo), hi)


def search_draw(mean, std, z, lo, hi):
    """Statement 2.  mean, std, lo, hi: (P,); z: (C, P) normals.  Returns the (C, P) float64 numbers inside the box."""
    mean, std, lo, hi = (np.asarray(v, np.float64) for v in (mean, std, lo, hi))
    v = std[None] * np.asarray(z, np.float64)
    v = mean[None] + v
    return search_clamp(v, lo[None], hi[None])


def search_rank(fit):
    """Statement 7: the candidates by fit descending, a tie going to the smaller index.  (C,) int32."""
    fit = np.asarray(fit, np.float64)
    return np.array(sorted(range(len(fit)), key=lambda c: (-fit[c], c)), np.int32)


def search_refit(fit, columns, K, floor):
    """Statements 7 and 8.  fit (C,), columns (C, P) float64: a parameter per column.  Returns (order (C,) int32, mean (P,), std (P,)),
    the two sequential chains over the K elites in rank order."""
    order = search_rank(fit)
    p = columns[order[:K]]                                                  # (K, P)
    kk = np.float64(K)
    m = np.zeros(p.shape[1], np.float64)
    for i in range(K):
        m = m + p[i]
    mean = m / kk
    s = np.zeros(p.shape[1], np.float64)
    for i in range(K):
        d = p[i] - mean
        q = d * d
        s = s + q
    v = s / kk
    sd = np.sqrt(v)
    return order, mean, first_max(sd, np.asarray(floor, np.float64))


def check_counts(fn_name, generations, candidates, elites):
    """The three counts as ints."""
    G, Cn, K = int(generations), int(candidates), int(elites)
    if G < 1 or not 2 <= Cn <= MAX_CANDIDATES or not 1 <= K <= Cn:
        raise ValueError("%s: generations >= 1, 2 <= candidates <= %d and 1 <= elites <= candidates are required, got %d, %d, %d"
                         % (fn_name, MAX_CANDIDATES, G, Cn, K))
    return G, Cn, K


def check_vectors(fn_name, names, values, defaults, fields):
    """One float64 vector of len(fields) finite numbers per name; defaults: None, or what stands in for a value that is None."""
    out = []
    for i, (name, v) in enumerate(zip(names, values)):
        a = defaults[i] if defaults is not None and v is None else np.ascontiguousarray(np.asarray(v, np.float64).reshape(-1))
        if a.shape != (len(fields),) or not np.isfinite(a).all():
            raise ValueError("%s: %s must be %d finite numbers over %s" % (fn_name, name, len(fields), (fields,)))
        out.append(a)
    return out


def check_box(fn_name, spread, floor, lo, hi):
    if (spread < 0).any() or (floor < 0).any() or (lo > hi).any():
        raise ValueError("%s: spread >= 0, floor >= 0 and lo <= hi are required" % fn_name)


def check_normals(fn_name, normals, seed, shape, wording):
    """The normals as a contiguous float64 array of `shape` (None: drawn from np.random.default_rng(seed)).  wording: how the message
    names that shape."""
    if normals is None:
        normals = np.random.default_rng(seed).standard_normal(shape)
    z = np.ascontiguousarray(np.asarray(normals, np.float64))
    if z.shape != tuple(shape) or not np.isfinite(z).all():
        raise ValueError("%s: normals must be %s, got shape %s" % (fn_name, wording, z.shape))
    return z


def search_summary(out):
    """best_rule, best_fit and best_per_generation from a search's outputs."""
    G = out["fit"].shape[0]
    first = out["order"][:, 0]
    out["best_per_generation"] = out["fit"][np.arange(G), first]
    out["best_rule"] = tuple(float(v) for v in out["candidates"][G - 1, first[G - 1]])
    out["best_fit"] = float(out["best_per_generation"][G - 1])
    return out
