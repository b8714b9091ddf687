"""The update every PAAC net ends with -- global norm, tf.clip_by_global_norm, Adam -- in one place for the tests: the float64
reference (oracle/nets.py on the float32 inputs the device holds), the per-element bound a device result is held to, inputs that
exercise it away from zero moments, and the float32 restatement of paac_adam_kernel (net_paac_host.h) with the alterations the
bound must see (tests/test_adam_bounds.py).

The bound is the one tests/test_gpu_flatnet_oracle.py introduced for the flat net's second step: 8 float32 roundings per buffer,
which covers the clip factor (norm and quotient rounded once each, the product with the gradient once) and the kernel's own
operations (-ffp-contract=off, no fast-math: one rounding per operation, the literals 0.9f / 0.1f / 0.999f / 0.001f / 1e-8f)."""
import numpy as np

from oracle import nets as NN

U = 8 * 2.0 ** -24
F32, F64 = np.float32, np.float64


def _f(x):
    """a scalar as the C ABI passes it: float32"""
    return float(F32(x))


def reference(g, m0, v0, p0, t, lr, clip_norm, grad_scale=1.0):
    """Update number t (>= 1) in float64.  g: the gradient as the device holds it; grad_scale multiplies the norm and the gradient
    (finalize_stats_kernel, flat_finalize_kernel); clip_norm <= 0: no clip.  lr, clip_norm and grad_scale enter as the float32
    values the device receives.  Returns a dict: p, m, v, gc (the clipped gradient), norm, m0, lr, t."""
    lr, clip_norm, grad_scale = _f(lr), _f(clip_norm), _f(grad_scale)
    gs = np.asarray(g, F32).astype(F64) * grad_scale
    if clip_norm > 0:
        gc, norm = NN.clip_by_global_norm(gs, clip_norm)
    else:
        gc, norm = gs, np.sqrt(np.sum(gs ** 2))
    m0 = np.asarray(m0, F32).astype(F64)
    p, m, v = NN.adam_step(np.asarray(p0, F32).astype(F64), gc, m0, np.asarray(v0, F32).astype(F64), t, lr)
    return dict(p=p, m=m, v=v, gc=gc, norm=float(norm), m0=m0, lr=lr, t=int(t))


def tolerances(ref):
    """per element: how far m, v and the parameters may lie from the reference"""
    m_tol = U * (np.abs(ref["m0"]) + np.abs(ref["gc"]))
    v_tol = U * ref["v"] + 1e-37
    t = ref["t"]
    lr_t = ref["lr"] * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
    p_tol = U * np.abs(ref["p"]) + lr_t * (m_tol + U * np.abs(ref["m"])) / (np.sqrt(ref["v"]) + 1e-8)
    return dict(m=m_tol, v=v_tol, p=p_tol)


def violations(ref, p, m, v):
    """{'p' | 'm' | 'v': boolean array, True where the buffer leaves the bound (or is not finite)}"""
    tol = tolerances(ref)
    got = dict(p=p, m=m, v=v)
    return {k: ~(np.abs(np.asarray(got[k], F64) - ref[k]) <= tol[k]) for k in ("p", "m", "v")}


def shares(ref, p, m, v):
    """{'p' | 'm' | 'v': share of the elements outside the bound}"""
    return {k: float(b.mean()) for k, b in violations(ref, p, m, v).items()}


def assert_within(ref, p, m, v, label=""):
    bad = violations(ref, p, m, v)
    for k in ("m", "v", "p"):
        n = int(bad[k].sum())
        if n:
            i = int(np.flatnonzero(bad[k])[0])
            got = dict(p=p, m=m, v=v)[k]
            raise AssertionError("%s %s: %d of %d elements (%.2f %%) outside the bound; first at %d: got %r, reference %r, tolerance %.3g"
                                 % (label, k, n, bad[k].size, 100.0 * n / bad[k].size, i, float(got[i]), float(ref[k][i]),
                                    float(tolerances(ref)[k][i])))


def adam_inputs(n, seed):
    """g, m0, v0, p0 (float32, n each) away from everything the zero-moment tests see: gradients over five decades with either
    sign and every 11th exactly 0; first moments whose sign is independent of the gradient's; second moments over five decades;
    every 7th entry of both moments exactly 0 (every 77th element is 0 / (0 + eps)).  Non-zero |g| >= 1e-8 and every value <= 1e3:
    no intermediate of the update is subnormal or infinite, so the device's flush mode does not enter."""
    rng = np.random.RandomState(seed)
    g = rng.normal(size=n) * np.exp(2 * rng.normal(size=n)) * 1e-2
    g = np.sign(g) * np.clip(np.abs(g), 1e-8, 1e3)
    g[::11] = 0
    m0 = 1e-3 * rng.normal(size=n)
    v0 = np.minimum(1e-6 * np.exp(3 * rng.normal(size=n)), 1e3)
    m0[::7] = 0
    v0[::7] = 0
    p0 = 0.05 * rng.normal(size=n)
    return g.astype(F32), m0.astype(F32), v0.astype(F32), p0.astype(F32)


def device_clip_factor(g, clip_norm, grad_scale=1.0):
    """(norm, factor) as finalize_stats_kernel rounds them: the float64 sum of squares, norm = float32(sqrt(s) * grad_scale),
    factor = grad_scale * (clip_norm / max(norm, clip_norm)) in float32 (1 without a clip)."""
    clip, gs = F32(clip_norm), F32(grad_scale)
    norm = F32(np.sqrt(np.sum(np.asarray(g, F32).astype(F64) ** 2)) * F64(gs))
    return norm, gs * (clip / np.maximum(norm, clip) if clip > 0 else F32(1))


def kernel_f32(g, m0, v0, p0, t, lr, clip_norm, grad_scale=1.0, b1=(0.9, 0.1), b2=(0.999, 0.001), eps=1e-8, one_minus_b2_on_device=False,
               bias_correction=True, clip="g"):
    """paac_adam_kernel behind finalize_stats_kernel and adam_lr_t in numpy float32, one rounding per operation.  The keywords are
    the alterations of the negative controls: b1 / b2 = (beta, 1 - beta) literals; one_minus_b2_on_device: 1.0f - b2 computed in
    float32; bias_correction False: lr_t = lr; clip 'g' (as built), 'none' (factor left out) or 'm' (applied to m instead of g)."""
    g, m0, v0, p0 = (np.asarray(a, F32) for a in (g, m0, v0, p0))
    _, factor = device_clip_factor(g, clip_norm, grad_scale)
    gs = F32(grad_scale)
    lr32 = F32(lr)
    lr_t = F32(F64(lr32) * np.sqrt(1.0 - 0.999 ** F64(t)) / (1.0 - 0.9 ** F64(t))) if bias_correction else lr32
    c1, d1, c2 = F32(b1[0]), F32(b1[1]), F32(b2[0])
    d2 = F32(1) - c2 if one_minus_b2_on_device else F32(b2[1])
    gi = g * (factor if clip == "g" else gs)
    mi = c1 * m0 + d1 * gi
    if clip == "m":
        mi = mi * (factor / gs)
    vi = c2 * v0 + d2 * gi * gi
    p = p0 - lr_t * mi / (np.sqrt(vi) + F32(eps))
    assert p.dtype == mi.dtype == vi.dtype == F32
    return p, mi, vi
