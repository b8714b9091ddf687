"""The bound the GPU tests hold the Adam updates to (tests/_adam_oracle.py), checked on the CPU: the float32 restatement of
paac_adam_kernel lies within it at every element, and each alteration of the arithmetic a zero-moment test cannot see leaves it on
at least a tenth of the buffer it touches."""
import numpy as np
import pytest

import _adam_oracle as AO

N, LR = 200000, 1e-3


@pytest.fixture(scope="module")
def inputs():
    g, m0, v0, p0 = AO.adam_inputs(N, seed=1)
    norm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    return g, m0, v0, p0, norm


def test_the_inputs_are_what_the_bound_was_checked_on(inputs):
    g, m0, v0, p0, _ = inputs
    assert all(a.dtype == np.float32 and a.shape == (N,) for a in (g, m0, v0, p0))
    assert (g[::11] == 0).all() and (m0[::7] == 0).all() and (v0[::7] == 0).all() and not g[::77].any()
    nz = g[g != 0]
    assert np.abs(nz).min() >= np.float32(1e-8) and max(np.abs(a).max() for a in (g, m0, v0, p0)) <= 1e3
    assert (np.sign(g) * np.sign(m0) < 0).mean() > 0.3 and (v0 >= 0).all()
    tiny = np.finfo(np.float32).tiny      # no subnormal input, and 0.001f * (g / 2)^2 stays normal
    for a in (g, m0, v0, p0):
        assert (np.abs(a[a != 0]) >= tiny).all()
    assert 1e-3 * (0.25 * np.abs(nz).min()) ** 2 > tiny


@pytest.mark.parametrize("t", [1, 7, 10 ** 6])
@pytest.mark.parametrize("clip", ["active", "inactive"])
def test_the_float32_kernel_lies_within_the_bound_at_every_element(inputs, t, clip):
    g, m0, v0, p0, norm = inputs
    clip_norm = norm * (0.5 if clip == "active" else 2.0)
    if t == 1:      # the first step starts from zero moments
        m0, v0 = np.zeros_like(m0), np.zeros_like(v0)
    ref = AO.reference(g, m0, v0, p0, t, LR, clip_norm)
    p, m, v = AO.kernel_f32(g, m0, v0, p0, t, LR, clip_norm)
    assert np.isfinite(p).all() and np.isfinite(m).all() and np.isfinite(v).all()
    assert (ref["norm"] > clip_norm) == (clip == "active")
    AO.assert_within(ref, p, m, v, "t=%d clip %s" % (t, clip))
    assert not np.array_equal(p, p0)


def test_grad_scale_multiplies_the_norm_and_the_gradient(inputs):
    g, m0, v0, p0, norm = inputs
    ref = AO.reference(g, m0, v0, p0, 7, LR, 0.25 * norm, grad_scale=0.5)
    np.testing.assert_allclose(ref["norm"], 0.5 * norm, rtol=1e-12)
    np.testing.assert_allclose(ref["gc"], g.astype(np.float64) * 0.25, rtol=1e-6)      # scaled by 0.5, then clipped to half its norm
    AO.assert_within(ref, *AO.kernel_f32(g, m0, v0, p0, 7, LR, 0.25 * norm, grad_scale=0.5))
    unclipped = AO.reference(g, m0, v0, p0, 7, LR, 0.0, grad_scale=0.5)      # clip_norm 0: no clip
    np.testing.assert_allclose(unclipped["gc"], g.astype(np.float64) * 0.5, rtol=0)
    AO.assert_within(unclipped, *AO.kernel_f32(g, m0, v0, p0, 7, LR, 0.0, grad_scale=0.5))


# what the zero-moment tests of the suite cannot see; buffer: where the alteration must show on >= 10 % of the elements
CONTROLS = [
    ("beta1 = 0.8", dict(b1=(0.8, 0.2)), "m"),
    ("beta2 = 0.99", dict(b2=(0.99, 0.01)), "v"),
    ("eps = 1e-7", dict(eps=1e-7), "p"),
    ("1 - beta2 computed in float32", dict(one_minus_b2_on_device=True), "v"),
    ("no bias correction", dict(bias_correction=False), "p"),
    ("clip factor left out", dict(clip="none"), "p"),
    ("clip applied to m instead of g", dict(clip="m"), "p"),
]


@pytest.mark.parametrize("label,kw,buffer", CONTROLS, ids=[c[0] for c in CONTROLS])
def test_an_altered_kernel_leaves_the_bound(inputs, label, kw, buffer):
    """Step 7 from the injected moments, clip at half the norm."""
    g, m0, v0, p0, norm = inputs
    ref = AO.reference(g, m0, v0, p0, 7, LR, 0.5 * norm)
    share = AO.shares(ref, *AO.kernel_f32(g, m0, v0, p0, 7, LR, 0.5 * norm, **kw))
    print("\n[adam bound] %s: outside the bound p %.1f %%, m %.1f %%, v %.1f %%" % (label, 100 * share["p"], 100 * share["m"], 100 * share["v"]))
    assert share[buffer] >= 0.10, (label, share)
