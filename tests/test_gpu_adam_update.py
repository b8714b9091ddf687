"""GPU: the update all four PAAC nets end with (float64 sum of squares, the one-thread finalize kernel, paac_adam_kernel), held per
element to the float64 oracle past the first step (tests/_adam_oracle.py: the bound of 8 float32 roundings and its inputs).

The other update tests of the suite start from zero moments on one fixed batch, where the bias-corrected step is
lr * g / (|g| + eps') whatever beta1 and beta2 are.  Here the gradient, both moments and the step count are injected (conv and
flat net: set_grads / apply_grads; field net: the device's own gradient of a bit-reproducible pass), so m, v and the parameters
each depend on every constant of the kernel.

Before the conv net moved to paac_adam_kernel its own kernel computed 1.0f - 0.999f on the device (1.3e-5 low, relative).  Measured
on the MI355X with that kernel, the conv cases of this file left the bound on v at 42.64 % of the 2 210 213 elements
(clip_active, step_1e6 and lr_zero: 942 388 each), 17.21 % (clip_inactive_half_scale), 90.91 % (first_step: every element with a
gradient) and 50.46 % (no_clip), and on the parameters at 0.49 % to 5.76 %; m never left it, nor did anything of zero_gradient
(1 - beta2 meets no non-zero square there).  The flat cases passed with either kernel."""
import numpy as np
import pytest

import _adam_oracle as AO
import _field_rollout_cases as FC
import test_gpu_fieldnet as TFI
import test_gpu_flatnet as TFL
import test_gpu_net as TN

pytestmark = pytest.mark.gpu

LR = 1e-3
NORM_RTOL = 2 * 2.0 ** -24      # one rounding of the double sum's root times grad_scale to float32, one of the sum itself

# name: (clip: 'half' of the gradient's norm | 40 | 0, t0, grad_scale, lr, gradient, moments)
CASES = {
    "clip_active": ("half", 6, 1.0, LR, "g", "injected"),
    "clip_inactive_half_scale": (40.0, 6, 0.5, LR, "g_small", "injected"),
    "step_1e6": ("half", 10 ** 6 - 1, 1.0, LR, "g", "injected"),
    "first_step": ("half", 0, 1.0, LR, "g", "zero"),
    "zero_gradient": ("half", 6, 1.0, LR, "zero", "injected"),
    "lr_zero": ("half", 6, 1.0, 0.0, "g", "injected"),
    "no_clip": (0.0, 6, 1.0, LR, "g", "injected"),
}

_data, _nets = {}, {}


def _inputs(n):
    """g, a power-of-two multiple of it whose norm lies below 40, m0, v0 and the float64 norm of g for a net of n parameters"""
    if n not in _data:
        g, m0, v0, _ = AO.adam_inputs(n, seed=3)
        norm = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
        k = min(0, int(np.floor(np.log2(30.0 / norm))))
        _data[n] = dict(g=g, g_small=(g * np.float32(2.0 ** k)).astype(np.float32), zero=np.zeros(n, np.float32), m0=m0, v0=v0, norm=norm)
    return _data[n]


def _conv_net(clip):
    """a conv net (4 Swarm envs, chunks of 40 samples, 2.2 M biased Glorot parameters) after one gradient pass: apply_grads is allowed"""
    from goldsrl import _ffi_net
    if "conv" not in _nets:
        eng, net, p, states, obs = TN._setup(4)
        act, adv, y = TN._train_inputs(4)
        _nets["conv"] = dict(eng=eng, obs=obs, batch=(act, adv, y), p0=net.get_params(), nets={40.0: net})
        net.train_obs(*obs, act, adv, y, lr=0.0, apply_update=False)
    c = _nets["conv"]
    value = 0.5 * _inputs(c["p0"].size)["norm"] if clip == "half" else clip
    if clip not in c["nets"]:
        net = _ffi_net.ConvNet(c["eng"], max_chunk_samples=40, clip_norm=value)      # clip_norm 0 is accepted: no clip
        net.set_params(c["p0"])
        net.train_obs(*c["obs"], *c["batch"], lr=0.0, apply_update=False)
        c["nets"][clip] = net
    return c["nets"][clip], c["p0"]


def _flat_net(clip):
    """a Solow flat net (max_samples 256) after one gradient pass; its parameter count is no multiple of 256: the last block of the
    sum-of-squares and Adam grids is partial"""
    if "flat" not in _nets:
        _nets["flat"] = dict(nets={}, p0=None, n=None)
    c = _nets["flat"]
    if clip not in c["nets"]:
        value = clip
        if clip == "half":
            value = 0.5 * _inputs(_flat_net(40.0)[0].num_params)["norm"]
        eng, net = TFL._net({}, max_samples=256, clip_norm=value)
        TFL._params(net)
        states, hist, act, adv, y = TFL._samples(100, 2, 2, 5, 1, seed=3)
        net.train(states, hist, act, adv, y, lr=0.0, apply_update=False)
        c["nets"][clip] = (net, eng, (states, hist, act, adv, y))
        c["p0"] = net.get_params()
    assert c["p0"].size % 256 != 0
    return c["nets"][clip][0], c["p0"]


def _update(net, p0, g, m0, v0, t0, lr, grad_scale, label):
    """one injected update on the device against the reference: the step count, the reported norm and the three buffers"""
    net.set_params(p0)
    net.set_grads(g)
    net.set_optimizer_state(m0, v0, t0)
    st = net.apply_grads(lr, grad_scale)
    p, opt = net.get_params(), net.get_optimizer_state()
    ref = AO.reference(g, m0, v0, p0, t0 + 1, lr, net.cfg.clip_norm, grad_scale)
    print("\n[adam update] %s: outside the bound %s of %d elements; global_norm %r (float64 %r)"
          % (label, {k: "%.2f %%" % (100 * s) for k, s in AO.shares(ref, p, opt["adam_m"], opt["adam_v"]).items()}, p.size,
             st["global_norm"], ref["norm"]))
    assert opt["adam_step"] == t0 + 1
    assert np.isfinite(p).all() and np.isfinite(opt["adam_m"]).all() and np.isfinite(opt["adam_v"]).all() and np.isfinite(list(st.values())).all()
    np.testing.assert_allclose(st["global_norm"], ref["norm"], rtol=NORM_RTOL, atol=0)
    AO.assert_within(ref, p, opt["adam_m"], opt["adam_v"], label)
    return ref, p, opt, st


def _run_case(make_net, case):
    clip, t0, grad_scale, lr, gk, mk = CASES[case]
    net, p0 = make_net(clip)
    d = _inputs(p0.size)
    g = d[gk]
    m0, v0 = (d["m0"], d["v0"]) if mk == "injected" else (d["zero"], d["zero"])
    ref, p, opt, st = _update(net, p0, g, m0, v0, t0, lr, grad_scale, case)
    raw = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    if case == "clip_inactive_half_scale":      # the reported norm is that of grad_scale * g, and it stays below the clip
        np.testing.assert_allclose(st["global_norm"], 0.5 * raw, rtol=NORM_RTOL)
        assert 0.5 * raw < 40.0 and np.array_equal(ref["gc"], 0.5 * g.astype(np.float64))
    elif clip == "half":
        assert gk == "zero" or ref["norm"] > net.cfg.clip_norm > 0
    else:
        assert net.cfg.clip_norm == 0 and np.array_equal(ref["gc"], g.astype(np.float64))
    if case == "zero_gradient":      # norm 0: the clip factor is clip / max(0, clip) = 1; untouched moments leave the parameter alone
        assert st["global_norm"] == 0.0
        idle = (m0 == 0) & (v0 == 0)
        assert idle.any() and np.array_equal(p[idle], p0[idle]) and not opt["adam_m"][idle].any() and not opt["adam_v"][idle].any()
        assert (p[~idle] != p0[~idle]).mean() > 0.9      # the others move by the decaying moments' step (held to the oracle above)
    elif case == "lr_zero":
        assert np.array_equal(p, p0) and (opt["adam_m"] != m0).mean() > 0.8 and (opt["adam_v"] != v0).mean() > 0.8
    else:
        assert (p != p0).mean() > 0.5
    return net


def _one_hot_norms(net, p0):
    """a gradient with one non-zero entry: the norm is |value| * grad_scale exactly, wherever the entry lies in the grid"""
    n, value = p0.size, np.float32(-3.7)
    zero = np.zeros(n, np.float32)
    for i, grad_scale in ((0, 1.0), (255, 0.5), (256, 1.0), (n - 1, 0.5)):
        g = zero.copy()
        g[i] = value
        net.set_params(p0)
        net.set_grads(g)
        net.set_optimizer_state(zero, zero, 0)
        st = net.apply_grads(0.0, grad_scale)
        assert st["global_norm"] == float(np.abs(value)) * grad_scale, (i, grad_scale, st)
        m = net.get_optimizer_state()["adam_m"]
        assert np.flatnonzero(m).tolist() == [i]


def _state(net):
    opt = net.get_optimizer_state()
    return [net.get_params(), opt["adam_m"], opt["adam_v"], np.int64(opt["adam_step"])]


@pytest.mark.parametrize("case", sorted(CASES))
def test_conv_update_matches_the_oracle_from_injected_state(case):
    net = _run_case(_conv_net, case)
    assert net.range_info() == {"gemm_f32": False, "fallbacks": 0, "update_skipped": False}


def test_conv_norm_of_a_one_hot_gradient_is_exact():
    _one_hot_norms(*_conv_net(40.0))


def test_conv_gradient_passes_leave_parameters_and_optimizer_state_alone():
    net, p0 = _conv_net("half")
    d, c = _inputs(p0.size), _nets["conv"]
    net.set_params(p0)
    net.set_optimizer_state(d["m0"], d["v0"], 6)
    before = _state(net)
    net.train_obs(*c["obs"], *c["batch"], lr=LR, apply_update=False)
    net.rollout(3, 0)
    c["eng"].wait()
    st = net.train_rollout_grads()
    assert np.isfinite(st["global_norm"]) and st["global_norm"] > 0
    for a, b in zip(before, _state(net)):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("case", sorted(CASES))
def test_flat_update_matches_the_oracle_from_injected_state(case):
    _run_case(_flat_net, case)


def test_flat_norm_of_a_one_hot_gradient_is_exact():
    _one_hot_norms(*_flat_net(40.0))


def test_flat_gradient_passes_leave_parameters_and_optimizer_state_alone():
    net, p0 = _flat_net("half")
    _, eng, batch = _nets["flat"]["nets"]["half"]
    d = _inputs(p0.size)
    net.set_params(p0)
    net.set_optimizer_state(d["m0"], d["v0"], 6)
    before = _state(net)
    net.train(*batch, lr=LR, apply_update=False)
    net.rollout(5)
    eng.wait()
    st = net.train_rollout_grads()
    assert np.isfinite(st["global_norm"]) and st["global_norm"] > 0
    for a, b in zip(before, _state(net)):
        assert np.array_equal(a, b)


def _check_field_update(net, p0, g, m0, v0, t0, st, label):
    """the field net's update on its own gradient g (as get_grads returns it) from the injected moments"""
    p, opt = net.get_params(), net.get_optimizer_state()
    ref = AO.reference(g, m0, v0, p0, t0 + 1, LR, net.cfg.clip_norm)
    print("\n[adam update] %s: outside the bound %s of %d elements; %d gradient entries exactly 0"
          % (label, {k: "%.2f %%" % (100 * s) for k, s in AO.shares(ref, p, opt["adam_m"], opt["adam_v"]).items()}, p.size, int((g == 0).sum())))
    assert opt["adam_step"] == t0 + 1 and ref["norm"] > net.cfg.clip_norm > 0
    np.testing.assert_allclose(st["global_norm"], ref["norm"], rtol=NORM_RTOL, atol=0)
    AO.assert_within(ref, p, opt["adam_m"], opt["adam_v"], label)
    # head columns of pixels no agent stands on: no gradient at all; with untouched moments the parameter keeps its bits
    idle = (g == 0) & (m0 == 0) & (v0 == 0)
    assert (g == 0).sum() > 100 and idle.any()
    assert np.array_equal(p[idle], p0[idle]) and not opt["adam_m"][idle].any() and not opt["adam_v"][idle].any()
    assert (p != p0).mean() > 0.5


def test_field_host_train_update_from_injected_moments():
    from goldsrl import _ffi_field
    conf = dict(TFI.REF_CONF, height=16, width=24, channels=2, filters=7, conv_layers=1, num_actions=2, scale=10.,
                entropy_regularisation_strength=0.02)
    eng, est = TFI._bind(conf)
    _, _, flat = TFI._shared_params(est, conf)
    H, W, C, A = conf['height'], conf['width'], conf['channels'], conf['num_actions']
    rng = np.random.RandomState(5)
    N = 23
    states = rng.uniform(size=(N, H, W, C)).astype(np.float32)
    pos = np.stack([rng.randint(0, H, N), rng.randint(0, W, N)], axis=1).astype(np.int32)
    pos[7] = pos[2]; pos[11] = pos[2]
    batch = (states, pos, rng.uniform(size=(N, A)).astype(np.float32), rng.normal(size=N).astype(np.float32), rng.normal(size=N).astype(np.float32))
    norm = est.train(*batch, lr=0.0, apply_update=False)["global_norm"]
    net = _ffi_field.FieldNet(eng, max_samples=64, scale=conf['scale'], entropy_beta=conf['entropy_regularisation_strength'],
                              clip_norm=0.5 * norm, **TFI._geom(conf))
    net.set_params(flat)
    net.train(*batch, lr=0.0, apply_update=False)
    g = net.get_grads()
    assert np.array_equal(g, est.net.get_grads())
    _, m0, v0, _ = AO.adam_inputs(flat.size, seed=5)
    net.set_optimizer_state(m0, v0, 6)
    st = net.train(*batch, lr=LR)
    assert np.array_equal(net.get_grads(), g)      # the update ran on the gradient the bound is taken on
    _check_field_update(net, flat, g, m0, v0, 6, st, "field host train")
    net.close(); est.net.close(); eng.close()


@pytest.mark.parametrize("fused", [pytest.param(True, id="fused"), pytest.param(False, id="layers")])
def test_field_rollout_update_from_injected_moments(fused, monkeypatch):
    geom = "G20_L2_F5"
    FC.set_fused(monkeypatch, fused)
    _, _, flat = FC.params(geom)
    eng1, eng2 = FC.engine(geom), FC.engine(geom)
    n1 = FC.net(eng1, geom, counter=FC.COUNTER0)
    n1.rollout(FC.T, 0)
    eng1.wait()
    norm = n1.train_rollout_grads()["global_norm"]
    n2 = FC.net(eng2, geom, clip_norm=0.5 * norm, counter=FC.COUNTER0)
    n2.rollout(FC.T, 0)
    eng2.wait()
    assert np.array_equal(n2.read_rollout("actions", FC.T), n1.read_rollout("actions", FC.T))      # the same rollout on the twin engine
    n2.train_rollout_grads()
    g = n2.get_grads()
    assert np.array_equal(g, n1.get_grads())
    _, m0, v0, _ = AO.adam_inputs(flat.size, seed=6)
    n2.set_optimizer_state(m0, v0, 6)
    st = n2.train_rollout(LR)
    assert np.array_equal(n2.get_grads(), g)
    _check_field_update(n2, flat, g, m0, v0, 6, st, "field rollout, %s" % ("fused" if fused else "layers"))
    for x in (n1, n2, eng1, eng2):
        x.close()


@pytest.mark.parametrize("gemm", ["default", "f32"])
def test_conv_state_derived_from_the_parameters_follows_every_way_they_change(gemm, monkeypatch, tmp_path):
    """The conv net keeps copies derived from its parameters (refresh_transposes, net_conv.hip: the transposed head and conv
    kernels wpvT, w3f, w2corr and the trunk's background rows).  After each of the four ways the parameters change, the used net
    must predict and differentiate bit for bit as a fresh net given the same parameters."""
    from goldsrl import _ffi_net
    if gemm == "f32":
        monkeypatch.setenv("GRL_NET_GEMM", "f32")      # read at create
    else:
        monkeypatch.delenv("GRL_NET_GEMM", raising=False)
    eng, used, _, _, obs = TN._setup(4)
    act, adv, y = TN._train_inputs(4)
    assert used.range_info()["gemm_f32"] == (gemm == "f32")
    seen = [used.get_params()]

    def outputs(net):
        pred = net.predict_obs(*obs)
        net.train_obs(*obs, act, adv, y, lr=0.0, apply_update=False)
        return pred, net.get_grads()

    def check(label):
        params = used.get_params()
        assert not any(np.array_equal(params, s) for s in seen), label      # the parameters did change
        seen.append(params)
        pred, grads = outputs(used)
        fresh = _ffi_net.ConvNet(eng, max_chunk_samples=40)
        fresh.set_params(params)
        fpred, fgrads = outputs(fresh)
        fresh.close()
        for k in pred:
            assert np.array_equal(pred[k], fpred[k]), (label, k)
        assert np.array_equal(grads, fgrads) and np.abs(grads).max() > 0, label

    used.train_obs(*obs, act, adv, y, lr=0.0, apply_update=False)
    used.apply_grads(LR)
    check("apply_grads")
    used.train_obs(*obs, act, adv, y, lr=LR, apply_update=True)
    check("train_obs")
    rng = np.random.RandomState(8)
    used.set_params((seen[0] * (1 + 0.05 * rng.normal(size=seen[0].size))).astype(np.float32))
    check("set_params")
    path = str(tmp_path / "ckpt.npz")
    zero = np.zeros(seen[0].size, np.float32)
    np.savez(path, params=(seen[0] * (1 + 0.05 * rng.normal(size=seen[0].size))).astype(np.float32), adam_m=zero, adam_v=zero, adam_step=3,
             action_counter=0)
    used.load_checkpoint(path)
    check("load_checkpoint")
    assert used.get_optimizer_state()["adam_step"] == 3
    assert used.range_info() == {"gemm_f32": gemm == "f32", "fallbacks": 0, "update_skipped": False}
    used.close(); eng.close()
