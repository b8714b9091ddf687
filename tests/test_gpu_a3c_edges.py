"""GPU: the three A3C nets (csrc/net_gauss.hip, net_gated.hip, net_discrete.hip on the trunk of net_a3c_core.inc) against their float64
oracles where the heads are NOT comfortable and the windows are not plain tails: the cases of tests/_a3c_edge_cases.py (held to their
conditions on the CPU by tests/test_a3c_edge_cases.py), through the same predict / train(apply_update=False) / get_grads calls as
test_gpu_gaussnet.py, test_gpu_gatednet.py and test_gpu_discretenet.py.

Bounds.  Every comparison starts from the bound the kind's existing file holds (gradient blocks 1e-6 policy / 3e-7 value, gated 1e-6
both; forward rtol 5e-5 / atol 5e-6, gated 2e-4 / 2e-5; statistics rtol 1e-4) and is multiplied by
max(1, conditioning(case) / conditioning(plain)): what one float32 half-ulp on every parameter, state, window entry and raw action
does to the ORACLE's own result on the case, over the same on the plain case (the file's parameters and _samples).  Both figures come
from the oracle alone; none was tuned to a device figure.  Conditioning figures (largest of four sign patterns) and resulting bounds:

  plain      policy   value    statistics          mixed saturation  policy -> bound      value -> bound       statistics -> bound
  solow      1.84e-7  6.11e-8  3.84e-6             solow             3.68e-3 -> 1.99e-2   1.43e-6 -> 7.04e-6   1.18e-3 -> 3.08e-2
  trade      2.81e-7  6.13e-8  3.06e-7             trade             3.60e-4 -> 1.28e-3   2.79e-6 -> 1.37e-5   1.30e-4 -> 4.26e-2
  gated      8.40e-8  6.41e-8  1.80e-7             gated             1.50e-6 -> 1.79e-5   7.42e-6 -> 1.16e-4   4.33e-6 -> 2.40e-3
  discrete3  7.07e-8  2.39e-8  4.28e-8             discrete3         6.26e-8 -> 1.00e-6   3.81e-5 -> 4.78e-4   2.64e-5 -> 6.17e-2
  discrete64 4.23e-8  4.35e-8  8.10e-8             discrete64        4.32e-8 -> 1.02e-6   2.56e-5 -> 1.77e-4   1.92e-5 -> 2.37e-2
  (the Gaussian policy figures are those of sigma = 1e-3 next to |mu| = 5 under weight; the value and statistics figures those of
  static states of 10^3 .. 10^4 behind ReLUs.)  Forward ratios of the mixed cases: solow mu 112, sigma 14, values 20; trade 12 / 55 /
  6.8; gated probs 503, mu 65, sigma 169, values 53; discrete3 probs 1.2, values 177; discrete64 1.0 / 224.
  Exact saturation: the policy side has no tolerance (gated: the class tower; its normal tower and trunk at 1e-6 x ratio 1); the value
  gradient is held to the file's value bound and the statistics to rtol 1e-4 as they stand.
  Window edges: the plain parameters; the ratios are below 2 (asserted on the CPU) and the plain bounds are used.

Measured on the MI355X (worst gradient block error, policy / value; LABNOTES Y has the forward and statistics figures):
  mixed saturation   solow 5.17e-4 / 9.71e-7   trade 3.44e-4 / 3.10e-6   gated 1.79e-6 / 9.66e-6   discrete3 3.05e-7 / 2.56e-5
                     discrete64 1.55e-7 / 1.82e-5
  exact saturation   policy exactly 0 (gated: class tower 0, the rest 5.08e-8); value solow 8.09e-8, trade 4.87e-8, gated 3.19e-7,
                     discrete3 8.21e-8, discrete64 8.11e-8
  window edges       worst of R = 1 / 5 / 20: solow 2.91e-7 / 1.28e-7, trade 4.13e-7 / 7.99e-8, gated 1.31e-7 / 9.38e-8,
                     discrete3 2.76e-7 / 6.75e-8, discrete64 1.15e-7 / 6.75e-8
  batch edges        n = 1 / 64 / 65: solow 2.16e-3, 1.76e-5, 1.76e-5 / 1.95e-6, 5.17e-7, 5.39e-7; trade 6.79e-6, 5.26e-4, 5.26e-4 /
                     2.41e-6, 1.44e-6, 1.44e-6; gated 2.03e-7, 3.85e-6, 2.98e-6 / 1.27e-5, 1.29e-5, 1.29e-5; discrete (n = 64, 65) 1.31e-7
                     (K = 3), 1.26e-7 (K = 64) / 1.56e-5, 8.23e-6; at n = 1 the saturated discrete sample has no policy gradient
"""
import numpy as np
import pytest

import _a3c_edge_cases as EC
import _a3c_replay_checks as RC
import test_gpu_discretenet as TDI
import test_gpu_gatednet as TGT
import test_gpu_gaussnet as TGA

pytestmark = pytest.mark.gpu
KINDS = EC.KINDS
STATS = ("policy_loss", "value_loss", "entropy_mean")


def _engine(kind, E=64, **kw):
    sp = EC.spec(kind)
    if sp.family == "gauss":
        return TGA._engine(kind, E, **kw)
    return TGT._engine(E, **kw) if sp.family == "gated" else TDI._engine(E, **kw)


def _net(kind, eng, R, **kw):
    sp = EC.spec(kind)
    kw.setdefault("max_samples", 256)
    if sp.family == "gauss":
        return TGA._net(eng, rnn_length=R, **kw)
    return TGT._net(eng, rnn_length=R, **kw) if sp.family == "gated" else TDI._net(eng, rnn_length=R, num_choices=sp.K, **kw)


@pytest.fixture(scope="module")
def engs():
    made = {}

    def get(kind):
        fam = kind if kind in EC.GAUSS else EC.spec(kind).family
        if fam not in made:
            made[fam] = _engine(kind)
        return made[fam]
    yield get
    for e in made.values():
        e.close()


def _train(net, case, apply_update=False, lr=1e-3):
    st = net.train(case["states"], case["win"], *case["heads"], case["adv"], case["tgt"], case["wt"], grad_mult=case["mult"], lr=lr,
                   apply_update=apply_update)
    return st, net.get_grads("policy"), net.get_grads("value")


def _loaded(kind, engs, case, **kw):
    net = _net(kind, engs(kind), case["R"], **kw)
    net.set_params(case["flat"])
    return net


def _fwd_errs(sp, got, ref):
    return {k: float((np.abs(got[k] - ref[k]) / (sp.fwd_atol + sp.fwd_rtol * np.abs(ref[k]))).max()) for k in sp.outs}


def _check_ranges(sp, got):
    assert all(np.isfinite(v).all() for v in got.values())
    if sp.family == "gauss":
        one = np.float32(1.0)
        assert (np.abs(got["mu"]) <= 5).all() and (got["sigma"] >= np.float32(1e-3)).all() and (got["sigma"] <= one + np.float32(1e-3)).all()
        return
    p = got["probs"]
    assert (p >= 0).all() and (p <= 1).all() and np.abs(p.astype(np.float64).sum(-1) - 1.0).max() < 1e-6
    if sp.family == "gated":
        assert (got["sigma"] >= np.float32(1e-7)).all()


def _against_oracle(sp, case, net, b, label):
    """forward, both gradients and the statistics of the case against the oracle at the bounds b; returns the device's results"""
    got = net.predict(case["states"], case["win"])
    ref = EC.oracle_forward(case)
    ferr = _fwd_errs(sp, got, ref)
    print("%s %s forward error / (atol + rtol |ref|): %s; bounds %s" % (case["kind"], label, {k: "%.3g" % v for k, v in ferr.items()},
                                                                        {k: "%.3g" % v for k, v in b["fwd"].items()}))
    _check_ranges(sp, got)
    stats, gp, gv = _train(net, case)
    (pl, vl, ent), rp, rv = EC.oracle_grads(case)
    ep, bp = sp.block_err(gp, rp)
    ev, bv = sp.block_err(gv, rv)
    print("%s %s worst block error: policy %.3g (%s) bound %.3g, value %.3g (%s) bound %.3g" % (case["kind"], label, ep, bp, b["policy"], ev, bv,
                                                                                              b["value"]))
    srel = [abs(stats[k] - r) / abs(r) for k, r in zip(STATS, (pl, vl, ent))]
    nrel = [abs(stats[k] - np.linalg.norm(r)) / np.linalg.norm(r) for k, r in (("policy_norm", rp), ("value_norm", rv))]
    print("%s %s statistics relative error: losses %s norms %s bound %.3g" % (case["kind"], label, ["%.3g" % v for v in srel],
                                                                              ["%.3g" % v for v in nrel], b["stats"]))
    assert np.isfinite(gp).all() and np.isfinite(gv).all() and all(np.isfinite(v) for v in stats.values())
    assert all(ferr[k] <= b["fwd"][k] for k in sp.outs), ferr
    assert ep < b["policy"] and ev < b["value"], (ep, bp, ev, bv)
    assert not gp[~sp.pmask].any() and not gv[~sp.vmask].any()
    assert max(srel) <= b["stats"] and max(nrel) <= b["stats"], (srel, nrel)
    return got, stats, gp, gv, rp, rv


# ------------------------------------------------------------------------------------------ a. mixed saturation
@pytest.mark.parametrize("kind", KINDS)
def test_mixed_saturation_against_oracle(engs, kind):
    sp, case = EC.spec(kind), EC.mixed(kind)
    b = EC.bounds(case, "mixed")
    net = _loaded(kind, engs, case)
    got, stats, gp, gv, rp, rv = _against_oracle(sp, case, net, b, "mixed")
    # the bound still sees one 64-sample group go missing
    keep = np.ones(EC.N, bool); keep[64:128] = False
    _, mp, mv = EC.oracle_grads(EC.subset(case, keep))
    assert sp.block_err(mp, rp)[0] > b["policy"] and sp.block_err(mv, rv)[0] > b["value"]
    # a second call: the same bits
    stats2, gp2, gv2 = _train(net, case)
    net.close()
    assert np.array_equal(gp, gp2) and np.array_equal(gv, gv2) and stats == stats2
    # the device's heads are saturated where the oracle's are
    sat = case["saturated"]
    if sp.family == "gauss":
        edge = (np.abs(got["mu"]) == 5).any(1) | (got["sigma"] == np.float32(1e-3)).any(1) | (got["sigma"] == np.float32(1) + np.float32(1e-3)).any(1)
    else:
        edge = (got["probs"].reshape(EC.N, -1) == 0).any(1)
        if sp.family == "gated":
            edge |= (got["sigma"].reshape(EC.N, -1) == np.float32(1e-7)).any(1)
    print("%s: device heads exactly saturated in %d samples, oracle (float32 of float64) in %d" % (kind, edge.sum(), sat.sum()))
    assert edge.mean() >= 0.2 and not edge[case["comfortable"]].any()


# ------------------------------------------------------------------------------------------ b. exact saturation
@pytest.mark.parametrize("kind,variant", [(k, v) for k in KINDS for v in EC.EXACT_VARIANTS[k]])
def test_exact_saturation_has_no_policy_gradient(engs, kind, variant):
    sp, case = EC.spec(kind), EC.exact(kind, variant)
    b = EC.bounds(case, "exact " + variant)
    P = sp.num_params
    net = _loaded(kind, engs, case, clip_norm=0.5)
    net.set_optimizer_state(np.full(P, 2.0, np.float32), np.full(P, 3.0, np.float32), 200000)
    got = net.predict(case["states"], case["win"])
    _check_ranges(sp, got)
    lead = np.zeros(got["probs"].shape, bool) if sp.family != "gauss" else None
    if sp.family == "gauss":
        assert (got["mu"] == 5).all() and (got["sigma"] == (np.float32(1) if variant == "sigma_hi" else np.float32(0)) + np.float32(1e-3)).all()
    elif sp.family == "gated":
        for a, c in enumerate(EC.GATED_LEAD):
            lead[:, a, c] = True
    else:
        lead[:, sp.K - 2] = True
    if lead is not None:
        assert (got["probs"][lead] == 1).all() and (got["probs"][~lead] == 0).all()
    stats, gp, gv = _train(net, case)
    (pl, vl, ent), rp, rv = EC.oracle_grads(case)
    zero = sp.pmask & ~sp.vmask                                       # the policy towers
    if sp.family == "gated":                                          # the class tower only; the normal tower and the trunk at the case's bound
        r = sp.ranges
        zero = np.zeros(P, bool); zero[r["class1_w"][0]:r["class3_b"][1]] = True
        assert not gp[zero].any()
        ep, bp = sp.block_err(gp, rp)
        print("gated exact: policy worst block error %.3g (%s) bound %.3g" % (ep, bp, b["policy"]))
        assert ep < b["policy"] and gp[~zero].any()
    else:
        assert not gp.any()                                           # no tolerance: the heads' derivatives are exactly 0
    ev, bv = sp.block_err(gv, rv)
    print("%s exact %s: value worst block error %.3g (%s) bound %.3g; stats %s oracle %s" % (kind, variant, ev, bv, sp.grad_bound["value"], stats,
                                                                                            (pl, vl, ent)))
    assert ev < sp.grad_bound["value"] and not gv[~sp.vmask].any()
    assert all(np.isfinite(stats[k]) for k in stats)
    # Discrete head: float32(1 + 1e-7) is 1 + 2^-23, so log(p + 1e-7) at p = 1 carries the rounding of its argument, at most half
    # an ulp of 1 per sample -- a float32 statement's legitimate distance from the float64 one, next to losses of 1e-7 themselves
    half_ulp = 2.0 ** -24 if sp.family == "discrete" else 0.0
    cp = case["mult"] * case["wt"].astype(np.float64) * case["adv"]
    for k, ref, atol in zip(STATS, (pl, vl, ent), (half_ulp * np.abs(cp).sum(), 0.0, half_ulp)):
        np.testing.assert_allclose(stats[k], ref, rtol=1e-4, atol=atol, err_msg=k)
    # one update: where the policy gradient is exactly zero and the value gradient does not reach, no parameter moves
    _train(net, case, apply_update=True)
    after = net.get_params()
    st = net.get_optimizer_state()
    net.close()
    assert st["global_step"] == 200002
    assert np.array_equal(after[zero], case["flat"][zero]) and zero.sum() > 50000
    assert not np.array_equal(after[sp.vmask], case["flat"][sp.vmask])          # the value step did happen
    np.testing.assert_allclose(st["ms_policy"][zero], 0.99 * 2.0, rtol=1e-6)


# ------------------------------------------------------------------------------------------ c. window edges
@pytest.mark.parametrize("R", [1, EC.R0, EC.MAXR])
@pytest.mark.parametrize("kind", KINDS)
def test_window_edges_against_oracle(engs, kind, R):
    sp, case = EC.spec(kind), EC.windows(kind, R)
    r = EC.bounds(case, "windows R=%d" % R)["ratio"]
    assert r["policy"] < 2 and r["value"] < 2 and r["stats"] < 2 and max(r["fwd"].values()) < 2
    plain = {"policy": sp.grad_bound["policy"], "value": sp.grad_bound["value"], "stats": sp.stats_rtol, "fwd": {k: 1.0 for k in sp.outs}}
    net = _loaded(kind, engs, case)
    _against_oracle(sp, case, net, plain, "windows R=%d" % R)
    net.close()


# ------------------------------------------------------------------------------------------ d. batch edges
TINY = float(np.finfo(np.float32).tiny)


def _rotation(case, n):
    """n consecutive samples of the batch (cyclically), the first one the batch's first saturated sample with weight"""
    i0 = int(np.flatnonzero(case["saturated"] & (case["wt"] > 0))[0])
    return (i0 + np.arange(n)) % EC.N


@pytest.mark.parametrize("n", [1, 64, 65])
@pytest.mark.parametrize("kind", KINDS)
def test_batch_edges_of_the_mixed_batch(engs, kind, n):
    sp, full = EC.spec(kind), EC.mixed(kind)
    b = EC.bounds(full, "mixed")
    case = EC.subset(full, _rotation(full, n))
    net = _loaded(kind, engs, case)
    stats, gp, gv = _train(net, case)
    net.close()
    _, rp, rv = EC.oracle_grads(case)
    assert np.isfinite(gp).all() and np.isfinite(gv).all() and rv.any()
    ev, bv = sp.block_err(gv, rv)
    if np.abs(rp).max() > TINY:
        ep, bp = sp.block_err(gp, rp)
    else:       # a one-hot discrete row alone: p_j - [j == choice] vanishes or p_choice does, the oracle's whole policy gradient is
        # below float32's smallest normal number and the device's is exactly 0
        assert n == 1 and sp.family == "discrete" and not gp.any()
        ep, bp = 0.0, "below float32"
    print("%s n=%d worst block error: policy %.3g (%s) bound %.3g, value %.3g (%s) bound %.3g" % (kind, n, ep, bp, b["policy"], ev, bv, b["value"]))
    assert ep < b["policy"] and ev < b["value"], (ep, bp, ev, bv)


# ------------------------------------------------------------------------------------------ e. no weight at all
@pytest.mark.parametrize("kind", KINDS)
def test_no_weight_at_all(engs, kind):
    sp, case = EC.spec(kind), EC.no_weight(EC.mixed(kind))
    P = sp.num_params
    net = _loaded(kind, engs, case)
    net.set_optimizer_state(np.full(P, 2.0, np.float32), np.full(P, 3.0, np.float32), 200000)
    stats, gp, gv = _train(net, case)
    assert not gp.any() and not gv.any()
    assert stats["policy_loss"] == 0 and stats["value_loss"] == 0 and stats["entropy_mean"] == 0
    assert stats["policy_norm"] == 0 and stats["value_norm"] == 0
    _train(net, case, apply_update=True)
    after, st = net.get_params(), net.get_optimizer_state()
    net.close()
    assert np.array_equal(after, case["flat"])
    assert st["global_step"] == 200002
    np.testing.assert_allclose(st["ms_policy"][sp.pmask], 0.99 * 2.0, rtol=1e-6)
    np.testing.assert_allclose(st["ms_value"][sp.vmask], 0.99 * 3.0, rtol=1e-6)
    assert (st["ms_policy"][~sp.pmask] == 2.0).all() and (st["ms_value"][~sp.vmask] == 3.0).all()


# ------------------------------------------------------------------------------------------ f. inert lanes at saturation
@pytest.mark.parametrize("kind", KINDS)
def test_inert_lanes_at_saturation(engs, kind):
    """test_gpu_a3c_padding.py's construction on the mixed batch: 70 samples, then the same 70 followed by 58 others of weight 0
    whose states all carry the large factor (so their raw actions are far from their mu, over a collapsed sigma).  A 0 * inf in
    one of those lanes would be a NaN in the group's gradient."""
    sp, full = EC.spec(kind), EC.subset(EC.mixed(kind), slice(0, 128))
    few_n = 70
    full["wt"] = full["wt"].copy(); full["wt"][few_n - 1] = 1.0 if not full["dead"][few_n - 1] else 0.0; full["wt"][few_n:] = 0.0
    full["states"] = full["states"].copy()
    full["states"][few_n::2] *= np.float32(EC.MIXED[kind][0])          # the even ones had no factor yet
    few = EC.subset(full, slice(0, few_n))
    net = _loaded(kind, engs, full)
    a, b = net.predict(few["states"], few["win"]), net.predict(full["states"], full["win"])
    assert all(np.isfinite(v).all() for v in b.values())
    for k in a:
        assert np.array_equal(a[k], b[k][:few_n]), k
    (st_few, gp_few, gv_few), (st_full, gp_full, gv_full) = _train(net, few), _train(net, full)
    net.close()
    assert np.isfinite(gp_full).all() and np.isfinite(gv_full).all()
    assert np.abs(gp_few).max() > 0 and np.abs(gv_few).max() > 0
    assert np.array_equal(gp_few, gp_full) and np.array_equal(gv_few, gv_full)
    assert st_few == st_full


# ------------------------------------------------------------------------------------------ g. a short rollout at exact saturation
@pytest.mark.parametrize("kind,variant", [(k, v) for k in KINDS for v in EC.EXACT_VARIANTS[k]])
def test_rollout_at_exact_saturation(kind, variant):
    E, T, R = 65, 4, 3
    sp = EC.spec(kind)
    case = EC.exact(kind, variant)
    b = EC.bounds(case, "exact " + variant)
    flat, P = case["flat"], sp.num_params
    eng = _engine(kind, E, seed=21)
    net = _net(kind, eng, R, max_samples=T * E)
    net.set_params(flat)
    net.set_action_counter(1000)
    net.rollout(T)
    heads = {"gauss": ("raw", "mu", "sigma", "actions"), "gated": ("choices", "raw", "probs", "mu", "sigma"),
             "discrete": ("choices", "probs", "actions")}[sp.family]
    r = {k: net.read_rollout(k) for k in ("states", "windows", "values", "adv", "targets", "weights") + heads}
    assert net.get_action_counter() == 1000 + T and (r["weights"][R - 1:] > 0).any()
    # the recorded heads are the oracle's forward on the recorded states and windows, exactly saturated
    S, W = r["states"].reshape(T * E, sp.S0), r["windows"].reshape(T * E, R, sp.D)
    rec = dict(case, states=S, win=W)
    ref = EC.oracle_forward(rec)
    got = {k: r[k].reshape(ref[k].shape) for k in sp.outs}
    ferr = _fwd_errs(sp, got, ref)
    print("%s rollout forward error / (atol + rtol |ref|): %s; bounds %s" % (kind, ferr, b["fwd"]))
    assert all(ferr[k] <= b["fwd"][k] for k in sp.outs), ferr
    EC.check_exact(dict(rec, variant=variant))
    # raw, choices and actions: the oracle's act / choose on the recorded float32 heads and the oracle's draws
    ids = np.arange(E)
    if sp.family == "gauss":
        assert (r["mu"] == 5).all() and (r["sigma"] == (np.float32(1) if variant == "sigma_hi" else np.float32(0)) + np.float32(1e-3)).all()
        RC.gauss_acting(r, eng.cfg.seed, ids, 1000, tanh_action=(kind == "trade"), stride=1)
        head_args = (r["raw"].reshape(T * E, -1),)
    elif sp.family == "gated":
        RC.gated_acting(r, eng.cfg.seed, ids, 1000, stride=1)
        assert (r["choices"] == np.array(EC.GATED_LEAD)).all()
        head_args = (r["choices"].reshape(T * E, 2), r["raw"].reshape(T * E, 2))
    else:
        RC.discrete_acting(r, eng.cfg.seed, ids, 1000, sp.K)
        assert (r["choices"] == sp.K - 2).all()
        head_args = (r["choices"].reshape(T * E),)
    # train_rollout is train on the recorded samples
    s1 = net.train_rollout(lr=1e-3)
    g_ro = net.get_grads("policy"), net.get_grads("value")
    p_ro = net.get_params()
    net.set_params(flat)
    net.set_optimizer_state(np.ones(P, np.float32), np.ones(P, np.float32), 0)
    s2 = net.train(S, W, *head_args, r["adv"].reshape(-1), r["targets"].reshape(-1), r["weights"].reshape(-1), grad_mult=1.0 / E, lr=1e-3)
    assert np.array_equal(net.get_grads("policy"), g_ro[0]) and np.array_equal(net.get_grads("value"), g_ro[1])
    assert np.array_equal(net.get_params(), p_ro) and g_ro[1].any()
    assert s1["policy_norm"] == s2["policy_norm"] and s1["value_norm"] == s2["value_norm"]
    if sp.family != "gated":
        assert not g_ro[0].any()
    net.close(); eng.close()
