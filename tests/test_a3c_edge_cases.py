"""CPU: the builders of tests/_a3c_edge_cases.py hold their conditions, the float64 oracles are finite on every case (warnings are
errors) and the conditioning figures that size the bounds of tests/test_gpu_a3c_edges.py are printed next to the plain case's."""
import warnings

import numpy as np
import pytest

import _a3c_edge_cases as EC


def _finite(case, label, bounds=True):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        stats, gp, gv = EC.oracle_grads(case)
        fwd = EC.oracle_forward(case)
        assert np.isfinite(stats).all() and np.isfinite(gp).all() and np.isfinite(gv).all(), label
        assert all(np.isfinite(v).all() for v in fwd.values()), label
        if not bounds:
            return stats, gp, gv
        b = EC.bounds(case, label)
    assert all(np.isfinite(b[k]) and b[k] > 0 for k in ("policy", "value", "stats"))
    return b, gp, gv


@pytest.mark.parametrize("kind", EC.KINDS)
def test_mixed_saturation_case(kind):
    case = EC.mixed(kind)
    sp = EC.spec(kind)
    n = len(case["wt"])
    assert n == EC.N == 130 and case["R"] == 5 and case["flat"].dtype == np.float32 and case["states"].dtype == np.float32
    sat, ok = EC.classes(case)
    print("%s: saturated %.0f %%, comfortable %.0f %%, weight 0 by the choice rule %d" % (kind, 100 * sat.mean(), 100 * ok.mean(), case["dead"].sum()))
    assert sat.mean() >= 0.2 and ok.mean() >= 0.2
    for m in (sat, ok):
        assert (case["wt"][m] == 0).any() and (case["wt"][m] > 0).any() and (case["adv"][m] < 0).any() and (case["adv"][m] > 0).any()
    assert EC.MIXED[kind][0] in ((30.0, 300.0) if kind in EC.GAUSS else (1e3, 1e4)) and EC.MIXED[kind][1] in (None, 8.0, 16.0, 32.0)
    f = EC.oracle_forward(case)
    if sp.family == "gauss":
        z = (case["heads"][0] - f["mu"]) / f["sigma"]
        assert np.abs(z).max() < 6                                       # (raw - mu) / sigma of order 1
    if sp.family == "gated":
        ch, raw = case["heads"]
        idx = np.arange(n)[:, None], np.arange(2)[None, :]
        assert (f["probs"][idx + (ch,)].astype(np.float32) >= 1e-30).all()
        live = case["wt"] > 0
        assert (np.abs(f["mu"][idx + (ch,)]) <= EC.GATED_MU_OVER_SIGMA * f["sigma"][idx + (ch,)])[live].all()
        assert (np.abs((raw - f["mu"][idx + (ch,)]) / f["sigma"][idx + (ch,)]) < 6)[live].all()
        collapsed = (f["sigma"][idx + (ch,)].astype(np.float32) == np.float32(1e-7)).any(1)
        assert collapsed.any() and not case["wt"][collapsed].any()       # d^2 / sigma^3 at sigma = 1e-7 stands next to cp = 0 only
    b, gp, gv = _finite(case, "mixed")
    # the bound still sees one 64-sample group go missing
    keep = np.ones(n, bool); keep[64:128] = False
    _, mp, mv = EC.oracle_grads(EC.subset(case, keep))
    assert sp.block_err(mp, gp)[0] > b["policy"] and sp.block_err(mv, gv)[0] > b["value"]
    stats, gp, gv = _finite(EC.no_weight(case), "mixed, no weight", bounds=False)
    assert not stats.any() and not gp.any() and not gv.any()


@pytest.mark.parametrize("kind,variant", [(k, v) for k in EC.KINDS for v in EC.EXACT_VARIANTS[k]])
def test_exact_saturation_case(kind, variant):
    case = EC.exact(kind, variant)
    EC.check_exact(case)
    sp = EC.spec(kind)
    assert (case["wt"] == 0).any() and (case["wt"] > 0).any() and (case["adv"] < 0).any() and (case["adv"] > 0).any()
    plain = sp.as64(sp.params())
    shifted = sp.as64(case["flat"])
    moved = {k for k in plain if not np.array_equal(plain[k], shifted[k])}
    assert moved == {"gauss": {"mu3_b", "sigma3_b"}, "gated": {"class3_b"}, "discrete": {"probs3_b"}}[sp.family]
    _finite(case, "exact " + variant)


@pytest.mark.parametrize("R", [1, EC.R0, EC.MAXR])
@pytest.mark.parametrize("kind", EC.KINDS)
def test_window_edge_case(kind, R):
    case = EC.windows(kind, R)
    pats = EC.window_patterns(R)
    count = np.array([pats[k].sum() for k in case["pattern"]])
    assert set(count[case["pattern"] <= R]) == set(range(R + 1)) and len(pats) == R + 1 + (2 if R >= 3 else 0)
    assert np.array_equal(EC.oracle_length(case), count)
    nonzero = np.abs(case["win"]).max(2) > 0
    assert np.array_equal(nonzero.sum(1), count)
    if R >= 3:
        for k, rows in ((R + 1, [0, 2]), (R + 2, [1, 2])):
            m = case["pattern"] == k
            assert (case["wt"][m] > 0).any() and (np.flatnonzero(nonzero[m][0]) == rows).all() and (count[m] == 2).all()
    b, _, _ = _finite(case, "windows R=%d" % R)
    r = b["ratio"]
    print("%s R=%d: conditioning ratios policy %.3g value %.3g stats %.3g forward %.3g" % (kind, R, r["policy"], r["value"], r["stats"],
                                                                                             max(r["fwd"].values())))
    # the plain parameters: the ratio is 1 up to the figure's scatter (EC.WINDOW_SEED), and the GPU test uses the plain bounds
    assert r["policy"] < 2 and r["value"] < 2 and r["stats"] < 2 and max(r["fwd"].values()) < 2


@pytest.mark.parametrize("kind", EC.KINDS)
def test_plain_case_is_the_existing_files(kind):
    case = EC.plain(kind)
    sp = EC.spec(kind)
    assert np.array_equal(case["flat"], sp.params()) and len(case["wt"]) == sp.plain_n and case["mult"] == 0.3
    c = EC.plain_conditioning(kind)
    print("%s plain: conditioning policy %.3g value %.3g stats %.3g fwd %s" % (kind, c["policy"], c["value"], c["stats"],
                                                                               {k: "%.3g" % v for k, v in c["fwd"].items()}))
    # one half-ulp per number cannot move the reference by more than the bound the device is held to at these parameters
    assert c["policy"] < sp.grad_bound["policy"] and c["value"] < sp.grad_bound["value"] and all(v < 1 for v in c["fwd"].values())
