"""CPU: the float64 restatement of the backward induction (tests/_solow_dp_oracle.py) and the numpy helpers of
goldsrl/_ffi_solowdp.py -- the last stage consumes everything, the quadrature weights sum to 1, the look-up is exact on the grid
points and clamps outside, and on the reference's seeded eval episode the induction's policy stands well above the best constant
savings rate."""
import numpy as np
import pytest

import _solow_dp_cases as DC
import _solow_dp_oracle as DO


def test_last_stage_policy_is_the_lowest_rate():
    from goldsrl._ffi_solowdp import solow_dp_grid
    g = solow_dp_grid(nk=6, nz=4, nq=3, ns=9)
    for ne, theta in ((3, DC.THETA), (1, 0.0)):
        policy, value, gap = DO.solve(g, 40, DC.RHO, theta, DC.DELTA, ne)
        assert policy.shape == (40, 6, 4, ne) and value.shape == (6, 4, ne) and policy.dtype == np.float32
        assert (policy[-1] == np.float32(g["s_lo"])).all()                # nothing follows: consume
        assert (policy[0] > np.float32(g["s_lo"])).any() and gap >= 0.0
    one, value1, _ = DO.solve(g, 1, DC.RHO, DC.THETA, DC.DELTA, 3)
    ax = DO.axes(g, 3)
    want = np.log((1.0 - g["s_lo"]) * (np.exp(ax["z"])[None, :] * ax["k"][:, None] ** 0.33) + 1e-4)
    assert np.array_equal(value1, np.repeat(want[:, :, None], 3, axis=2))


@pytest.mark.parametrize("nq", [1, 2, 3, 7, 15])
def test_grid_weights_sum_to_one(nq):
    from goldsrl._ffi_solowdp import solow_dp_grid
    g = solow_dp_grid(nq=nq, sigma=0.1)
    assert g["e_weights"].shape == (nq,) and g["e_weights"].dtype == np.float64 and abs(g["e_weights"].sum() - 1.0) <= 4e-16 * nq
    assert (np.diff(g["e_nodes"]) > 0).all() and abs((g["e_weights"] * g["e_nodes"] ** 2).sum() - (0.01 if nq > 1 else 0.0)) < 1e-15
    with pytest.raises(ValueError):
        solow_dp_grid(nq=16)
    d = solow_dp_grid()
    assert (d["nk"], d["nz"], d["nq"], d["ns"], d["k_lo"], d["k_hi"], d["z_max"], d["s_lo"], d["s_hi"]) == (96, 25, 7, 96, 5.0, 400.0, 1.6, 0.001, 0.999)


def test_policy_actions_on_the_grid_and_outside():
    from goldsrl._ffi_solowdp import solow_dp_grid, solow_dp_policy_actions
    g = solow_dp_grid(nk=5, nz=4, nq=3, ns=4, k_lo=8.0, k_hi=128.0, z_max=0.75)
    tab = np.random.RandomState(0).uniform(size=(5, 4, 3)).astype(np.float32)
    k = np.array([8.0, 16.0, 128.0, 1.0, 1e4, 16.0, 16.0])               # k_i = 8 * 2^i, z_i = -0.75 + 0.5 i: exact in float64
    z = np.array([-0.75, -0.25, 0.75, -0.75, 0.75, -9.0, 9.0])
    e = np.array([g["e_nodes"][0], g["e_nodes"][1], g["e_nodes"][2], -1.0, 1.0, g["e_nodes"][1], g["e_nodes"][1]])
    got = solow_dp_policy_actions(g, tab, k, z, e)
    assert got.dtype == np.float32
    want = np.array([tab[0, 0, 0], tab[1, 1, 1], tab[4, 3, 2], tab[0, 0, 0], tab[4, 3, 2], tab[1, 0, 1], tab[1, 3, 1]])
    assert np.allclose(got, want, rtol=0, atol=2e-7)                       # log(16) - log(8) is a rounded log 2
    mid = solow_dp_policy_actions(g, tab, [8.0], [-0.5], [0.5 * g["e_nodes"][0]])
    assert abs(mid[0] - 0.25 * (tab[0, 0, 0] + tab[0, 1, 0] + tab[0, 0, 1] + tab[0, 1, 1])) < 2e-7
    flat = solow_dp_policy_actions(g, tab[:, :, :1], k, z, e)               # q = 0: one plane, e is ignored
    assert np.allclose(flat, [tab[0, 0, 0], tab[1, 1, 0], tab[4, 3, 0], tab[0, 0, 0], tab[4, 3, 0], tab[1, 0, 0], tab[1, 3, 0]], rtol=0, atol=2e-7)


def test_oracle_clears_the_constant_floor_on_the_seeded_episode():
    """The seeded eval episode of Solow-1-1-finite-eval-v0 in numpy float64.  Measured: the induction's policy on 32 x 9 x 3,
    32 actions, 128 stages totals 931.16, the best of the reference's 20 constant rates (0.334) 879.05."""
    from goldsrl._ffi_solowdp import solow_dp_grid, solow_dp_policy_actions
    from goldsrl.baselines import REFERENCE_RATES
    z0, es = DC.seeded_shocks()
    g = solow_dp_grid(sigma=DC.SIGMA, **DC.FLOOR_GRID)
    policy, _, _ = DO.solve(g, DC.FLOOR_HORIZON, DC.RHO, DC.THETA, DC.DELTA, g["nq"])
    floor = max(DO.episode(z0, es, DC.STEPS, DC.DELTA, DC.RHO, DC.THETA, lambda t, k, z, e: s).sum() for s in REFERENCE_RATES)

    def rule(t, k, z, e):
        stage = max(0, DC.FLOOR_HORIZON - (DC.STEPS - t))
        return solow_dp_policy_actions(g, policy[stage], [k], [z], [e])[0]

    ceiling = DO.episode(z0, es, DC.STEPS, DC.DELTA, DC.RHO, DC.THETA, rule).sum()
    print("floor %.4f ceiling %.4f" % (floor, ceiling))
    assert ceiling >= floor + DC.MARGIN, (floor, ceiling)


def test_optimal_flag_needs_the_eval_envs():
    from goldsrl.scripts import train_paac_solow, train_solow, train_solow_grid
    for script in (train_solow, train_solow_grid, train_paac_solow):
        with pytest.raises(SystemExit):
            script.parse_args(["--optimal"])
        args = script.parse_args(["--optimal", "--eval-envs", "3"])
        assert args.optimal and not args.baseline
        assert not script.parse_args([]).optimal
