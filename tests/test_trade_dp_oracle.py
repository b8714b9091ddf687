"""CPU: the numpy restatement of the TradeAR1 induction (tests/_trade_dp_oracle.py) in its n = 1 form against a loop over scalars
written from include/goldsrl_tradedp.h, on a 3 x 3 grid whose edge nodes leave the price axis, and the action look-up of
goldsrl/_ffi_tradedp.py at nodes, where it is the table's entry."""
import math

import numpy as np

import _trade_dp_oracle as TO


def _scalar_stage(grid, V):
    nu, nx, na, nq, xm = grid["nu"], grid["nx"], grid["na"], grid["nq"], grid["x_max"]
    dx = 2.0 * xm / (nx - 1)

    def look(u, xp):                                                     # bilinear, clamped
        pu, px = min(max(u * (nu - 1), 0.0), nu - 1.0), min(max((xp + xm) / dx, 0.0), nx - 1.0)
        iu, jx = min(int(pu), nu - 2), min(int(px), nx - 2)
        fu, fx = pu - iu, px - jx
        lo = (1 - fx) * V[iu][jx] + fx * V[iu][jx + 1]
        hi = (1 - fx) * V[iu + 1][jx] + fx * V[iu + 1][jx + 1]
        return (1 - fu) * lo + fu * hi

    out, pol = np.zeros((nu, nx)), np.zeros((nu, nx))
    for iu in range(nu):
        for jx in range(nx):
            u, x, best = iu / (nu - 1.0), -xm + jx * dx, -math.inf
            for ia in range(na):
                a = (2 * ia - (na - 1)) / (na - 1.0)
                up = u + a * (1.0 - u) if a > 0 else u * (1.0 + a)
                q = 0.0
                for k in range(nq):
                    xp = 0.9 * x + grid["e_nodes"][k]
                    g = (1.0 - up) + up * math.exp(xp - x)
                    q += grid["e_weights"][k] * (math.log(g) + look(up * math.exp(xp - x) / g, xp))
                if q > best:
                    best, pol[iu, jx] = q, a
            out[iu, jx] = best
    return out, pol


def test_oracle_n1_is_the_scalar_loop():
    from goldsrl._ffi_tradedp import trade_dp_grid
    grid = trade_dp_grid(nu=3, nx=3, na=3, nq=2, x_max=0.05, std_p=0.2)
    assert 0.9 * 0.05 + grid["e_nodes"][1] > 0.05                        # the edge node's move leaves the axis: the clamp is hit
    V = np.zeros((3, 3))
    for _ in range(3):
        want, want_pol = _scalar_stage(grid, V)
        got, got_pol = TO.stage(grid, 1, V)
        assert np.abs(got - want).max() <= 1e-14 and np.array_equal(got_pol[..., 0], want_pol.astype(np.float32))
        V = got
    assert V.max() > 1e-3 and len(np.unique(got_pol)) > 1               # there is something to earn and to decide
    pol, top = TO.solve(grid, 1, 3)
    assert np.array_equal(top, V) and pol.shape == (3, 3, 3, 1)


def test_actions_at_nodes_are_the_tables_entries():
    from goldsrl._ffi_tradedp import trade_dp_actions, trade_dp_grid
    grid = trade_dp_grid(nu=3, nx=3, na=3, nq=2, x_max=0.1)
    table = np.random.RandomState(0).uniform(-1, 1, size=(4, 3, 3, 3, 3, 2)).astype(np.float32)
    p = np.exp(np.array([[-0.1, 0.0], [0.1, 0.1], [5.0, -5.0]]))         # nodes (0, 1), (2, 2) and, clamped, (2, 0)
    q = np.array([[0.0, 50.0], [50.0, 50.0], [0.0, 0.0]]) / p            # shares (0, 1/2), (1/2, 1/2) and (0, 0) of W = 100
    cash = np.array([50.0, 0.0, 100.0])
    got = trade_dp_actions(table, grid, 4, cash, q, p, remaining=np.array([3, 9, 1]))
    assert np.abs(got[0] - table[1, 0, 1, 0, 1]).max() <= 2.0 ** -23     # two moves left: row 1
    assert np.abs(got[1] - table[3, 1, 1, 2, 2]).max() <= 2.0 ** -23     # eight moves left: the top row
    assert (got[2] == 0).all()                                           # the last step: nothing left to earn
    assert np.array_equal(trade_dp_actions(table, grid, 4, cash, q, p, None)[2], table[3, 0, 0, 2, 0])
