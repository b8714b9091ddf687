"""CPU: the model behind the ARMA-state optimal-savings yardstick (include/goldsrl_solowarmadp.h).  The forecasts f = Mz zv + Me ev
iterated by f' = A f + b eps must be the shock of oracle/'s Solow recursion; the binding's derivation and look-up must be the
restatement's (tests/_solow_arma_dp_oracle.py) bit for bit; orders outside p >= 1, m <= 4 are refused by the grid builder."""
import numpy as np
import pytest

import _solow_arma_dp_oracle as AO
from oracle import oracle as O

ORDERS = [(1, 0), (1, 1), (1, 2), (3, 1), (2, 2), (3, 3)]


@pytest.mark.parametrize("p,q", ORDERS)
def test_state_space_follows_the_env_recursion(p, q):
    rho_z, rho_e = O.solow_rhos(p, q)
    A, b, Mz, Me = AO.model(rho_z, rho_e)
    rng = np.random.RandomState(10 * p + q)
    E, z, e = 3, rng.normal(scale=0.1, size=(3, p)), rng.normal(scale=0.1, size=(3, len(rho_e)))
    k = np.full(E, 50.0)
    f = z @ Mz.T + e @ Me.T
    assert f.shape == (E, max(p, len(rho_e) + 1))
    worst = 0.0
    for _ in range(200):
        eps = rng.normal(scale=0.1, size=E)
        k, z, e, _, _ = O.solow_step(k, z, e, eps, np.full(E, 0.3), rho_z, rho_e)
        f = f @ A.T + eps[:, None] * b[None, :]
        worst = max(worst, float(np.abs(f[:, 0] - z[:, -1]).max()), float(np.abs(f - (z @ Mz.T + e @ Me.T)).max()))
    assert worst <= 1e-12, worst


@pytest.mark.parametrize("p,q", ORDERS)
def test_binding_restates_the_oracle(p, q):
    from goldsrl import _ffi_solowarmadp as F
    grid = F.solow_arma_dp_grid(p, q, nk=6, nx=(4, 3, 2, 3)[:max(p, max(q, 1) + 1)], sigma=0.1)
    got = grid["model"]
    A, b, Mz, Me = AO.model(*F.handle_rhos(p, q))
    for name, want in (("A", A), ("b", b), ("Mz", Mz), ("Me", Me), ("f_std", AO.f_std(A, b, 0.1))):
        assert got[name].tobytes() == want.tobytes(), name
    assert grid["x_max"] == [3.0 * s for s in got["f_std"]]
    rng = np.random.RandomState(p + q)
    table = rng.uniform(size=F.table_shape(grid, 1)[1:]).astype(np.float32)
    k, zv, ev = rng.uniform(2.0, 600.0, size=50), rng.normal(scale=0.2, size=(50, p)), rng.normal(scale=0.2, size=(50, got["q"]))
    assert F.solow_arma_dp_policy_actions(grid, table, k, zv, ev).tobytes() == AO.lookup(grid, table, Mz, Me, k, zv, ev).tobytes()
    node = tuple(n - 1 for n in grid["nx"]) + (0,)               # far outside the box: the corner's entry itself
    far = AO.lookup(grid, table, Mz, Me, np.array([1e-3]), np.full((1, p), 50.0), np.zeros((1, got["q"])))
    assert far[0] == table[node]


@pytest.mark.parametrize("p,q", [(0, 1), (5, 1), (1, 4), (4, 4)])
def test_builder_refuses_what_the_grid_cannot_hold(p, q):
    from goldsrl import _ffi_solowarmadp as F
    with pytest.raises(ValueError, match="m = max"):
        F.solow_arma_dp_grid(p, q)
