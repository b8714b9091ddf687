"""What the CPU and the GPU tests of the optimal-savings yardstick share: the model of the eval registration, the seeded eval
episode's shocks, the grids."""
import numpy as np

DELTA, SIGMA = 0.02, 0.1                              # SolowEnv's defaults
RHO, THETA = float(np.float32(0.95)), 0.5             # rho_z[0], rho_e[0] of p = 1, q = 1 as the float32 env holds them
STEPS = 1024                                          # the eval registration's TimeLimit
FLOOR_GRID = dict(nk=32, nz=9, nq=3, ns=32)           # the grid the floor-and-ceiling checks solve on
FLOOR_HORIZON = 128
MARGIN = 40.0                                         # the least the ceiling must stand above the floor


def seeded_shocks(T=2048):
    """z0 and es of `Solow-1-1-finite-eval-v0` (seed 1692) as SolowEnv._reset draws them: z = normal(scale=sigma, size=(p,)), then
    es = normal(0, sigma, (T,)); es is popped from the end."""
    rs = np.random.RandomState(1692)
    z0 = rs.normal(scale=SIGMA, size=(1,))
    es = rs.normal(0, SIGMA, (T,))
    return float(z0[0]), es
