"""`python -m goldsrl.scripts.optimal_solow` -- floor, ceiling and gap of an eval registration of the Solow env: the best constant
savings rate (the reference's scripts/constant_solow.py, one kernel launch) and the optimal policy by backward induction (one
launch per stage, then every env's episode in one launch), both on the same N seeded eval episodes.  Solow-1-q with q 0 or 1 is
solved on a (k, z, e) grid; every other order on the m = max(p, q + 1) forecasts of the ARMA shock (m <= 4).  The gap is what there
was to learn: a trained policy's eval/mean_total_reward is read as a share of it.  --orders prints the scale for (1,1), (2,2) and
(3,3), as the reference's constant_solow prints its three floors.  The reference has no counterpart of the ceiling."""
import argparse
import json

from goldsrl import _ffi_solowarmadp, _ffi_solowdp
from goldsrl.agents.a3c.policy_monitor import make_eval_engine
from goldsrl.baselines import ConstantSavingsBaseline, OptimalSavingsBaseline

ORDERS = ("Solow-1-1-finite-eval-v0", "Solow-2-2-finite-eval-v0", "Solow-3-3-finite-eval-v0")


def get_arg_parser():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--env", default="Solow-1-1-finite-eval-v0", help="Solow-p-q-finite-eval-v0")
    p.add_argument("--orders", action="store_true", help="the three orders the reference's constant_solow prints, in place of --env")
    p.add_argument("--envs", type=int, default=1, help="seeded eval episodes (env 0 is the reference's single one)")
    p.add_argument("--grid", nargs=4, type=int, metavar=("NK", "NX", "NQ", "NS"), default=None,
                   help="points in k, in z (per forecast axis for the ARMA-state grid), quadrature nodes, savings rates "
                        "(default 96 25 7 96 for Solow-1-0 and 1-1, 48 9 3 48 otherwise)")
    p.add_argument("--horizon", type=int, default=None, help="stages of the induction (default 256 for Solow-1-0 and 1-1, 128 otherwise)")
    p.add_argument("--json", help="write the figures to this file")
    p.add_argument("--device", type=int, default=0)
    return p


def scale(env, n_envs, sizes, horizon, device):
    """floor, ceiling and gap of one registration, printed and returned as a record"""
    eng = make_eval_engine(env, n_envs, device)
    grid = None
    if sizes is not None:
        nk, nx, nq, ns = sizes
        if eng.cfg.solow_p == 1 and eng.cfg.solow_q <= 1:
            grid = _ffi_solowdp.solow_dp_grid(nk=nk, nz=nx, nq=nq, ns=ns, sigma=eng.cfg.solow_sigma)
        else:
            grid = _ffi_solowarmadp.engine_grid(eng, nk=nk, nx=nx, nq=nq, ns=ns)
    floor_rate, floor = ConstantSavingsBaseline(engine=eng).best_total()
    b = OptimalSavingsBaseline(engine=eng, grid=grid, horizon=horizon)
    ceiling = b.total()
    total = b.stats["total"]
    nx = b.grid["nx"][0] if "nx" in b.grid else b.grid["nz"]
    record = {"env": env, "n_envs": n_envs, "grid": [b.grid["nk"], nx, b.grid["nq"], b.grid["ns"]], "horizon": b.horizon,
              "floor_rate": float(floor_rate), "floor": floor, "ceiling": ceiling, "gap": ceiling - floor,
              "ceiling_standard_error": float(total.std(ddof=1) / len(total) ** 0.5) if len(total) > 1 else None}
    print("%s, %d env(s): floor %.6f (constant rate %.6g)  ceiling %.6f (grid %dx%dx%d, %d actions, %d stages)  gap %.6f"
          % ((env, n_envs, floor, floor_rate, ceiling) + tuple(record["grid"]) + (b.horizon, ceiling - floor)))
    eng.close()
    return record


def main(argv=None):
    parser = get_arg_parser()
    args = parser.parse_args(argv)
    if args.envs < 1 or (args.horizon is not None and args.horizon < 1):
        parser.error("--envs and --horizon need a value >= 1")
    records = [scale(env, args.envs, args.grid, args.horizon, args.device) for env in (ORDERS if args.orders else (args.env,))]
    record = {"orders": records} if args.orders else records[0]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f)
    return record


if __name__ == "__main__":
    main()
