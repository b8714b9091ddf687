"""`python -m goldsrl.scripts.optimal_solow` -- floor, ceiling and gap of an eval registration of the Solow env: the best constant
savings rate (the reference's scripts/constant_solow.py, one kernel launch) and the optimal policy by backward induction on a
(k, z, e) grid (one launch per stage, then every env's episode in one launch), both on the same N seeded eval episodes.  The
gap is what there was to learn: a trained policy's eval/mean_total_reward is read as a share of it.  The reference has no
counterpart of the ceiling."""
import argparse
import json

from goldsrl import _ffi_solowdp
from goldsrl.agents.a3c.policy_monitor import make_eval_engine
from goldsrl.baselines import ConstantSavingsBaseline, OptimalSavingsBaseline


def get_arg_parser():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--env", default="Solow-1-1-finite-eval-v0", help="Solow-1-q-finite-eval-v0 with q 0 or 1")
    p.add_argument("--envs", type=int, default=1, help="seeded eval episodes (env 0 is the reference's single one)")
    p.add_argument("--grid", nargs=4, type=int, metavar=("NK", "NZ", "NQ", "NS"), default=(96, 25, 7, 96),
                   help="points in k, z, quadrature nodes, savings rates")
    p.add_argument("--horizon", type=int, default=_ffi_solowdp.DEFAULT_HORIZON, help="stages of the induction")
    p.add_argument("--json", help="write the figures to this file")
    p.add_argument("--device", type=int, default=0)
    return p


def main(argv=None):
    parser = get_arg_parser()
    args = parser.parse_args(argv)
    if args.envs < 1 or args.horizon < 1:
        parser.error("--envs and --horizon need a value >= 1")
    eng = make_eval_engine(args.env, args.envs, args.device)
    nk, nz, nq, ns = args.grid
    grid = _ffi_solowdp.solow_dp_grid(nk=nk, nz=nz, nq=nq, ns=ns, sigma=eng.cfg.solow_sigma)
    floor_rate, floor = ConstantSavingsBaseline(engine=eng).best_total()
    ceiling = OptimalSavingsBaseline(engine=eng, grid=grid, horizon=args.horizon).total()
    record = {"env": args.env, "n_envs": args.envs, "grid": [nk, nz, nq, ns], "horizon": args.horizon, "floor_rate": float(floor_rate),
              "floor": floor, "ceiling": ceiling, "gap": ceiling - floor}
    print("%s, %d env(s): floor %.6f (constant rate %.6g)  ceiling %.6f (grid %dx%dx%d, %d actions, %d stages)  gap %.6f"
          % (args.env, args.envs, floor, floor_rate, ceiling, nk, nz, nq, ns, args.horizon, ceiling - floor))
    eng.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f)
    return record


if __name__ == "__main__":
    main()
