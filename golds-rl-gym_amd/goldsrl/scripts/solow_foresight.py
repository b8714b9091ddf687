"""`python -m goldsrl.scripts.solow_foresight` -- floor, induction and foresight ceiling of an eval registration of the Solow env,
side by side on the same N seeded eval episodes: the best constant savings rate (one launch), the optimal non-anticipating policy
by backward induction where the order has one (m = max(p, q + 1) <= 4), and the plan of a saver who knows the episode's shock path
(include/goldsrl_solowforesight.h: every order, one launch).  What lies between the induction and the ceiling is the price of not
knowing the shocks; the ceiling's played total and the grid's own value V_0(k_0) bracket the true ceiling on the paths measured.
The reference has no counterpart of either figure."""
import argparse
import json

from goldsrl.agents.a3c.policy_monitor import make_eval_engine
from goldsrl.baselines import ConstantSavingsBaseline, OptimalSavingsBaseline, SolowForesightCeiling
from goldsrl._ffi_solowforesight import solow_foresight_grid


def get_arg_parser():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--env", default="Solow-1-1-finite-eval-v0", help="Solow-p-q-finite-eval-v0")
    p.add_argument("--orders", nargs=2, type=int, metavar=("P", "Q"), default=None, help="the orders, in place of --env")
    p.add_argument("--envs", type=int, default=64, help="seeded eval episodes")
    p.add_argument("--grid", nargs=2, type=int, metavar=("NK", "NS"), default=(96, 96), help="points in k, savings rates")
    p.add_argument("--no-induction", action="store_true", help="skip the induction where the order has one")
    p.add_argument("--json", help="write the figures to this file")
    p.add_argument("--device", type=int, default=0)
    return p


def main(argv=None):
    parser = get_arg_parser()
    args = parser.parse_args(argv)
    if args.envs < 1:
        parser.error("--envs needs a value >= 1")
    env = args.env if args.orders is None else "Solow-%d-%d-finite-eval-v0" % tuple(args.orders)
    eng = make_eval_engine(env, args.envs, args.device)
    rate, floor = ConstantSavingsBaseline(engine=eng).best_total()
    top = SolowForesightCeiling(engine=eng, grid=solow_foresight_grid(eng, nk=args.grid[0], ns=args.grid[1]))
    record = {"env": env, "n_envs": args.envs, "grid": list(args.grid), "k_range": [top.grid["k_lo"], top.grid["k_hi"]],
              "floor_rate": float(rate), "floor": floor, "induction": None, "ceiling": top.ceiling(), "grid_value": top.value(),
              "clamped_steps": int(top.stats["clamped"].sum())}
    cfg = eng.cfg
    if not args.no_induction and max(cfg.solow_p, max(cfg.solow_q, 1) + 1) <= 4:
        record["induction"] = OptimalSavingsBaseline(engine=eng).total()
    eng.close()
    middle = "induction none (m > 4)" if record["induction"] is None else "induction %.6f" % record["induction"]
    print("%s, %d env(s): floor %.6f (constant rate %.6g)  %s  ceiling %.6f (V_0(k_0) %.6f, %d x %d, %d steps outside the k range)"
          % (env, args.envs, floor, rate, middle, record["ceiling"], record["grid_value"], args.grid[0], args.grid[1], record["clamped_steps"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f)
    return record


if __name__ == "__main__":
    main()
