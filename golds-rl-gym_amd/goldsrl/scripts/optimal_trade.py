"""`python -m goldsrl.scripts.optimal_trade` -- the four-point scale of TradeAR1 on one set of N seeded envs: the best default
trading rule, the tuned four-number rule (fitted on other seeds, played here), the attainable optimum -- the env's own stochastic
model solved by backward induction on a (shares, log prices) grid, one launch per stage, and the table played on the envs in one
launch -- and the foresight ceiling of the trader who knows the coming prices.  What lies between the optimum and the ceiling is
closed to every trader that cannot see ahead; what lies below the optimum is what there is to learn.  1 or 2 assets.  The
reference has no counterpart."""
import argparse
import json

import numpy as np

from goldsrl import _ffi, _ffi_tradedp
from goldsrl.agents.a3c.policy_monitor import TRADE_TUNE_SEED
from goldsrl.baselines import TradeForesightCeiling, TradeOptimalBaseline, TradeRuleSearch, TradingRuleBaseline


def get_arg_parser():
    d = _ffi_tradedp.DEFAULT_SIZES
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--assets", type=int, default=2, choices=(1, 2))
    p.add_argument("--envs", type=int, default=64, help="seeded episodes (seed 1692, the eval registration's)")
    p.add_argument("--steps", type=int, default=256, help="steps per episode: the TimeLimit")
    p.add_argument("--grid", nargs=4, type=int, metavar=("NU", "NX", "NA", "NQ"), default=(d["nu"], d["nx"], d["na"], d["nq"]),
                   help="points per share axis, per log-price axis, per action component, quadrature nodes per asset")
    p.add_argument("--x-max", type=float, default=None, help="the log-price axes end at +-x_max (default: 4 std_p)")
    p.add_argument("--horizon", type=int, default=_ffi_tradedp.DEFAULT_HORIZON, help="stages of the induction")
    p.add_argument("--search", nargs=3, type=int, metavar=("G", "C", "K"), default=(8, 32, 8), help="generations, candidates, elites of the tuned rule")
    p.add_argument("--json", help="write the figures to this file")
    p.add_argument("--device", type=int, default=0)
    return p


def main(argv=None):
    parser = get_arg_parser()
    args = parser.parse_args(argv)
    if args.envs < 1 or args.horizon < 1 or args.steps < 1:
        parser.error("--envs, --steps and --horizon need a value >= 1")
    make = lambda seed: _ffi.Engine(_ffi.ENV_TRADE, args.envs, device_id=args.device, seed=seed, n_assets=args.assets, max_episode_steps=args.steps)
    eng, tuned_on = make(1692), make(TRADE_TUNE_SEED)
    eng.reset(); tuned_on.reset()
    nu, nx, na, nq = args.grid
    grid = _ffi_tradedp.trade_dp_grid(nu=nu, nx=nx, na=na, nq=nq, x_max=args.x_max, std_p=eng.cfg.trade_std_p)
    _, rule, floor = TradingRuleBaseline(eng).best_total()
    G, C, K = args.search
    search = TradeRuleSearch(tuned_on, G, C, K)
    tuned = search.play_on(eng)
    best = TradeOptimalBaseline(eng, grid, args.horizon)
    optimal = best.total()
    sem = float(best.stats["total"].std(ddof=1) / np.sqrt(args.envs)) if args.envs > 1 else 0.0
    foresight = TradeForesightCeiling(eng, (0,)).ceiling()
    record = {"n_assets": args.assets, "n_envs": args.envs, "steps": args.steps, "grid": [nu, nx, na, nq], "x_max": grid["x_max"],
              "horizon": args.horizon, "rule": floor, "rule_gain_bias": list(rule), "tuned": tuned, "tuned_rule": list(search.best()[0]),
              "optimal": optimal, "optimal_sem": sem, "foresight": foresight}
    print("TradeAR1, %d asset(s), %d env(s) x %d steps: best default rule %.6f  tuned rule %.6f  attainable optimum %.6f (+- %.6f; grid "
          "%dx%d, %d actions, %d nodes, %d stages)  foresight ceiling %.6f"
          % (args.assets, args.envs, args.steps, floor, tuned, optimal, sem, nu, nx, na, nq, args.horizon, foresight))
    eng.close(); tuned_on.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f)
    return record


if __name__ == "__main__":
    main()
