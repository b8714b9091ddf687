"""`python -m goldsrl.scripts.trade_foresight` -- floor, ceiling and the worth of foresight on the TradeAR1 env: the best scripted rule
(goldsrl/baselines.py:TradingRuleBaseline, one kernel launch) and, per horizon, the trader who knows that many rows of its price path
beyond the one it trades at -- 0: every row of its episode, the exact ceiling of eval/total_reward (TradeForesightCeiling, one call)
-- on the first episodes of a fresh engine of --envs envs with --assets assets.  The reference has no counterpart."""
import argparse
import json

from goldsrl import _ffi
from goldsrl.baselines import DEFAULT_TRADE_HORIZONS, TradeForesightCeiling, TradingRuleBaseline


def get_arg_parser():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--envs", type=int, default=64, help="episodes (one per env)")
    p.add_argument("--assets", type=int, default=2, help="assets per env, 1..64")
    p.add_argument("--steps", type=int, default=1024, help="steps per episode")
    p.add_argument("--horizons", nargs="+", type=int, default=list(DEFAULT_TRADE_HORIZONS), help="rows known ahead; 0: the whole episode")
    p.add_argument("--seed", type=int, default=1692, help="the engine's seed (1692: the eval registration's)")
    p.add_argument("--json", help="write the figures to this file")
    p.add_argument("--device", type=int, default=0)
    return p


def main(argv=None):
    parser = get_arg_parser()
    args = parser.parse_args(argv)
    if args.envs < 1 or args.steps < 1 or not 1 <= args.assets <= 64:
        parser.error("--envs and --steps need a value >= 1 and --assets one in 1..64")
    eng = _ffi.Engine(_ffi.ENV_TRADE, args.envs, device_id=args.device, seed=args.seed, n_assets=args.assets, max_episode_steps=args.steps)
    eng.reset()
    i, (gain, bias), floor = TradingRuleBaseline(eng).best_total()
    c = TradeForesightCeiling(eng, args.horizons)
    rows = c.table()
    eng.close()
    print("%d env(s) x %d asset(s) x %d steps: floor %.6f (rule %d: gain %g, bias %g)" % (args.envs, args.assets, args.steps, floor, i, gain, bias))
    print("%-14s %12s %10s %10s" % ("rows known", "total", "length", "trades"))
    for h, total, length, trades in rows:
        print("%-14s %12.6f %10.1f %10.1f" % ("whole episode" if h == 0 else h, total, length, trades))
    record = {"n_envs": args.envs, "n_assets": args.assets, "steps": args.steps, "seed": args.seed, "floor_rule": i, "floor": floor,
              "horizons": [{"horizon": h, "total": t, "length": n, "trades": k} for h, t, n, k in rows]}
    if 0 in args.horizons:
        record["ceiling"] = c.ceiling()
        record["gap"] = record["ceiling"] - floor
        print("ceiling %.6f  gap %.6f" % (record["ceiling"], record["gap"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f)
    return record


if __name__ == "__main__":
    main()
