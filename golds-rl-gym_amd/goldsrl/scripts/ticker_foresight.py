"""`python -m goldsrl.scripts.ticker_foresight` -- floor, ceiling and the worth of foresight on a price table of the Ticker env: the
best scripted rule (goldsrl/baselines.py:TickerRuleBaseline, one kernel launch) and, per horizon, the trader who knows that many
rows of the table beyond the one it trades at -- 0: every row of its episode, the exact ceiling of eval/total_reward
(TickerForesightCeiling, one launch) -- on the N seeded eval windows of the gated trader's monitor.  The table comes from a CSV
(columns Open, Close, Volume) or a .npz, as in train_ticker.  The reference has no counterpart."""
import argparse
import json

from goldsrl.agents.a3c.policy_monitor import make_ticker_eval_engine
from goldsrl.baselines import DEFAULT_TICKER_HORIZONS, TickerForesightCeiling, TickerRuleBaseline
from goldsrl.scripts.train_ticker import load_table


def get_arg_parser():
    p = argparse.ArgumentParser(description=__doc__)
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--csv", help="price table CSV (Open, Close, Volume)")
    src.add_argument("--table", help=".npz with the three columns")
    p.add_argument("--envs", type=int, default=64, help="seeded eval windows")
    p.add_argument("--steps", type=int, default=1023, help="steps per episode, 1..1023")
    p.add_argument("--horizons", nargs="+", type=int, default=list(DEFAULT_TICKER_HORIZONS), help="rows known ahead; 0: the whole episode")
    p.add_argument("--json", help="write the figures to this file")
    p.add_argument("--device", type=int, default=0)
    return p


def main(argv=None):
    parser = get_arg_parser()
    args = parser.parse_args(argv)
    if args.envs < 1 or not 1 <= args.steps <= 1023:
        parser.error("--envs needs a value >= 1 and --steps one in 1..1023")
    eng = make_ticker_eval_engine(load_table(args), args.envs, args.device, max_episode_steps=args.steps)
    eng.reset()
    i, rule, floor = TickerRuleBaseline(eng).best_total()
    c = TickerForesightCeiling(eng, args.horizons)
    rows = c.table()
    eng.close()
    print("%d window(s) x %d steps: floor %.6f (rule %d: %s)" % (args.envs, args.steps, floor, i, " ".join("%g" % v for v in rule)))
    print("%-14s %12s %10s %10s" % ("rows known", "total", "length", "trades"))
    for h, total, length, trades in rows:
        print("%-14s %12.6f %10.1f %10.1f" % ("whole episode" if h == 0 else h, total, length, trades))
    record = {"n_envs": args.envs, "steps": args.steps, "floor_rule": i, "floor": floor,
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
