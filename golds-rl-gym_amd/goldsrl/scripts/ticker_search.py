"""`python -m goldsrl.scripts.ticker_search` -- tune the six numbers of the Ticker rule family (up0, up1, dn0, dn1, band, lookback)
on a price table: a cross-entropy search from every start rule (goldsrl/baselines.py:TickerRuleSearch, every generation of a start
in one device call) on the N seeded eval windows of the gated trader's monitor, and -- with --eval-table / --eval-csv -- every found
rule played on the same number of windows of a held-out table: six numbers fitted in sample, played out of sample.  The table comes
from a CSV (columns Open, Close, Volume) or a .npz, as in train_ticker.  --starts: `default` (the best default rule on the table),
`all` (every default rule) or rules written up0,up1,dn0,dn1,band,lookback.  The reference has no counterpart."""
import argparse
import json

import numpy as np

from goldsrl.agents.a3c.policy_monitor import make_ticker_eval_engine
from goldsrl.baselines import DEFAULT_TICKER_RULES, TickerRuleBaseline, TickerRuleSearch
from goldsrl.scripts.swarm_rules import search_arg
from goldsrl.scripts.train_ticker import load_table


def starts_arg(words):
    """--starts as None (the best default rule), or an (n, 6) float32 array."""
    if words == ["default"]:
        return None
    if words == ["all"]:
        return DEFAULT_TICKER_RULES
    try:
        rows = np.array([[float(v) for v in w.split(",")] for w in words], np.float32)
    except ValueError:
        rows = np.zeros((0, 0), np.float32)
    if rows.ndim != 2 or rows.shape[1] != 6:
        raise ValueError("--starts takes `default`, `all` or rules written up0,up1,dn0,dn1,band,lookback")
    return rows


def get_arg_parser():
    p = argparse.ArgumentParser(description=__doc__)
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--csv", help="price table CSV (Open, Close, Volume)")
    src.add_argument("--table", help=".npz with the three columns")
    ev = p.add_mutually_exclusive_group()
    ev.add_argument("--eval-csv", "--eval_csv", dest="eval_csv", help="held-out price table CSV the found rules are played on")
    ev.add_argument("--eval-table", "--eval_table", dest="eval_table", help="held-out price table .npz the found rules are played on")
    p.add_argument("--envs", type=int, default=64, help="seeded eval windows")
    p.add_argument("--steps", type=int, default=1023, help="steps per episode, 1..1023")
    p.add_argument("--search", type=search_arg, default=(8, 32, 8), metavar="G[:C[:K]]",
                   help="G generations of C candidates (default 32) refitted over K elites (default 8)")
    p.add_argument("--starts", nargs="+", default=["default"], help="default, all, or rules written up0,up1,dn0,dn1,band,lookback")
    p.add_argument("--seed", type=int, default=0, help="of the search's normals")
    p.add_argument("--json", help="write the figures to this file")
    p.add_argument("--device", type=int, default=0)
    return p


def main(argv=None):
    parser = get_arg_parser()
    args = parser.parse_args(argv)
    if args.envs < 1 or not 1 <= args.steps <= 1023:
        parser.error("--envs needs a value >= 1 and --steps one in 1..1023")
    try:
        starts = starts_arg(args.starts)
    except ValueError as e:
        parser.error(str(e))
    G, C, K = args.search
    eng = make_ticker_eval_engine(load_table(args), args.envs, args.device, max_episode_steps=args.steps)
    eng.reset()
    held = None
    if args.eval_csv or args.eval_table:
        held = make_ticker_eval_engine(load_table(args, args.eval_csv, args.eval_table), args.envs, args.device, max_episode_steps=args.steps)
        held.reset()
    i, rule, floor = TickerRuleBaseline(eng).best_total()
    print("%d window(s) x %d steps: best default rule %d (%s) total %.6f" % (args.envs, args.steps, i, " ".join("%g" % v for v in rule), floor))
    se = TickerRuleSearch(eng, starts=starts, generations=G, candidates=C, elites=K, seed=args.seed)
    se.run()
    rows = []
    print("search: %d generations of %d candidates, %d elites per start" % (G, C, K))
    for start, found, fit in se.results:
        row = {"start": start, "rule": found, "in_sample": fit}
        line = "start %-28s -> %-60s in-sample %.6f" % (" ".join("%g" % v for v in start), " ".join("%.6g" % v for v in found), fit)
        if held is not None:
            row["held_out"] = se.play_on(held, found)
            line += "  held-out %.6f" % row["held_out"]
        print(line)
        rows.append(row)
    best, fit = se.best()
    record = {"n_envs": args.envs, "steps": args.steps, "search": [G, C, K], "default_rule": i, "default_total": floor, "starts": rows,
              "best_rule": best, "best_in_sample": fit}
    if held is not None:
        record["best_held_out"] = se.play_on(held)
        record["default_held_out"] = se.play_on(held, rule)
        print("held-out: best default rule %.6f, tuned rule %.6f" % (record["default_held_out"], record["best_held_out"]))
        held.close()
    eng.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f)
    return record


if __name__ == "__main__":
    main()
