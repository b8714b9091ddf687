"""`python -m goldsrl.scripts.trade_search` -- the scale of TradeAR1's eval/total_reward for a given --n-assets, four points on N
seeded envs: the best default (gain, bias) rule (goldsrl/baselines.py:TradingRuleBaseline), the four-number rule (gain_buy,
gain_sell, bias, ref) a cross-entropy search tunes from it (TradeRuleSearch, every generation of a start in one device call) where
it was tuned, that rule on the same number of envs with another seed -- four numbers fitted in sample, played out of sample -- and
the foresight ceiling (TradeForesightCeiling).  --starts: `default` (the best default rule, lifted to (g, g, b, 1)) or rules
written gain_buy,gain_sell,bias,ref.  The reference has no counterpart."""
import argparse
import json

import numpy as np

from goldsrl import _ffi
from goldsrl.baselines import TradeForesightCeiling, TradeRuleSearch, TradingRuleBaseline
from goldsrl.scripts.swarm_rules import search_arg


def starts_arg(words):
    """--starts as None (the best default rule), or an (n, 4) float32 array."""
    if words == ["default"]:
        return None
    try:
        rows = np.array([[float(v) for v in w.split(",")] for w in words], np.float32)
    except ValueError:
        rows = np.zeros((0, 0), np.float32)
    if rows.ndim != 2 or rows.shape[1] != 4 or not np.isfinite(rows).all():
        raise ValueError("--starts takes `default` or rules written gain_buy,gain_sell,bias,ref")
    return rows


def get_arg_parser():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--n-assets", "--n_assets", dest="n_assets", type=int, default=2, help="assets of the env, 1..64")
    p.add_argument("--envs", type=int, default=64, help="seeded envs, in sample and out of sample each")
    p.add_argument("--steps", type=int, default=256, help="steps per episode")
    p.add_argument("--search", type=search_arg, default=(8, 32, 8), metavar="G[:C[:K]]",
                   help="G generations of C candidates (default 32) refitted over K elites (default 8)")
    p.add_argument("--starts", nargs="+", default=["default"], help="default, or rules written gain_buy,gain_sell,bias,ref")
    p.add_argument("--seed", type=int, default=0, help="of the search's normals")
    p.add_argument("--env-seed", "--env_seed", dest="env_seed", type=int, default=1692, help="of the envs the rule is tuned on")
    p.add_argument("--other-seed", "--other_seed", dest="other_seed", type=int, default=1693, help="of the envs it is then played on")
    p.add_argument("--json", help="write the figures to this file")
    p.add_argument("--device", type=int, default=0)
    return p


def main(argv=None):
    parser = get_arg_parser()
    args = parser.parse_args(argv)
    if args.envs < 1 or args.steps < 1 or not 1 <= args.n_assets <= 64 or args.env_seed == args.other_seed:
        parser.error("--envs and --steps need a value >= 1, --n-assets one in 1..64, and the two env seeds must differ")
    try:
        starts = starts_arg(args.starts)
    except ValueError as e:
        parser.error(str(e))
    G, C, K = args.search

    def engine(seed):
        eng = _ffi.Engine(_ffi.ENV_TRADE, args.envs, device_id=args.device, seed=seed, n_assets=args.n_assets, max_episode_steps=args.steps)
        eng.reset()
        return eng

    eng, other = engine(args.env_seed), engine(args.other_seed)
    i, (gain, bias), floor = TradingRuleBaseline(eng).best_total()
    lifted = (gain, gain, bias, 1.0)
    se = TradeRuleSearch(eng, G, C, K, starts=starts, seed=args.seed)
    se.run()
    rule, fit = se.best()
    record = {"n_assets": args.n_assets, "n_envs": args.envs, "steps": args.steps, "search": [G, C, K], "default_rule": i,
              "default_gain_bias": [gain, bias], "default_total": floor, "default_total_other_seeds": se.play_on(other, lifted),
              "starts": [{"start": s, "rule": r, "in_sample": f} for s, r, f in se.results],
              "tuned_rule": rule, "tuned_in_sample": fit, "tuned_other_seeds": se.play_on(other),
              "ceiling": TradeForesightCeiling(eng).ceiling(), "ceiling_other_seeds": TradeForesightCeiling(other).ceiling()}
    print("TradeAR1, %d assets, %d envs x %d steps; search: %d generations of %d candidates, %d elites per start"
          % (args.n_assets, args.envs, args.steps, G, C, K))
    print("%-28s %12s %12s" % ("mean total_reward", "in sample", "other seeds"))
    print("%-28s %12.6f %12.6f   rule %d (gain %g, bias %g)" % ("best default rule", floor, record["default_total_other_seeds"], i, gain, bias))
    print("%-28s %12.6f %12.6f   (gain_buy %.6g, gain_sell %.6g, bias %.6g, ref %.6g)"
          % (("tuned rule", fit, record["tuned_other_seeds"]) + tuple(rule)))
    print("%-28s %12.6f %12.6f" % ("foresight ceiling", record["ceiling"], record["ceiling_other_seeds"]))
    eng.close()
    other.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f)
    return record


if __name__ == "__main__":
    main()
