"""`python -m goldsrl.scripts.constant_solow` -- the reference's scripts/constant_solow.py on the device: for (p, q) in (1,1), (2,2),
(3,3) the eval episode of `Solow-p-q-finite-eval-v0` once per constant savings rate, all of them in one kernel launch, and the line
`p s_max max_mean (max, min, std)` of the best rate.  With --envs N the sweep plays N seeded eval episodes: env 0 is the printed
one (the reference's single episode), and the best rate by the mean over all N of the episode's total reward is printed too --
the yardstick for eval/mean_total_reward of train_solow, train_solow_grid and train_paac_solow."""
import argparse
import json

import numpy as np

from goldsrl.baselines import ConstantSavingsBaseline

ORDERS = ((1, 1), (2, 2), (3, 3))       # constant_solow.py:13


def get_arg_parser():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--envs", type=int, default=1, help="seeded eval episodes per order (env 0 is the printed one)")
    p.add_argument("--rates", nargs=3, metavar=("LO", "HI", "N"), default=("0.05", "0.95", "20"), help="np.linspace(lo, hi, n)")
    p.add_argument("--json", help="write every order's statistics to this file")
    p.add_argument("--device", type=int, default=0)
    return p


def main(argv=None):
    parser = get_arg_parser()
    args = parser.parse_args(argv)
    lo, hi, n = float(args.rates[0]), float(args.rates[1]), int(args.rates[2])
    if n < 1 or args.envs < 1:
        parser.error("--rates needs n >= 1 and --envs needs N >= 1")
    rates = np.linspace(lo, hi, n)
    record = {}
    for p, q in ORDERS:
        b = ConstantSavingsBaseline("Solow-%d-%d-finite-eval-v0" % (p, q), n_envs=args.envs, rates=rates, device_id=args.device)
        st = b.run()
        s_max, max_mean, stats = b.best(0)
        print(p, s_max, max_mean, stats)
        rate, total = b.best_total()
        print("   best mean total reward over %d env(s): %.6f at rate %s" % (args.envs, total, rate))
        record["Solow-%d-%d-finite-eval-v0" % (p, q)] = {
            "rates": rates.tolist(), "s_max": float(s_max), "max_mean": float(max_mean),
            "stats": None if stats is None else [float(v) for v in stats], "best_total_rate": float(rate), "best_total": total,
            "n_envs": args.envs, "mean": st["mean"][:, 0].tolist(), "mean_total": st["total"].mean(axis=1).tolist()}
        b.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f)
    return record


if __name__ == "__main__":
    main()
