"""`python -m goldsrl.scripts.train_ticker` -- the Ticker gated trader (TickerGatedTraderWorker, fed_gym/agents/a3c/worker.py:445-494)
trained on the device: E envs x T steps per update, each env one A3C worker (include/goldsrl_gatednet.h).  The price table comes
from a CSV (columns Open, Close, Volume) or a --table .npz (Open / Close / Volume or tbl_open / tbl_close / tbl_volume arrays)
through the sampler of goldsrl.envs.data; scalars go to a TF-events file, the checkpoint to <out>/checkpoint.npz.  With --eval-envs M
the GatedPolicyMonitor (goldsrl/agents/a3c/policy_monitor.py) plays, every --eval-every updates and after the last one, M greedy
episodes in one kernel launch on --eval-csv / --eval-table (a held-out price table; default: the training table): per asset the
most probable choice with mu of that choice.  Totals go to <out>/Ticker.json and the eval/* scalars.  With --baseline the scripted
rules of goldsrl/baselines.py (hold cash, buy and hold, a constant mix, follow the trend) play the eval envs' price windows once
before the first update (one launch; the eval engine is reseeded at every reset, so every evaluation plays these windows): the best
rule is logged, eval/baseline_total_reward and eval/mean_total_reward_minus_baseline are written at every evaluation.  With --ceiling the
foresight traders of goldsrl/baselines.py:TickerForesightCeiling play the same windows once (one launch): the mean total of every
horizon is logged, eval/ceiling_total_reward -- the trader who knows every row of its episode -- is written at every evaluation, and
with --baseline also eval/mean_total_reward_share_of_gap = (mean - baseline) / (ceiling - baseline).  With --search-baseline G[:C[:K]]
the six numbers of the rule family are tuned by a cross-entropy search (goldsrl/baselines.py:TickerRuleSearch, every generation in one
call) -- on the TRAINING table when --eval-csv / --eval-table names a held-out one, and the found rule is then played on the eval
envs: six numbers fitted in sample, played out of sample.  The rule and both totals are logged before the first update;
eval/search_baseline_total_reward, eval/mean_total_reward_minus_search_baseline and, when tuned on another table,
eval/search_baseline_in_sample_total_reward are written at every evaluation; the scalars of --baseline and --ceiling are left alone.
Training is untouched."""
import argparse
import logging
import os
import sys
import time

import numpy as np

from goldsrl import _ffi, _ffi_gated
from goldsrl.agents.a3c.policy_monitor import GatedPolicyMonitor
from goldsrl.envs.data.sampler import OpenCloseSampler
from goldsrl.scripts.swarm_rules import search_arg
from goldsrl.utils_tfevents import EventFileWriter

logging.basicConfig(stream=sys.stdout, level=logging.INFO)


def get_arg_parser():
    p = argparse.ArgumentParser(description=__doc__)
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--csv", help="price table CSV (Open, Close, Volume)")
    src.add_argument("--table", help=".npz with the three columns")
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--steps", type=int, default=20, help="env steps per update (T)")
    p.add_argument("--updates", type=int, default=100)
    p.add_argument("--rnn-length", type=int, default=5, help="the worker's max_seq_length (R), 1..20")
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--scale", type=float, default=1.0)
    p.add_argument("--seed", type=int, default=3)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--out", default="logs/ticker")
    p.add_argument("--resume", help="checkpoint .npz to continue from")
    p.add_argument("--checkpoint-every", type=int, default=50)
    p.add_argument("--eval-envs", "--eval_envs", dest="eval_envs", type=int, default=0,
                   help="greedy eval episodes per evaluation (0: no evaluation)")
    p.add_argument("--eval-every", "--eval_every", dest="eval_every", type=int, default=10, help="evaluate every N updates")
    p.add_argument("--baseline", action="store_true",
                   help="play the scripted rules on the eval envs before the first update (one kernel launch) and write "
                        "eval/baseline_total_reward and eval/mean_total_reward_minus_baseline at every evaluation (needs --eval-envs)")
    p.add_argument("--ceiling", action="store_true",
                   help="play the foresight traders on the eval envs before the first update (one kernel launch) and write "
                        "eval/ceiling_total_reward and, with --baseline, eval/mean_total_reward_share_of_gap at every evaluation "
                        "(needs --eval-envs)")
    p.add_argument("--search-baseline", "--search_baseline", dest="search_baseline", type=search_arg, default=None, metavar="G[:C[:K]]",
                   help="tune the rule's six numbers before the first update: G generations of C candidates (default 32) refitted over K "
                        "elites (default 8), one call, on the training table when a held-out eval table is given; writes "
                        "eval/search_baseline_total_reward and eval/mean_total_reward_minus_search_baseline at every evaluation "
                        "(needs --eval-envs)")
    ev = p.add_mutually_exclusive_group()
    ev.add_argument("--eval-csv", "--eval_csv", dest="eval_csv", help="held-out price table CSV for the evaluation")
    ev.add_argument("--eval-table", "--eval_table", dest="eval_table", help="held-out price table .npz for the evaluation")
    return p


def load_table(args, csv=None, table=None):
    csv, table = (args.csv, args.table) if csv is None and table is None else (csv, table)
    if csv:
        return OpenCloseSampler(path=csv)
    with np.load(table) as z:
        keys = ("Open", "Close", "Volume") if "Open" in z.files else ("tbl_open", "tbl_close", "tbl_volume")
        return OpenCloseSampler(table={"Open": z[keys[0]], "Close": z[keys[1]], "Volume": z[keys[2]]})


def parse_args(argv=None):
    parser = get_arg_parser()
    args = parser.parse_args(argv)
    if args.baseline and args.eval_envs <= 0:
        parser.error("--baseline plays the eval envs of the device monitor: it needs --eval-envs M > 0")
    if args.ceiling and args.eval_envs <= 0:
        parser.error("--ceiling plays the eval envs of the device monitor: it needs --eval-envs M > 0")
    if args.search_baseline and args.eval_envs <= 0:
        parser.error("--search-baseline plays the eval envs of the device monitor: it needs --eval-envs M > 0")
    return args


def main(argv=None):
    args = parse_args(argv)
    sampler = load_table(args)
    eng = _ffi.Engine(_ffi.ENV_TICKER, args.envs, device_id=args.device, seed=args.seed)
    eng.ticker_set_table(sampler.data_matrix)
    eng.reset()
    eng.episodes_enable()
    net = _ffi_gated.GatedNet(eng, rnn_length=args.rnn_length, scale=args.scale, max_samples=max(1, args.envs))
    if args.resume:
        net.load_checkpoint(args.resume)
    else:
        net.set_params(_ffi_gated.default_init_gated(args.seed))
    os.makedirs(args.out, exist_ok=True)
    writer = EventFileWriter(args.out)
    ckpt = os.path.join(args.out, "checkpoint.npz")
    log_file = os.path.join(args.out, "Ticker.json")
    monitor = None
    if args.eval_envs > 0:
        if args.eval_every < 1:
            raise SystemExit("--eval-every must be at least 1")
        held_out = load_table(args, args.eval_csv, args.eval_table) if args.eval_csv or args.eval_table else sampler
        monitor = GatedPolicyMonitor(held_out, summary_writer=writer, n_envs=args.eval_envs, max_seq_length=args.rnn_length,
                                     scale=args.scale, device_id=args.device)
        if args.baseline:
            i, rule, total = monitor.ticker_baseline()
            logging.info("Ticker rule baseline on the eval envs: rule %d (up %.6g %.6g, down %.6g %.6g, band %.6g, lookback %d), "
                         "mean total_reward %.6g", i, rule[0], rule[1], rule[2], rule[3], rule[4], int(rule[5]), total)
        if args.ceiling:
            monitor.ticker_ceiling()
            logging.info("Ticker foresight on the eval envs, mean total_reward by rows known ahead: %s",
                         ", ".join("%s %.6g" % ("whole episode" if h == 0 else str(h), tot) for h, tot, _, _ in monitor.ceiling_table))
        if args.search_baseline:
            G, C, K = args.search_baseline
            rule, total = monitor.ticker_search_baseline(G, C, K, tune_table=sampler if held_out is not sampler else None)
            logging.info("Ticker tuned rule (%d generations of %d candidates, %d elites, tuned on the %s table): up %.6g %.6g, down %.6g "
                         "%.6g, band %.6g, lookback %d; mean total_reward on the eval envs %.6g, where it was tuned %.6g", G, C, K,
                         "training" if held_out is not sampler else "eval", rule[0], rule[1], rule[2], rule[3], rule[4], int(rule[5]),
                         total, monitor.search_baseline_in_sample_total_reward)
    for u in range(args.updates):
        t0 = time.time()
        net.rollout(args.steps)
        stats = net.train_rollout(args.lr)
        dt = time.time() - t0
        step = net.get_optimizer_state()["global_step"]
        for k, v in stats.items():
            writer.add_scalar("train/" + k, v, step)
        eps = eng.episodes_read()
        if len(eps):
            writer.add_scalar("episode/total_reward", float(np.mean(eps["total_reward"])), step)
            writer.add_scalar("episode/length", float(np.mean(eps["length"])), step)
        writer.add_scalar("perf/env_steps_per_s", args.envs * args.steps / dt, step)
        if monitor is not None and ((u + 1) % args.eval_every == 0 or u + 1 == args.updates):
            total_reward, episode_length = monitor.eval_once(net.get_params())[:2]
            monitor.write_scalars(step)
            if args.baseline:
                monitor.write_baseline_scalars(step)
            if args.ceiling:
                monitor.write_ceiling_scalars(step)
            if args.search_baseline:
                monitor.write_search_baseline_scalars(step)
            monitor.write_log(log_file)
            logging.info("Eval results at step %d: total_reward %.6g, episode_length %d, mean over %d envs %.6g", step, total_reward,
                         episode_length, monitor.n_envs, monitor.log["mean_total_reward"][-1])
        writer.flush()
        logging.info("update %d  global step %d  policy loss %.4g  value loss %.4g  entropy %.4g  %.0f env-steps/s", u + 1, step,
                     stats["policy_loss"], stats["value_loss"], stats["entropy_mean"], args.envs * args.steps / dt)
        if (u + 1) % args.checkpoint_every == 0 or u + 1 == args.updates:
            net.save_checkpoint(ckpt)
    writer.close()
    if monitor is not None:
        monitor.close()
    net.close()
    eng.close()


if __name__ == "__main__":
    main()
