"""`python -m goldsrl.scripts.train_trade` -- scripts/train_trade.py of the reference on the device: the TradeWorker
(fed_gym/agents/a3c/worker.py:418-442) on `TradeAR1-v0` (2 assets, 1 024-step episodes), E envs x t_max steps per update, each env
one A3C worker (include/goldsrl_gaussnet.h).  The reference's settings: t_max 64, max_seq_length 20, value scale 1,
always_bootstrap off, learning rate 1e-4.  The reference's TradeWorker cannot run as written; the device form takes the evident
reading (per-action mu and sigma, the raw draw stored and trained on, tanh to the env).  Scalars go to a
TF-events file, the checkpoint to <model_dir>/checkpoint.npz.  With --eval-every N and --eval-envs M the PolicyMonitor of
scripts/train_trade.py:94-124 runs on the device (goldsrl/agents/a3c/policy_monitor.py): every N updates M greedy episodes of
`TradeAR1-v0` in one kernel launch, action tanh(mu); totals go to TradeAR1.json and the eval/* scalars.  With --baseline the
scripted trading rules of goldsrl/baselines.py play the same episodes directly before every evaluation (one more launch): the best
rule is logged, eval/baseline_total_reward and eval/mean_total_reward_minus_baseline are written.  With --ceiling the foresight
traders of goldsrl/baselines.py:TradeForesightCeiling play the same episodes directly before every evaluation too (one more call):
the mean total of every horizon is logged, eval/ceiling_total_reward -- the trader who knows every row of its episode -- is written,
and with --baseline also eval/mean_total_reward_share_of_gap = (mean - baseline) / (ceiling - baseline).  With --search-baseline
G[:C[:K]] the four-number rule of goldsrl/baselines.py:TradeRuleSearch is tuned once, before the first evaluation, on a second
eval-style engine with its own seed (G generations of C candidates, K elites, one device call) and played on the eval envs directly
before every evaluation: the rule and both totals are logged, eval/search_baseline_total_reward,
eval/mean_total_reward_minus_search_baseline and eval/search_baseline_in_sample_total_reward are written; the scalars of --baseline
and --ceiling are left alone.  Training is untouched."""
import argparse
import logging
import os
import sys
import time

import numpy as np

from goldsrl import _ffi, _ffi_gauss
from goldsrl.agents.a3c.policy_monitor import PolicyMonitor
from goldsrl.scripts.swarm_rules import search_arg
from goldsrl.utils_tfevents import EventFileWriter

logging.basicConfig(stream=sys.stdout, level=logging.INFO)

MAX_SEQ_LENGTH = 20         # scripts/train_trade.py:119
SCALE = 1.0


def get_arg_parser():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--model_dir", "--out", dest="model_dir", default="/tmp/a3c", help="directory of the events file and the checkpoint")
    p.add_argument("--t_max", type=int, default=64, help="number of steps before performing an update")
    p.add_argument("--envs", "--parallelism", dest="envs", type=int, default=4096, help="number of envs, each one A3C worker")
    p.add_argument("--updates", type=int, default=100)
    p.add_argument("--eval-every", "--eval_every", dest="eval_every", type=int, default=0,
                   help="evaluate the greedy policy every N updates (0: never)")
    p.add_argument("--eval-envs", "--eval_envs", dest="eval_envs", type=int, default=64, help="eval episodes per evaluation")
    p.add_argument("--baseline", action="store_true",
                   help="play the scripted trading rules on the eval envs directly before every evaluation (one kernel launch) and write "
                        "eval/baseline_total_reward and eval/mean_total_reward_minus_baseline (needs --eval-every and --eval-envs)")
    p.add_argument("--ceiling", action="store_true",
                   help="play the foresight traders on the eval envs directly before every evaluation (one more call) and write "
                        "eval/ceiling_total_reward and, with --baseline, eval/mean_total_reward_share_of_gap (needs --eval-every and "
                        "--eval-envs)")
    p.add_argument("--search-baseline", "--search_baseline", dest="search_baseline", type=search_arg, default=None, metavar="G[:C[:K]]",
                   help="tune the four-number rule once on a second eval-style engine (G generations of C candidates, default 32, K "
                        "elites, default 8), play it on the eval envs directly before every evaluation and write "
                        "eval/search_baseline_total_reward, eval/mean_total_reward_minus_search_baseline and "
                        "eval/search_baseline_in_sample_total_reward (needs --eval-every and --eval-envs)")
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--seed", type=int, default=3)
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--resume", help="checkpoint .npz to continue from")
    p.add_argument("--checkpoint-every", type=int, default=50)
    return p


def parse_args(argv=None):
    parser = get_arg_parser()
    args = parser.parse_args(argv)
    if args.baseline and not (args.eval_envs > 0 and args.eval_every > 0):
        parser.error("--baseline plays the eval envs of the device monitor: it needs --eval-every N > 0 and --eval-envs M > 0")
    if args.ceiling and not (args.eval_envs > 0 and args.eval_every > 0):
        parser.error("--ceiling plays the eval envs of the device monitor: it needs --eval-every N > 0 and --eval-envs M > 0")
    if args.search_baseline and not (args.eval_envs > 0 and args.eval_every > 0):
        parser.error("--search-baseline plays the eval envs of the device monitor: it needs --eval-every N > 0 and --eval-envs M > 0")
    return args


def main(argv=None):
    args = parse_args(argv)
    eng = _ffi.Engine(_ffi.ENV_TRADE, args.envs, device_id=args.device, seed=args.seed, n_assets=2, max_episode_steps=1024)
    eng.reset()
    eng.episodes_enable()
    net = _ffi_gauss.GaussNet(eng, rnn_length=MAX_SEQ_LENGTH, scale=SCALE, always_bootstrap=0, max_samples=max(1, args.envs))
    if args.resume:
        net.load_checkpoint(args.resume)
    else:
        net.set_params(_ffi_gauss.default_init_gauss(args.seed, **_ffi_gauss.TRADE_SIZES))
    os.makedirs(args.model_dir, exist_ok=True)
    writer = EventFileWriter(args.model_dir)
    ckpt = os.path.join(args.model_dir, "checkpoint.npz")
    log_file = os.path.join(args.model_dir, "TradeAR1.json")
    monitor = None
    if args.eval_every > 0 and args.eval_envs > 0:
        monitor = PolicyMonitor("TradeAR1-v0", summary_writer=writer, n_envs=args.eval_envs, max_seq_length=MAX_SEQ_LENGTH, scale=SCALE,
                                device_id=args.device)
    for u in range(args.updates):
        t0 = time.time()
        net.rollout(args.t_max)
        stats = net.train_rollout(args.lr)
        dt = time.time() - t0
        step = net.get_optimizer_state()["global_step"]
        for k, v in stats.items():
            writer.add_scalar("train/" + k, v, step)
        eps = eng.episodes_read()
        if len(eps):
            writer.add_scalar("episode/total_reward", float(np.mean(eps["total_reward"])), step)
            writer.add_scalar("episode/length", float(np.mean(eps["length"])), step)
        writer.add_scalar("perf/env_steps_per_s", args.envs * args.t_max / dt, step)
        if monitor is not None and ((u + 1) % args.eval_every == 0 or u + 1 == args.updates):
            if args.baseline:       # the price generator moves on between evaluations: the rules must see this evaluation's prices
                i, (gain, bias), total = monitor.rule_baseline()
                logging.info("Trading-rule baseline on the eval envs: rule %d (gain %.6g, bias %.6g), mean total_reward %.6g", i, gain, bias, total)
            if args.ceiling:        # likewise: this evaluation's prices
                monitor.trade_ceiling()
                logging.info("TradeAR1 foresight on the eval envs, mean total_reward by rows known ahead: %s",
                             ", ".join("%s %.6g" % ("whole episode" if h == 0 else str(h), tot) for h, tot, _, _ in monitor.ceiling_table))
            if args.search_baseline:    # tuned once on other seeds; played on this evaluation's prices
                G, C, K = args.search_baseline
                rule, total = monitor.search_baseline(G, C, K)
                logging.info("Tuned rule (gain_buy %.6g, gain_sell %.6g, bias %.6g, ref %.6g) on the eval envs: mean total_reward %.6g "
                             "(in sample %.6g)", *(rule + (total, monitor.search_baseline_in_sample_total_reward)))
            total_reward, episode_length = monitor.eval_once(net.get_params())[:2]
            monitor.write_scalars(step)
            if args.search_baseline:
                monitor.write_search_baseline_scalars(step)
            if args.baseline:
                monitor.write_baseline_scalars(step)
            if args.ceiling:
                monitor.write_ceiling_scalars(step)
            monitor.write_log(log_file)
            logging.info("Eval results at step %d: total_reward %.6g, episode_length %d, mean over %d envs %.6g", step, total_reward,
                         episode_length, monitor.n_envs, monitor.log["mean_total_reward"][-1])
        writer.flush()
        logging.info("update %d  global step %d  policy loss %.4g  value loss %.4g  entropy %.4g  %.0f env-steps/s", u + 1, step,
                     stats["policy_loss"], stats["value_loss"], stats["entropy_mean"], args.envs * args.t_max / dt)
        if (u + 1) % args.checkpoint_every == 0 or u + 1 == args.updates:
            net.save_checkpoint(ckpt)
    writer.close()
    if monitor is not None:
        monitor.close()
    net.close()
    eng.close()


if __name__ == "__main__":
    main()
