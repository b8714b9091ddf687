"""`python -m goldsrl.scripts.train_trade_grid` -- the grid trader on `TradeAR1-v0` (2 assets, 1 024-step episodes) on the device: a
softmax policy per asset over a grid of --n-grid actions in [-1, 1] (DiscretePolicyEstimator with num_outputs = 2), E envs x t_max
steps per update, each env one A3C worker (include/goldsrl_gridtradenet.h).  The reference has no Trade grid worker: the agent is
TradeWorker's state, window and bootstrap rule with GridSolowWorker's acting and update, and the settings are
scripts/train_trade.py's (t_max 64, max_seq_length 20, value scale 1, always_bootstrap off, learning rate 1e-4).  Its action set is
the one the yardsticks play: the default 17 points are the attainable optimum's own action grid, and -1, 0 and 1 are points of it.
Scalars go to a TF-events file, the checkpoint to <model_dir>/checkpoint.npz (--resume continues from one).  --eval-every,
--eval-envs, --baseline, --ceiling, --search-baseline and --optimal are train_trade's flags with train_trade's scalars; the
evaluation is GridTradeMonitor's (goldsrl/agents/a3c/policy_monitor.py): M greedy episodes in one kernel launch, per asset the grid
point of the largest probability; totals go to TradeAR1-grid.json.  Training is untouched by them.

--teach-updates N (default 0: the script as it always was) first fits the net to the attainable optimum
(include/goldsrl_gridtradeteach.h): TradeOptimalBaseline's default grid is solved once ON THE TRAINING HANDLE -- the table lives
per handle; the monitor's is on the eval handle -- then N times a teach rollout, in which the table labels every step and each env
follows the agent with probability --teach-agent-share and the teacher otherwise, and the cross-entropy update at --teach-lr.
teach/cross_entropy, teach/agreement and teach/value_loss are written per update; the evaluations run as in the A3C phase, one of
them directly after the last teach update.  The A3C updates then start from the taught net."""
import logging
import os
import sys
import time

import numpy as np

from goldsrl import _ffi, _ffi_gridtrade
from goldsrl.agents.a3c.policy_monitor import GridTradeMonitor
from goldsrl.scripts import train_trade
from goldsrl.utils_tfevents import EventFileWriter

logging.basicConfig(stream=sys.stdout, level=logging.INFO)

MAX_SEQ_LENGTH, SCALE = train_trade.MAX_SEQ_LENGTH, train_trade.SCALE


def get_arg_parser():
    p = train_trade.get_arg_parser()
    p.description = __doc__
    p.set_defaults(model_dir="/tmp/a3c_trade_grid")
    p.add_argument("--n-grid", "--n_grid", dest="n_grid", type=int, default=17,
                   help="grid points of each asset's action in [-1, 1] (2..%d; odd: 0, the hold, is a point)" % _ffi_gridtrade.K_MAX)
    p.add_argument("--teach-updates", dest="teach_updates", type=int, default=0,
                   help="supervised updates on the attainable optimum's table before the first A3C update (0: none)")
    p.add_argument("--teach-agent-share", dest="teach_agent_share", type=float, default=0.0,
                   help="share of the teach rollout's steps an env takes with the agent's own action (0: it follows the teacher)")
    p.add_argument("--teach-lr", dest="teach_lr", type=float, default=None, help="learning rate of the teach updates (default: --lr)")
    return p


def parse_args(argv=None):
    parser = get_arg_parser()
    args = parser.parse_args(argv)
    for flag, on in (("--baseline", args.baseline), ("--ceiling", args.ceiling), ("--search-baseline", args.search_baseline),
                     ("--optimal", args.optimal)):
        if on and not (args.eval_envs > 0 and args.eval_every > 0):
            parser.error("%s plays the eval envs of the device monitor: it needs --eval-every N > 0 and --eval-envs M > 0" % flag)
    if args.teach_updates < 0 or not 0.0 <= args.teach_agent_share <= 1.0:
        parser.error("--teach-updates must be >= 0 and --teach-agent-share in [0, 1]")
    return args


def evaluate(args, monitor, net, step, log_file):
    """Every yardstick asked for, then the greedy evaluation of the net's current parameters, their scalars and the log lines."""
    # the price generator moves on between evaluations: every yardstick plays directly before the evaluation, on its prices
    if args.baseline:
        i, (gain, bias), total = monitor.rule_baseline()
        logging.info("Trading-rule baseline on the eval envs: rule %d (gain %.6g, bias %.6g), mean total_reward %.6g", i, gain, bias, total)
    if args.ceiling:
        monitor.trade_ceiling()
        logging.info("TradeAR1 foresight on the eval envs, mean total_reward by rows known ahead: %s",
                     ", ".join("%s %.6g" % ("whole episode" if h == 0 else str(h), tot) for h, tot, _, _ in monitor.ceiling_table))
    if args.search_baseline:
        G, C, K = args.search_baseline
        rule, total = monitor.search_baseline(G, C, K)
        logging.info("Tuned rule (gain_buy %.6g, gain_sell %.6g, bias %.6g, ref %.6g) on the eval envs: mean total_reward %.6g "
                     "(in sample %.6g)", *(rule + (total, monitor.search_baseline_in_sample_total_reward)))
    if args.optimal:
        logging.info("Attainable optimum on the eval envs: mean total_reward %.6g", monitor.trade_optimal())
    total_reward, episode_length = monitor.eval_once(net.get_params())[:2]
    mean = monitor.log["mean_total_reward"][-1]
    monitor.write_scalars(step)
    if args.search_baseline:
        monitor.write_search_baseline_scalars(step)
    if args.baseline:
        monitor.write_baseline_scalars(step)
    if args.ceiling:
        monitor.write_ceiling_scalars(step)
    if args.optimal:
        monitor.write_trade_optimal_scalars(step)
    monitor.write_log(log_file)
    logging.info("Eval results at step %d: total_reward %.6g, episode_length %d, mean over %d envs %.6g", step, total_reward,
                 episode_length, monitor.n_envs, mean)
    floor = monitor.baseline_total_reward if args.baseline else None
    for name, top in (("attainable gap", monitor.attainable_total_reward if args.optimal else None),
                      ("gap to the ceiling", monitor.ceiling_total_reward if args.ceiling else None)):
        if floor is not None and top is not None and top != floor:
            logging.info("Share of the %s at step %d: %.4g", name, step, (mean - floor) / (top - floor))


def main(argv=None):
    args = parse_args(argv)
    eng = _ffi.Engine(_ffi.ENV_TRADE, args.envs, device_id=args.device, seed=args.seed, n_assets=2, max_episode_steps=1024)
    eng.reset()
    eng.episodes_enable()
    net = _ffi_gridtrade.GridTradeNet(eng, rnn_length=MAX_SEQ_LENGTH, scale=SCALE, num_choices=args.n_grid, max_samples=max(1, args.envs))
    if args.resume:
        net.load_checkpoint(args.resume)
    else:
        net.set_params(_ffi_gridtrade.default_init_gridtrade(args.seed, args.n_grid))
    os.makedirs(args.model_dir, exist_ok=True)
    writer = EventFileWriter(args.model_dir)
    ckpt = os.path.join(args.model_dir, "checkpoint.npz")
    log_file = os.path.join(args.model_dir, "TradeAR1-grid.json")
    monitor = None
    if args.eval_every > 0 and args.eval_envs > 0:
        monitor = GridTradeMonitor("TradeAR1-v0", summary_writer=writer, n_envs=args.eval_envs, n_grid=args.n_grid,
                                   max_seq_length=MAX_SEQ_LENGTH, scale=SCALE, device_id=args.device)
    if args.teach_updates > 0:
        from goldsrl.baselines import TradeOptimalBaseline
        TradeOptimalBaseline(eng).solve()           # on the training handle: the teach rollout reads its table
        teach_lr = args.lr if args.teach_lr is None else args.teach_lr
    for u in range(args.teach_updates):
        net.teach_rollout(args.t_max, args.teach_agent_share)
        stats = net.train_teach_rollout(teach_lr)
        step = net.get_optimizer_state()["global_step"]
        for k in ("cross_entropy", "agreement", "value_loss"):
            writer.add_scalar("teach/" + k, stats[k], step)
        if monitor is not None and ((u + 1) % args.eval_every == 0 or u + 1 == args.teach_updates):
            evaluate(args, monitor, net, step, log_file)
        writer.flush()
        logging.info("teach update %d  global step %d  cross-entropy %.4g  agreement %.4g  value loss %.4g", u + 1, step, stats["cross_entropy"],
                     stats["agreement"], stats["value_loss"])
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
            evaluate(args, monitor, net, step, log_file)
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
