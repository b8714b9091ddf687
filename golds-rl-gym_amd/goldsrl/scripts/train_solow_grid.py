"""`python -m goldsrl.scripts.train_solow_grid` -- the GridSolowWorker (fed_gym/agents/a3c/worker.py:343-391) on
`Solow-1-1-finite-v0` (1 024-step episodes) on the device: a softmax policy over a grid of --n-grid savings rates in [0.01, 0.99],
E envs x t_max steps per update, each env one A3C worker (include/goldsrl_discretenet.h).  The reference has no script for this
worker; the settings are scripts/train_solow.py's (t_max 64, max_seq_length 5, always_bootstrap on, learning rate 1e-4) with the
worker's own defaults (n_grid 51, value scale 1).  Scalars go to a TF-events file, the checkpoint to <model_dir>/checkpoint.npz
(--resume continues from one).  With --eval-envs N, every --eval-every updates the greedy evaluation
(goldsrl/agents/a3c/policy_monitor.py:GridPolicyMonitor) plays N seeded episodes of `Solow-1-1-finite-eval-v0` in one kernel launch
and writes Solow-1-1-grid.json ({total_reward, episode_length} of env 0, mean_total_reward, std_total_reward, n_envs)."""
import argparse
import logging
import os
import sys
import time

import numpy as np

from goldsrl import _ffi, _ffi_discrete
from goldsrl.agents.a3c.policy_monitor import GridPolicyMonitor
from goldsrl.utils_tfevents import EventFileWriter

logging.basicConfig(stream=sys.stdout, level=logging.INFO)

P_ORDER, Q_ORDER = 1, 1
MAX_SEQ_LENGTH = 5          # scripts/train_solow.py:128
SCALE = 1.0                 # GridSolowWorker's default (worker.py:346)


def get_arg_parser():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--model_dir", "--out", dest="model_dir", default="/tmp/a3c_grid", help="directory of the events file and the checkpoint")
    p.add_argument("--t-max", "--t_max", dest="t_max", type=int, default=64, help="number of steps before performing an update")
    p.add_argument("--envs", "--parallelism", dest="envs", type=int, default=4096, help="number of envs, each one A3C worker")
    p.add_argument("--n-grid", "--n_grid", dest="n_grid", type=int, default=51, help="grid points of the savings rate (2..64)")
    p.add_argument("--updates", type=int, default=100)
    p.add_argument("--eval-every", "--eval_every", dest="eval_every", type=int, default=5,
                   help="evaluate the greedy policy every N updates (0: never)")
    p.add_argument("--eval-envs", "--eval_envs", dest="eval_envs", type=int, default=0,
                   help="seeded eval episodes per evaluation, one kernel launch (0: no evaluation)")
    p.add_argument("--baseline", action="store_true",
                   help="play the constant-savings baseline on the eval envs before the first update (one kernel launch) and write "
                        "eval/baseline_total_reward and eval/mean_total_reward_minus_baseline at every evaluation (needs --eval-envs)")
    p.add_argument("--optimal", action="store_true",
                   help="solve the optimal savings policy by backward induction and play it on the eval envs before the first update; write "
                        "eval/optimal_total_reward and, with --baseline, eval/mean_total_reward_share_of_gap at every evaluation (needs --eval-envs)")
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
        parser.error("--baseline plays the eval envs of the device monitor: it needs --eval-envs N > 0 (and --eval-every > 0)")
    if args.optimal and not (args.eval_envs > 0 and args.eval_every > 0):
        parser.error("--optimal plays the eval envs of the device monitor: it needs --eval-envs N > 0 (and --eval-every > 0)")
    return args


def main(argv=None):
    args = parse_args(argv)
    eng = _ffi.Engine(_ffi.ENV_SOLOW, args.envs, device_id=args.device, seed=args.seed, solow_p=P_ORDER, solow_q=Q_ORDER,
                      max_episode_steps=1024)
    eng.reset()
    eng.episodes_enable()
    net = _ffi_discrete.DiscreteNet(eng, rnn_length=MAX_SEQ_LENGTH, scale=SCALE, num_choices=args.n_grid, max_samples=max(1, args.envs))
    if args.resume:
        net.load_checkpoint(args.resume)
    else:
        net.set_params(_ffi_discrete.default_init_discrete(args.seed, args.n_grid))
    os.makedirs(args.model_dir, exist_ok=True)
    writer = EventFileWriter(args.model_dir)
    ckpt = os.path.join(args.model_dir, "checkpoint.npz")
    log_file = os.path.join(args.model_dir, "Solow-%d-%d-grid.json" % (P_ORDER, Q_ORDER))
    monitor = None
    if args.eval_every > 0 and args.eval_envs > 0:
        monitor = GridPolicyMonitor("Solow-%d-%d-finite-eval-v0" % (P_ORDER, Q_ORDER), summary_writer=writer, n_envs=args.eval_envs,
                                    n_grid=args.n_grid, max_seq_length=MAX_SEQ_LENGTH, scale=SCALE, device_id=args.device)
    if args.baseline:
        logging.info("Constant-savings baseline on the eval envs (the agent's grid): rate %.6g, mean total_reward %.6g", *monitor.baseline())
    if args.optimal:
        logging.info("Optimal savings policy on the eval envs: mean total_reward %.6g", monitor.optimal())
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
            total_reward, episode_length = monitor.eval_once(net.get_params())[:2]
            monitor.write_scalars(step)
            if args.baseline or args.optimal:
                monitor.write_baseline_scalars(step)
            monitor.write_log(log_file)
            logging.info("Eval results at step %d: total_reward %.6g, episode_length %d", step, total_reward, episode_length)
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
