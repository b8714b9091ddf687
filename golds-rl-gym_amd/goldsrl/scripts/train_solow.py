"""`python -m goldsrl.scripts.train_solow` -- scripts/train_solow.py of the reference on the device: the SolowWorker
(fed_gym/agents/a3c/worker.py:394-415) on `Solow-1-1-finite-v0` (1 024-step episodes), E envs x t_max steps per update, each env one
A3C worker (include/goldsrl_gaussnet.h).  The reference's settings: t_max 64, max_seq_length 5, value scale 100, always_bootstrap
on, learning rate 1e-4.  Scalars go to a TF-events file, the checkpoint to <model_dir>/checkpoint.npz.  Every --eval-every updates
the greedy evaluation of a3c/policy_monitor.py:42-96 plays one episode of the seeded `Solow-1-1-finite-eval-v0` with the action
sigmoid(mu) and appends to Solow-1-1.json ({total_reward: [...], episode_length: [...]}, policy_monitor.py:110-118).  With
--eval-envs N the evaluation runs on the device instead (goldsrl/agents/a3c/policy_monitor.py): N seeded eval episodes in one
kernel launch, env 0 the same episode as before; the JSON gains mean_total_reward, std_total_reward and n_envs."""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np

from goldsrl import _ffi, _ffi_gauss
from goldsrl.agents.a3c.estimators import GaussianPolicyEstimator
from goldsrl.agents.a3c.policy_monitor import PolicyMonitor
from goldsrl.agents.state_processors import SolowStateProcessor
from goldsrl.envs import fed_env
from goldsrl.utils_tfevents import EventFileWriter

logging.basicConfig(stream=sys.stdout, level=logging.INFO)

P_ORDER, Q_ORDER = 1, 1
MAX_SEQ_LENGTH = 5          # scripts/train_solow.py:128
SCALE = 100.0               # SolowWorker (worker.py:399), ValueEstimator(scale=100.) (train_solow.py:72)


def get_arg_parser():
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--model_dir", "--out", dest="model_dir", default="/tmp/a3c", help="directory of the events file and the checkpoint")
    p.add_argument("--t_max", type=int, default=64, help="number of steps before performing an update")
    p.add_argument("--envs", "--parallelism", dest="envs", type=int, default=4096, help="number of envs, each one A3C worker")
    p.add_argument("--updates", type=int, default=100)
    p.add_argument("--eval-every", "--eval_every", dest="eval_every", type=int, default=5,
                   help="evaluate the greedy policy every N updates (0: never)")
    p.add_argument("--eval-envs", "--eval_envs", dest="eval_envs", type=int, default=0,
                   help="evaluate N seeded eval episodes on the device, one kernel launch per evaluation (0: one episode driven from the host)")
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


class GreedyMonitor(object):
    """PolicyMonitor.eval_once (a3c/policy_monitor.py:42-96): one episode of the eval env, action = sigmoid(mu), the window is the
    last max_sequence_length processed states; driven from the host through predict on the eval env's own 1-env handle."""

    def __init__(self, device_id=0, log_file="Solow-1-1.json"):
        fed_env.register_solow_env(P_ORDER, Q_ORDER)
        cls, max_steps, kwargs = fed_env.registry["Solow-%d-%d-finite-eval-v0" % (P_ORDER, Q_ORDER)]
        self.env = cls(max_episode_steps=max_steps, device_id=device_id, **kwargs)
        self.net = _ffi_gauss.GaussNet(self.env._eng, rnn_length=MAX_SEQ_LENGTH, scale=SCALE, max_samples=1)
        self.policy_net = GaussianPolicyEstimator(1, static_size=2, temporal_size=2, net=self.net)
        self.state_processor = SolowStateProcessor()
        self.log_file, self.total_rewards, self.episode_lengths = log_file, [], []

    def eval_once(self, params, max_sequence_length=MAX_SEQ_LENGTH):
        self.net.set_params(params)                                       # copy_params_op: global -> policy_eval
        done = False
        processed_state = np.asarray(self.state_processor.process_state(self.env.reset()), np.float64).reshape(-1)
        history = processed_state[None]
        total_reward, episode_length = 0.0, 0
        while not done:
            mu = self.policy_net.predict(processed_state, history)["mu"].flatten()[0]
            action = 1. / (1 + np.exp(-float(mu)))
            next_state, reward, done, _ = self.env.step(action)
            processed_state = np.asarray(self.state_processor.process_state(next_state), np.float64).reshape(-1)
            history = np.vstack([history, processed_state[None]])[-max_sequence_length:, :]
            total_reward += reward
            episode_length += 1
        self.total_rewards.append(total_reward)
        self.episode_lengths.append(episode_length)
        with open(self.log_file, "w") as f:
            json.dump({"total_reward": self.total_rewards, "episode_length": self.episode_lengths}, f)
        return total_reward, episode_length

    def close(self):
        self.net.close()


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
    net = _ffi_gauss.GaussNet(eng, rnn_length=MAX_SEQ_LENGTH, scale=SCALE, always_bootstrap=1, max_samples=max(1, args.envs))
    if args.resume:
        net.load_checkpoint(args.resume)
    else:
        net.set_params(_ffi_gauss.default_init_gauss(args.seed, **_ffi_gauss.SOLOW_SIZES))
    os.makedirs(args.model_dir, exist_ok=True)
    writer = EventFileWriter(args.model_dir)
    ckpt = os.path.join(args.model_dir, "checkpoint.npz")
    log_file = os.path.join(args.model_dir, "Solow-%d-%d.json" % (P_ORDER, Q_ORDER))
    monitor = None
    if args.eval_every > 0 and args.eval_envs > 0:
        monitor = PolicyMonitor("Solow-%d-%d-finite-eval-v0" % (P_ORDER, Q_ORDER), summary_writer=writer, n_envs=args.eval_envs,
                                max_seq_length=MAX_SEQ_LENGTH, scale=SCALE, device_id=args.device)
    elif args.eval_every > 0:
        monitor = GreedyMonitor(args.device, log_file)
    if args.baseline:
        logging.info("Constant-savings baseline on the eval envs: rate %.6g, mean total_reward %.6g", *monitor.baseline())
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
            if args.eval_envs > 0:
                monitor.write_scalars(step)
                if args.baseline or args.optimal:
                    monitor.write_baseline_scalars(step)
                monitor.write_log(log_file)
            else:
                writer.add_scalar("eval/total_reward", total_reward, step)
                writer.add_scalar("eval/episode_length", episode_length, step)
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
