"""`python -m goldsrl.scripts.train_paac_solow` -- the reference's scripts/train_paac_solow.py CLI
(same flags and defaults, :96-129) driving the device learner."""
import copy
import logging
import sys

from goldsrl.agents.paac import environment_creator
from goldsrl.agents.paac.emulator_runner import SolowRunner
from goldsrl.agents.paac.paac import PAACLearner
from goldsrl.agents.paac.policy_v_network import FlatPolicyVNetwork
from goldsrl.agents.state_processors import SolowStateProcessor
from goldsrl.scripts.train_paac_conv import get_arg_parser as _conv_parser

logging.basicConfig(stream=sys.stdout, level=logging.INFO)


def get_network_and_environment_creator(args, random_seed=3):
    env_creator = environment_creator.SolowEnvironmentCreator(1, 1)       # train_paac_solow.py:60
    args.num_actions = env_creator.num_actions
    args.random_seed = random_seed
    network_conf = {
        'num_actions': args.num_actions, 'entropy_regularisation_strength': args.entropy_regularisation_strength,
        'device': args.device, 'scale': args.scale, 'clip_norm': args.clip_norm, 'clip_norm_type': args.clip_norm_type,
        'static_size': args.static_size, 'temporal_size': args.temporal_size, 'static_hidden_size': args.static_hidden_size,
        'rnn_hidden_size': args.temporal_hidden_size,
    }

    def network_creator(name='local_learning'):
        conf = copy.copy(network_conf)
        conf['name'] = name
        return FlatPolicyVNetwork(conf)

    return network_creator, env_creator


def get_arg_parser():
    p = _conv_parser(baseline_help="play the constant-savings baseline on the eval envs before the first update (one kernel launch) and write "
                                   "eval/baseline_total_reward and eval/mean_total_reward_minus_baseline at every evaluation (needs --eval-envs)",
                     rule_baseline=False, eval_envs=False)
    p.set_defaults(scale=100.)              # train_paac_solow.py:122 (the conv script uses 1000)
    p.add_argument('--eval-envs', default=0, type=int, dest="eval_envs",
                   help="envs of Solow-1-1-finite-eval-v0 evaluated on the device between updates (paac.py:63-77), one launch per "
                        "evaluation; 0: no evaluation")
    p.add_argument('--optimal', action='store_true',
                   help="solve the optimal savings policy by backward induction and play it on the eval envs before the first update; write "
                        "eval/optimal_total_reward and, with --baseline, eval/mean_total_reward_share_of_gap at every evaluation (needs --eval-envs)")
    p.add_argument('--eval-updates', default=0, type=int, dest="eval_updates",
                   help="evaluate after every K-th update; 0: when --eval-every seconds have passed")
    p.add_argument('--true-history', action='store_true', dest="true_history",
                   help="train and evaluate the GRU over the true last --rnn_length states of each env's episode (what the reference's "
                        "monitor feeds) instead of the worker's copies of the current state (quirk Q11)")
    p.add_argument('--max_episode_steps', default=None, type=int, dest="max_episode_steps",
                   help="TimeLimit of the training and eval envs (the registered ids have 1024)")
    return p


def parse_args(argv=None):
    parser = get_arg_parser()
    args = parser.parse_args(argv)
    if args.baseline and args.eval_envs <= 0:
        parser.error("--baseline plays the eval envs of the device monitor: it needs --eval-envs N > 0")
    if args.optimal and args.eval_envs <= 0:
        parser.error("--optimal plays the eval envs of the device monitor: it needs --eval-envs N > 0")
    return args


def main(args):
    network_creator, env_creator = get_network_and_environment_creator(args)
    learner = PAACLearner(network_creator, env_creator, args, SolowRunner, SolowStateProcessor())
    logging.info('Starting training')
    try:
        learner.train()
    finally:
        learner.cleanup()      # the device monitor's eval engine and net, when --eval-envs built them
    logging.info('Finished training')


if __name__ == '__main__':
    main(parse_args())
