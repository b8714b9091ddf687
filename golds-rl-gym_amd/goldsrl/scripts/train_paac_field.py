"""`python -m goldsrl.scripts.train_paac_field` -- PAAC on Swarm-v0 with the field policy (ConvPolicyVFieldNetwork,
policy_v_network.py:83-191): the arguments of train_paac_conv, with --height (the grid of the density image and of the mu / sigma
fields, default 20: SwarmStateProcessor's), --filters (5) and --conv_layers (2) describing the net.  The reference carries this
learner only as commented-out feeds (paac.py:292,317,356,369,377); here GridPAACLearner drives it through the same two device
calls per update as the conv policy (include/goldsrl_fieldrollout.h)."""
import copy
import logging

from goldsrl.agents.paac import environment_creator
from goldsrl.agents.paac.emulator_runner import SwarmRunner
from goldsrl.agents.paac.paac import GridPAACLearner
from goldsrl.agents.paac.policy_v_network import ConvPolicyVFieldNetwork
from goldsrl.scripts import train_paac_conv


def get_network_and_environment_creator(args, random_seed=3):
    env_creator = environment_creator.SwarmEnvironmentCreator()
    args.num_actions = env_creator.num_actions
    args.random_seed = random_seed
    network_conf = {
        'num_actions': args.num_actions, 'entropy_regularisation_strength': args.entropy_regularisation_strength,
        'device': args.device, 'height': args.height, 'width': args.height, 'channels': 2, 'filters': args.filters,
        'conv_layers': args.conv_layers, 'scale': args.scale, 'clip_norm': args.clip_norm, 'clip_norm_type': args.clip_norm_type,
    }

    def network_creator(name='local_learning'):
        conf = copy.copy(network_conf)
        conf['name'] = name
        return ConvPolicyVFieldNetwork(conf)

    return network_creator, env_creator


def get_arg_parser():
    p = train_paac_conv.get_arg_parser(eval_envs=False)
    p.description = "PAAC on Swarm-v0 with the field policy (device engine)"
    p.set_defaults(height=20, filters=5)
    p.add_argument('--conv_layers', dest='conv_layers', type=int, default=2)
    p.add_argument('--eval-envs', default=1, type=int, dest="eval_envs",
                   help="seeded episodes of Swarm-eval-v0 per evaluation (--eval-every), all in one kernel launch; env 0 is the registration's "
                        "episode, the one the scalars and swarm-eval.json speak of; above 1 eval/mean_total_reward is written too")
    return p


def main(args):
    train_paac_conv.check_baseline_flags(args)
    if args.height % (2 ** args.conv_layers):
        raise SystemExit("--height must be a multiple of 2^conv_layers")
    network_creator, env_creator = get_network_and_environment_creator(args)
    learner = GridPAACLearner(network_creator, env_creator, args, SwarmRunner, state_processor=None)
    logging.info('Starting training')
    learner.train()
    logging.info('Finished training')


if __name__ == '__main__':
    main(get_arg_parser().parse_args())
