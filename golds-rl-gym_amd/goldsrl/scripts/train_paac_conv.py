"""`python -m goldsrl.scripts.train_paac_conv` -- the reference's scripts/train_paac_conv.py CLI
(same flags and defaults, :95-121) driving the device learner."""
import argparse
import copy
import logging
import sys

from goldsrl.agents.paac import environment_creator
from goldsrl.agents.paac.emulator_runner import SwarmRunner
from goldsrl.agents.paac.paac import GridPAACLearner
from goldsrl.agents.paac.policy_v_network import ConvSingleAgentPolicyNetwork
from goldsrl.agents.state_processors import SwarmStateProcessor
from goldsrl.scripts.swarm_rules import cem_plan_arg, plan_arg, search_arg

logging.basicConfig(stream=sys.stdout, level=logging.INFO)


def bool_arg(text):
    """'true' / 'false' (any case) -> bool, as the reference's flag type does."""
    table = {'true': True, 'false': False}
    if text.lower() not in table:
        raise argparse.ArgumentTypeError("Expected True or False, but got {}".format(text))
    return table[text.lower()]


def get_network_and_environment_creator(args, random_seed=3):
    env_creator = environment_creator.SwarmEnvironmentCreator()
    args.num_actions = env_creator.num_actions
    args.random_seed = random_seed
    network_conf = {
        'num_actions': args.num_actions, 'entropy_regularisation_strength': args.entropy_regularisation_strength,
        'device': args.device, 'height': args.height, 'width': args.height, 'channels': 3, 'filters': args.filters,
        'conv_layers': 2, 'scale': args.scale, 'clip_norm': args.clip_norm, 'clip_norm_type': args.clip_norm_type,
        'static_size': args.static_size, 'temporal_size': args.temporal_size, 'static_hidden_size': args.static_hidden_size,
        'rnn_hidden_size': args.temporal_hidden_size,
    }

    def network_creator(name='local_learning'):
        conf = copy.copy(network_conf)
        conf['name'] = name
        return ConvSingleAgentPolicyNetwork(conf)

    return network_creator, env_creator


# (flag strings, dest, type, default): the reference script's options and defaults (scripts/train_paac_conv.py:95-121)
_REFERENCE_FLAGS = (
    (('-d', '--device'), 'device', str, '/gpu:0'),
    (('--e',), 'e', float, 0.1),
    (('--alpha',), 'alpha', float, 0.99),
    (('-lr', '--initial_lr'), 'initial_lr', float, 1e-4),
    (('-lra', '--lr_annealing_steps'), 'lr_annealing_steps', int, 80000000),
    (('--entropy',), 'entropy_regularisation_strength', float, 0.02),
    (('--clip_norm',), 'clip_norm', float, 40.0),
    (('--clip_norm_type',), 'clip_norm_type', str, 'global'),
    (('--gamma',), 'gamma', float, 0.99),
    (('--max_global_steps',), 'max_global_steps', int, 80000000),
    (('--max_local_steps',), 'max_local_steps', int, 5),
    (('--single_life_episodes',), 'single_life_episodes', bool_arg, False),
    (('-ec', '--emulator_counts'), 'emulator_counts', int, 32),
    (('-ew', '--emulator_workers'), 'emulator_workers', int, 8),
    (('-df', '--debugging_folder'), 'debugging_folder', str, 'logs/'),
    (('-rs', '--random_start'), 'random_start', bool_arg, True),
    (('--scale',), 'scale', float, 1000.0),
    (('--height',), 'height', int, 84),
    (('--filters',), 'filters', int, 32),
    (('--rnn-length',), 'rnn_length', int, 5),
    (('--static-size',), 'static_size', int, 2),
    (('--temporal-size',), 'temporal_size', int, 2),
    (('--static-hidden-size',), 'static_hidden_size', int, 32),
    (('--temporal-hidden-size',), 'temporal_hidden_size', int, 32),
)


_BASELINE_HELP = ("play the scripted do-nothing baseline (drift / hold) on the eval env before the first update (one kernel launch) and "
                  "write eval/baseline_total_reward and eval/total_reward_minus_baseline at every evaluation (needs --eval-every > 0)")


def check_baseline_flags(args):
    """The five yardstick flags play the monitor's eval env: refused without it."""
    for flag, dest in (("--baseline", "baseline"), ("--rule-baseline", "rule_baseline"), ("--plan-baseline", "plan_baseline"),
                       ("--search-baseline", "search_baseline"), ("--cem-plan-baseline", "cem_plan_baseline")):
        if getattr(args, dest, None) and not args.eval_every > 0:
            raise SystemExit("%s plays the eval env of the monitor: it needs --eval-every > 0" % flag)


def get_arg_parser(baseline_help=_BASELINE_HELP, rule_baseline=True, eval_envs=True):
    """eval_envs: this script's --eval-envs; the scripts that build their parser from this one and have an --eval-envs of their own
    (train_paac_field, train_paac_solow) switch it off."""
    p = argparse.ArgumentParser(description="PAAC on Swarm-v0 with the conv policy (device engine)")
    for flags, dest, kind, default in _REFERENCE_FLAGS:
        p.add_argument(*flags, dest=dest, type=kind, default=default)
    p.add_argument('--reward-layout', default='broadcast', choices=['broadcast', 'reference'], dest="reward_layout",
                   help="'reference' reproduces paac.py:331-338's (T, E*10) indexing (quirk Q4)")
    p.add_argument('--eval-every', default=30.0, type=float, dest="eval_every",
                   help="seconds between eval episodes on Swarm-eval-v0 (paac.py:277-282); 0 disables the monitor")
    if eval_envs:
        p.add_argument('--eval-envs', default=0, type=int, dest="eval_envs",
                       help="0: one eval episode driven from the host, step by step (the reference's monitor).  N >= 1: N seeded episodes of "
                            "Swarm-eval-v0 per evaluation played on the device and read back once; env 0 is the registration's episode (the "
                            "same episode, bit for bit), the one the scalars and swarm-eval.json speak of; above 1 eval/mean_total_reward is "
                            "written too (needs --eval-every > 0)")
    p.add_argument('--baseline', action='store_true', help=baseline_help)
    if rule_baseline:      # Swarm only: train_paac_solow builds its parser from this one without it
        p.add_argument('--rule-baseline', action='store_true', dest="rule_baseline",
                       help="play the feedback-rule baseline (goldsrl.baselines.DEFAULT_SWARM_RULES: drift, hold and rules that steer the agents "
                            "relative to the swarm) on the eval env before the first update (one kernel launch), log the best rule and write "
                            "eval/baseline_total_reward and eval/total_reward_minus_baseline at every evaluation (needs --eval-every > 0); with "
                            "--baseline as well, the rule baseline is the one written")
        p.add_argument('--plan-baseline', type=plan_arg, default=None, dest="plan_baseline", metavar="H[:K]",
                       help="play the receding-horizon rule planner (goldsrl.baselines.SwarmRulePlanner: every default rule H steps ahead, the "
                            "best committed for K steps, default K = H, again) on the eval env before the first update (one call), log its "
                            "total and write eval/baseline_total_reward and eval/total_reward_minus_baseline at every evaluation (needs "
                            "--eval-every > 0); with --rule-baseline or --baseline as well, the plan is the one written: it is the highest "
                            "of the three")
        p.add_argument('--search-baseline', type=search_arg, default=None, dest="search_baseline", metavar="G[:C[:K]]",
                       help="tune the best default rule's five real numbers on the eval env before the first update "
                            "(goldsrl.baselines.SwarmRuleSearch: G generations of C candidates refitted over K elites, default 32 and 8; one "
                            "call), log the found rule and write eval/search_baseline_total_reward and eval/total_reward_minus_search_baseline "
                            "at every evaluation (needs --eval-every > 0); it also supplies eval/baseline_total_reward and "
                            "eval/total_reward_minus_baseline when no other baseline flag is given, and leaves them alone otherwise")
        p.add_argument('--cem-plan-baseline', type=cem_plan_arg, default=None, dest="cem_plan_baseline", metavar="H[:K[:G[:C[:M]]]]",
                       help="play the search planner (goldsrl.baselines.SwarmSearchPlanner: at every decision G generations of C candidates "
                            "refitted over M elites, every candidate and default rule H steps ahead, the better committed for K steps; defaults "
                            "K = H, 2, 12 and 4; one call) on the eval env before the first update, log its total and write "
                            "eval/cem_plan_baseline_total_reward and eval/total_reward_minus_cem_plan_baseline at every evaluation (needs "
                            "--eval-every > 0); it also supplies eval/baseline_total_reward and eval/total_reward_minus_baseline when no other "
                            "baseline flag is given, and leaves them alone otherwise")
    p.add_argument('--checkpoint-every', default=0, type=int, dest="checkpoint_every", help="updates between flat-weights checkpoints")
    p.add_argument('--checkpoint-path', default='checkpoint.npz', type=str, dest="checkpoint_path")
    p.add_argument('--resume', default=None, type=str, help="flat-weights checkpoint to start from")
    p.add_argument('--summaries', default=True, type=bool_arg,
                   help="write global_norm / loss scalars per update to <debugging_folder> (JSON lines + TensorBoard event file)")
    return p


def main(args):
    check_baseline_flags(args)
    if getattr(args, "eval_envs", 0) > 0 and not args.eval_every > 0:
        raise SystemExit("--eval-envs sizes the eval set of the monitor: it needs --eval-every > 0")
    network_creator, env_creator = get_network_and_environment_creator(args)
    learner = GridPAACLearner(network_creator, env_creator, args, SwarmRunner,
                              state_processor=None if args.emulator_counts > 4096 else SwarmStateProcessor(grid_size=args.height))
    logging.info('Starting training')
    learner.train()
    logging.info('Finished training')


if __name__ == '__main__':
    main(get_arg_parser().parse_args())
