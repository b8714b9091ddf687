"""`python -m goldsrl.scripts.swarm_rules` -- the feedback-rule baseline of the Swarm env (goldsrl/baselines.py:SwarmRuleBaseline)
on `Swarm-eval-v0`: every default rule plays the seeded eval episode in ONE kernel launch, and every rule's total reward is printed
-- the yardstick for eval/total_reward of train_paac_conv.  --json keeps the best rule's episode as {'score', 'actions'}, the
format of the swarm-eval.json SwarmPolicyMonitor writes; --gif hands that file to goldsrl.scripts.make_swarm_gif, which replays
the recorded actions, prints `score reproduced` and draws the episode.  --plan H[:K] also plays the receding-horizon planner over the
same rules (goldsrl/baselines.py:SwarmRulePlanner) and keeps ITS episode instead.  --search G[:C[:K]] tunes the best rule's five real
numbers (goldsrl/baselines.py:SwarmRuleSearch, one call), prints every generation's best and keeps the found rule's episode.
--cem-plan H[:K[:G[:C[:M]]]] plays the search planner (goldsrl/baselines.py:SwarmSearchPlanner, one call), which tunes the rule at
every decision, prints its total and keeps ITS episode.  The reference has no counterpart."""
import argparse
import json

import numpy as np

from goldsrl.baselines import DEFAULT_SWARM_RULES, SwarmRuleBaseline, SwarmRulePlanner, SwarmRuleSearch, SwarmSearchPlanner


def plan_arg(text):
    """--plan (and the trainers' --plan-baseline): 'H' or 'H:K' as (horizon, replan) with 1 <= K <= H; K defaults to H."""
    try:
        parts = [int(v) for v in text.split(":")]
    except ValueError:
        parts = []
    if len(parts) not in (1, 2) or not 1 <= parts[-1] <= parts[0]:
        raise argparse.ArgumentTypeError("expected H or H:K with 1 <= K <= H, got %r" % text)
    return parts[0], parts[-1]


def search_arg(text):
    """--search (and the trainers' --search-baseline): 'G', 'G:C' or 'G:C:K' as (generations, candidates, elites) with G >= 1,
    2 <= C <= 1024 and 1 <= K <= C; C defaults to 32 and K to min(8, C)."""
    try:
        parts = [int(v) for v in text.split(":")]
    except ValueError:
        parts = []
    if len(parts) not in (1, 2, 3):
        raise argparse.ArgumentTypeError("expected G, G:C or G:C:K, got %r" % text)
    G = parts[0]
    C = parts[1] if len(parts) > 1 else 32
    K = parts[2] if len(parts) > 2 else min(8, C)
    if G < 1 or not 2 <= C <= 1024 or not 1 <= K <= C:
        raise argparse.ArgumentTypeError("expected G >= 1, 2 <= C <= 1024 and 1 <= K <= C, got %r" % text)
    return G, C, K


def cem_plan_arg(text):
    """--cem-plan (and the trainers' --cem-plan-baseline): 'H[:K[:G[:C[:M]]]]' as (horizon, replan, generations, candidates, elites)
    with 1 <= K <= H, G >= 1, 2 <= C <= 1024 and 1 <= M <= C; K defaults to H, G to 2, C to 12 and M to min(4, C)."""
    try:
        parts = [int(v) for v in text.split(":")]
    except ValueError:
        parts = []
    if not 1 <= len(parts) <= 5:
        raise argparse.ArgumentTypeError("expected H[:K[:G[:C[:M]]]], got %r" % text)
    H = parts[0]
    K = parts[1] if len(parts) > 1 else H
    G = parts[2] if len(parts) > 2 else 2
    C = parts[3] if len(parts) > 3 else 12
    M = parts[4] if len(parts) > 4 else min(4, C)
    if not 1 <= K <= H or G < 1 or not 2 <= C <= 1024 or not 1 <= M <= C:
        raise argparse.ArgumentTypeError("expected 1 <= K <= H, G >= 1, 2 <= C <= 1024 and 1 <= M <= C, got %r" % text)
    return H, K, G, C, M


def get_arg_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--seed", type=int, default=192, help="the env's seed (192: Swarm-eval-v0's registration)")
    p.add_argument("--json", help="write the best rule's episode here as {'score', 'actions'}")
    p.add_argument("--gif", help="draw the best rule's episode with make_swarm_gif (seed 192 only; writes --json, default <gif>.json)")
    p.add_argument("--plan", type=plan_arg, default=None, metavar="H[:K]",
                   help="also play the receding-horizon planner over the same rules (every rule H steps ahead, the best committed for K "
                        "steps, default K = H, again; one call) and print its total beside the rules'; --json / --gif then keep the planned episode")
    p.add_argument("--search", type=search_arg, default=None, metavar="G[:C[:K]]",
                   help="also tune the best rule's five real numbers under its anchor: G generations of C candidates (default 32) refitted "
                        "over K elites (default 8), one call; prints every generation's best; --json / --gif then keep the found rule's "
                        "episode (after --plan as well, the found rule's is the one kept)")
    p.add_argument("--cem-plan", type=cem_plan_arg, default=None, dest="cem_plan", metavar="H[:K[:G[:C[:M]]]]",
                   help="also play the search planner from the best rule: at every decision G generations (default 2) of C candidates "
                        "(default 12) refitted over M elites (default 4), every candidate and every rule H steps ahead, the better "
                        "committed for K steps (default K = H), again; one call; --json / --gif then keep its episode (after --plan and "
                        "--search as well)")
    p.add_argument("--device", type=int, default=0)
    return p


def main(argv=None):
    parser = get_arg_parser()
    args = parser.parse_args(argv)
    if args.gif and args.seed != 192:
        parser.error("--gif replays the file on Swarm-eval-v0, whose seed is 192")
    from goldsrl.envs import registry
    cls, max_steps, kwargs = registry["Swarm-eval-v0"]
    kwargs = dict(kwargs, seed=args.seed)
    env = cls(max_episode_steps=max_steps, device_id=args.device, **kwargs)
    env.reset()
    b = SwarmRuleBaseline(env._eng, DEFAULT_SWARM_RULES)
    st = b.run(keep_actions=True)
    for i, rule in enumerate(b.rules):
        print("rule %2d  cancel %g gain %-3g anchor %d offset (%4g, %4g) radius %-3g  length %3d  total reward %.6f"
              % ((i,) + tuple(rule[:2]) + (int(rule[2]),) + tuple(rule[3:]) + (int(st["length"][0, i]), float(st["totals"][0, i]))))
    best, six, total = b.best_total()
    print("best: rule %d %s, total reward %.6f; hold %.6f, drift %.6f" % (best, six, total, float(st["totals"][0, 1]), float(st["totals"][0, 0])))
    n = int(st["length"][0, best])
    rewards, actions = st["rewards"][0, best, :n], st["actions"][0, best, :n]
    if args.plan:
        horizon, replan = args.plan
        pl = SwarmRulePlanner(env._eng, DEFAULT_SWARM_RULES, horizon, replan)
        ps = pl.run(keep_actions=True)
        n = int(ps["length"][0])
        rewards, actions = ps["rewards"][0, :n], ps["actions"][0, :n]
        c = ps["choices"][0]
        print("plan: horizon %d, replan %d: %d decisions, %d switches, rules chosen %s, length %d, total reward %.6f (%+.6f on the best rule)"
              % (horizon, replan, int((c >= 0).sum()), pl.switches(), sorted(set(int(v) for v in c[c >= 0])), n, pl.total(), pl.total() - total))
    if args.search:
        G, C, K = args.search
        se = SwarmRuleSearch(env._eng, six, G, C, K)
        ss = se.run()
        for g in range(G):
            print("search: generation %d best %.6f  (cancel %g gain %g anchor %d offset (%g, %g) radius %g)"
                  % ((g, float(ss["best_per_generation"][g])) + tuple(ss["candidates"][g, ss["order"][g, 0]])))
        found, fit = se.best()
        ps = se.play_best(keep_actions=True)
        n = int(ps["length"][0, 0])
        rewards, actions = ps["rewards"][0, 0, :n], ps["actions"][0, 0, :n]
        print("search: %d generations of %d candidates, %d elites: rule %s, length %d, total reward %.6f (%+.6f on the best rule)"
              % (G, C, K, found, n, fit, fit - total))
    if args.cem_plan:
        H, K, G, C, M = args.cem_plan
        cp = SwarmSearchPlanner(env._eng, DEFAULT_SWARM_RULES, six, H, K, G, C, M)
        cs = cp.run(keep_actions=True)
        n = int(cs["length"][0])
        rewards, actions = cs["rewards"][0, :n], cs["actions"][0, :n]
        ch = cs["choices"][0]
        print("cem-plan: horizon %d, replan %d, %d generations of %d, %d elites: %d decisions, %d searched, library rules chosen %s, length %d, "
              "total reward %.6f (%+.6f on the best rule)"
              % (H, K, G, C, M, int((ch >= 0).sum()), cp.searched(), sorted(set(int(v) for v in ch[(ch >= 0) & (ch < len(DEFAULT_SWARM_RULES))])),
                 n, cp.total(), cp.total() - total))
    score = float(np.sum(rewards))                                      # the monitor's total_reward
    path = args.json or (args.gif + ".json" if args.gif else None)
    if path:
        with open(path, "w") as f:
            json.dump({"score": score, "actions": actions.tolist()}, f)
        print("wrote %s (%d actions, score %.17g)" % (path, n, score))
    if args.gif:
        from goldsrl.scripts import make_swarm_gif
        make_swarm_gif.main(["--actions", path, "--out", args.gif, "--device", str(args.device)])
    return best, six, score


if __name__ == "__main__":
    main()
