"""`python -m goldsrl.scripts.make_swarm_gif` -- the reference's scripts/make_swarm_gif.py on the device: reset `Swarm-eval-v0`,
replay the actions of swarm-eval.json (the best eval episode SwarmPolicyMonitor kept) in ONE kernel launch, print the episode's
length, mean and total reward beside the file's score, and write the episode as a GIF (numpy frames, PIL writer; no matplotlib).

The score is reproduced only in the arithmetic the episode was recorded in: the eval monitor steps float64 rows (--dtype float64,
the default), whereas a file whose rows went through the worker's float32 shared array was stepped with float32 wind / dt
arithmetic (quirk Q7) and replayed as float64 it differs -- replay such a file with --dtype float32.  The exit status is 0 either
way; the last line says `score reproduced` (relative difference within 1e-9) or `score differs`."""
import argparse

import numpy as np

from goldsrl.replay import SwarmReplay, frames, load_actions, save_gif


def get_arg_parser():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--actions", type=str, default="swarm-eval.json")
    p.add_argument("--out", type=str, default="swarm.gif")
    p.add_argument("--dtype", choices=("float64", "float32"), default="float64",
                   help="the arithmetic of the action rows: float64 as the eval monitor steps them, float32 as the worker's shared "
                        "array gives them (quirk Q7); a file recorded in one and replayed in the other prints `score differs`")
    p.add_argument("--frames-npy", dest="frames_npy", metavar="PATH", help="also keep the frames, (T, 320, 720, 3) uint8, with np.save")
    p.add_argument("--no-gif", dest="gif", action="store_false", help="do not write the GIF")
    p.add_argument("--device", type=int, default=0)
    return p


def main(argv=None):
    args = get_arg_parser().parse_args(argv)
    score, actions = load_actions(args.actions)
    from goldsrl.envs import registry
    cls, max_steps, kwargs = registry["Swarm-eval-v0"]
    env = cls(max_episode_steps=max_steps, device_id=args.device, **kwargs)
    env.reset()
    out = SwarmReplay(env).play(actions, trace_env=0, dtype=args.dtype)
    n = int(out["length"][0, 0])
    rewards, total = out["rewards"][0, 0, :n], float(out["totals"][0, 0])
    print("episode length %d of %d recorded actions (%s)" % (n, len(actions), "done" if out["finished"][0, 0] else "the script ran out"))
    print("mean reward %.17g, total reward %.17g" % (float(np.mean(rewards)), total))
    diff = total - score
    print("recorded score %.17g, difference %.3g" % (score, diff))
    picture = frames(out["x_traj"][0, :n], out["xa_traj"][0, :n])
    if args.frames_npy:
        np.save(args.frames_npy, picture)
    if args.gif:
        save_gif(picture, args.out)
        print("wrote %s (%d frames)" % (args.out, n))
    print("score reproduced" if abs(diff) <= 1e-9 * abs(score) else "score differs")
    return total, score


if __name__ == "__main__":
    main()
