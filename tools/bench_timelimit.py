#!/usr/bin/env python3
"""The cost of the final-observation store of time-limit bootstrapping, in one process: time per launch (HIP
events around each launch, random actions, every actor re-armed before each) of the rollout step with the policy fused
into it, without the store (unreal_*_policy_rollout_step) and with it (unreal_*_policy_rollout_step_tl), for the arcade
games and a first-person navigation maze (N = 7, goal_respawn), at B = 512 and B = 4096 and a step limit short enough
that time-outs occur (--max-episode-steps, default 20; cut_per_launch: the actors cut off per launch, on average).  The
two forms are timed in turn, twice per row, and the table is printed --repeat times.

  python tools/bench_timelimit.py [--launches 200] [--repeat 3] [--max-episode-steps 20] [--game breakout,duel,invaders]

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_fp_maze import DEV, layouts    # noqa: E402


def fused_ms(env, B, A, launches, entry):
    """Mean HIP-event time of one policy-fused rollout step of `env` (random feature rows and weights)."""
    from unreal_amd import ops
    rs = np.random.RandomState(0)
    dev = lambda a, dt: torch.from_numpy(np.asarray(a)).to(DEV, dt)
    net = type("Net", (), {"p": dict(W_base_fc_p=dev(rs.uniform(-.3, .3, 256 * A), torch.float32),
                                     b_base_fc_p=dev(rs.uniform(-.1, .1, A), torch.float32),
                                     W_base_fc_v=dev(rs.uniform(-.3, .3, 256), torch.float32),
                                     b_base_fc_v=dev(rs.uniform(-.1, .1, 1), torch.float32))})
    X = dev(rs.uniform(-1, 1, B * 256), torch.float32)
    us = [dev(rs.uniform(0, 1, B), torch.float64) for _ in range(8)]
    z = lambda dt, n=B: torch.zeros(n, dtype=dt, device=DEV)
    pi, v, a, r, t = z(torch.float32, A * B), z(torch.float32), z(torch.int32), z(torch.float32), z(torch.int32)
    active, log, n, te = torch.ones(B, dtype=torch.int32, device=DEV), z(torch.int32), z(torch.int32), z(torch.int32)
    cuts = torch.zeros((), dtype=torch.int64, device=DEV)

    def step(k):
        active.fill_(1)
        env.policy_rollout_step(net, X, 256, us[k % 8], pi, v, a, r, t, active, log, n, te, A=A)
    for k in range(40):                                  # (past the first limit)
        step(k)
    ops.kernel_timer_start(entry)
    for k in range(launches):
        step(k)
        cuts += (t == 2).sum()                           # (bookkeeping between the timed launches)
    res = ops.kernel_timer_stop()
    assert res["launches"] == launches, res
    return res["ms"] / launches, int(cuts) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--max-episode-steps", type=int, default=20)
    ap.add_argument("--game", default="breakout,duel,invaders")
    args = ap.parse_args()
    from unreal_amd.environment.arcade_environment import ArcadeConfig, BatchedArcadeEnvironment
    from unreal_amd.environment.maze_environment import MazeConfig, batched_maze_environment
    limit = args.max_episode_steps
    nav = MazeConfig(layouts(7, apples=4), view="first_person", random_start=True, random_goal=True, show_goal=True,
                     goal_respawn=True, max_episode_steps=limit)
    for rep in range(args.repeat):
        for B in (512, 4096):
            for name in args.game.split(",") + ["nav_maze"]:
                maze = name == "nav_maze"
                stem = "unreal_maze_policy_rollout_step" if maze else "unreal_arcade_policy_rollout_step"
                row = dict(bench="timelimit_store", env=name, B=B, max_episode_steps=limit, repeat=rep)
                envs = {}
                for store in (False, True):
                    if maze:
                        envs[store] = batched_maze_environment(B, 3, DEV, config=nav, seed=1, final_obs=store)
                    else:
                        envs[store] = BatchedArcadeEnvironment(B, 3, DEV, config=ArcadeConfig(game=name, max_episode_steps=limit),
                                                               final_obs=store)
                for k in range(2):                               # the two forms in turn, twice
                    for store in (False, True):
                        ms, cuts = fused_ms(envs[store], B, 4, args.launches, stem + ("_tl" if store else ""))
                        row["%s_us_%d" % ("store" if store else "plain", k)] = round(1e3 * ms, 2)
                        if store:
                            row["cut_per_launch_%d" % k] = round(cuts, 1)
                print(json.dumps(row), flush=True)
                del envs
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
