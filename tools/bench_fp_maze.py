#!/usr/bin/env python3
"""First-person vs top-down device mazes, in one process:

  * the step kernel's time per launch (HIP events around each launch, random actions) for the top-down and the
    first-person view of the same configured mazes, at B = 512 and B = 4096, N = 7 and N = 21;
  * Trainer.process() ms for full UNREAL at B = 4096 in both views (replay history --history, filled untimed);
  * navigation rows: the step of a navigation block (apples, rewards (10, 1, 0), goal_respawn, Lab's six
    actions) next to the plain first-person step of the same layouts, and Trainer.process() at A = 6;
  * generated mazes (--gen-only): the step of a generated block next to the static first-person step of the
    same N and B, (a) at a 200-step limit, where resets are rare, and (b) at max_episode_steps=1, where every launch
    resets every actor and the generated block also regenerates its layout: (b) minus its static counterpart is the cost
    of generation per reset.  Then Trainer.process() on a generated config at B = 4096;
  * styled walls (--style-only): the step of a styled block next to the unstyled step of the same N, B and
    step limit, static (the same layouts, three wall cells in four carrying a digit 1..7) and generated (landmark
    density 64);
  * goal sense (--sense-only): the step of a goal_sense block next to the step of the same navigation block
    without the option, static and generated; the objective launch on its own; a full-batch reset() of a generated
    N = 21 maze with and without the option (the difference is the breadth-first search); Trainer.process() on both;
  * foraging (--forage-only): the step of a forage block (three more kinds of pickup, one of them ending the
    episode) next to the step of the navigation block with the same pickup cells, all apples, static and generated; the
    two blocks are timed in turn, twice per row, and the whole table is printed --repeat times; Trainer.process() on both.

  python tools/bench_fp_maze.py [--launches 200] [--steps 10] [--warmup 3] [--history 100]
                                [--nav-only | --gen-only | --style-only | --sense-only | --forage-only [--repeat 2]]

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda:0"


def layouts(N, L=8, seed=0, apples=0):
    from maze_model import random_layout
    rs = np.random.RandomState(seed + N)
    return [random_layout(N, rs, marks="A" * apples) for _ in range(L)]


NAV_APPLES = {7: 8, 21: 64}
# seven styles: plain, striped and half-dark patterns
STYLES = [(200, 100, 50, 0xAA), (0, 255, 0, 0x00), (255, 255, 255, 0xFF), (10, 20, 250, 0x0F), (90, 90, 90, 0x81),
          (255, 0, 255, 0x3C), (120, 60, 200, 0x55)]


def styled_layouts(N, L=8, seed=0):
    """layouts(N, L, seed) with three wall cells in four drawn in a style 1..7."""
    rs = np.random.RandomState(seed + 1000 + N)
    out = []
    for lay in layouts(N, L, seed):
        k = rs.randint(0, 28, len(lay))
        out.append("".join(str(1 + d % 7) if ch == "+" and d < 21 else ch for ch, d in zip(lay, k)))
    return out


def kernel_ms(env, B, launches, A=4, entry="unreal_maze_step"):
    """Mean HIP-event time of one step launch (the entry point env.process calls), or of the launches of `entry`."""
    from unreal_amd import ops
    rs = np.random.RandomState(0)
    acts = [torch.from_numpy(rs.randint(0, A, B).astype(np.int32)).to(DEV) for _ in range(8)]
    r = torch.zeros(B, dtype=torch.float32, device=DEV)
    t = torch.zeros(B, dtype=torch.int32, device=DEV)
    for k in range(10):
        env.process(acts[k % 8], None, r, t, track_score=True)
    ops.kernel_timer_start(entry)
    for k in range(launches):
        env.process(acts[k % 8], None, r, t, track_score=True)
    res = ops.kernel_timer_stop()
    assert res["launches"] == launches, res
    return res["ms"] / launches


def reset_ms(env, launches):
    """Mean HIP-event time of the reset launch of a full-batch env.reset()."""
    from unreal_amd import ops
    for _ in range(10):
        env.reset()
    ops.kernel_timer_start("unreal_maze_reset")
    for _ in range(launches):
        env.reset()
    res = ops.kernel_timer_stop()
    assert res["launches"] == launches, res
    return res["ms"] / launches


def trainer_ms(env_name, B, history, steps, warmup):
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.options import get_options
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer, log_uniform
    flags = get_options("training", preset="lab", argv=["--env_type", "maze", "--env_name", env_name])
    Environment.action_size = -1
    A = Environment.get_action_size("maze", env_name)
    net = UnrealModel(A, Environment.get_objective_size("maze", env_name), -1, flags.use_lstm, flags.use_pixel_change, flags.use_value_replay,
                      flags.use_reward_prediction, flags.pixel_change_lambda, flags.entropy_beta, DEV, seed=1)
    lr0 = log_uniform(flags.initial_alpha_low, flags.initial_alpha_high, flags.initial_alpha_log_rate)
    applier = RMSPropApplier(None, decay=flags.rmsp_alpha, momentum=0.0, epsilon=flags.rmsp_epsilon,
                             clip_norm=flags.grad_norm_clip, device=DEV)
    tr = Trainer(0, net, lr0, None, applier, "maze", env_name, flags.use_lstm, flags.use_pixel_change,
                 flags.use_value_replay, flags.use_reward_prediction, flags.pixel_change_lambda, flags.entropy_beta,
                 flags.local_t_max, flags.n_step_TD, flags.gamma, flags.gamma_pc, history, flags.max_time_step, DEV,
                 batch_size=B, seed=0xA3C)
    tr.prepare()
    while not tr._full:
        tr.process(None, 0)
    for _ in range(warmup):
        tr.process(None, 0)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        tr.process(None, 0)
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / steps
    out = e0.elapsed_time(e1) / steps, wall
    del tr, net, applier
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--history", type=int, default=100)
    ap.add_argument("--skip-trainer", action="store_true")
    ap.add_argument("--nav-only", action="store_true", help="only the navigation rows and their plain references")
    ap.add_argument("--gen-only", action="store_true", help="only the generated-maze rows and their static references")
    ap.add_argument("--style-only", action="store_true", help="only the styled rows and their unstyled references")
    ap.add_argument("--sense-only", action="store_true", help="only the goal-sense rows and their references")
    ap.add_argument("--forage-only", action="store_true", help="only the forage rows and their navigation references")
    ap.add_argument("--repeat", type=int, default=2, help="--forage-only: how often the whole table is measured")
    args = ap.parse_args()
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.maze_environment import MazeConfig, batched_maze_environment
    kw = dict(random_start=True, random_goal=True, show_goal=True, max_episode_steps=200)
    nav_kw = dict(goal_reward=10, apple_reward=1, hit_reward=0, goal_respawn=True, action_set="lab")
    if args.forage_only:
        # lemons at -1, a +5, and a melon at +20 that ends the episode: every fourth pickup cell of the navigation block each
        kinds = [(-1, (255, 255, 0), False), (5, (0, 255, 255), False), (20, (255, 0, 255), True)]
        okw = dict(kw, **nav_kw)

        def forage_layout(lay):
            k, out = 0, []
            for ch in lay:
                out.append("ABCD"[k % 4] if ch == "A" else ch)
                k += ch == "A"
            return "".join(out)
        for run in range(args.repeat):
            for N in (7, 21):   # forage vs the navigation block of the same cells, all 'A': same process, in turn
                for B in (512, 4096):
                    for kind in ("static", "generated"):
                        n = NAV_APPLES[N]
                        if kind == "static":
                            lays = layouts(N, apples=n)
                            cfgs = dict(nav=MazeConfig(lays, view="first_person", **okw),
                                        forage=MazeConfig([forage_layout(l) for l in lays], view="first_person",
                                                          pickups=kinds, **okw))
                        else:
                            cfgs = dict(nav=MazeConfig(None, view="first_person", generate=N, gen_apples=n, **okw),
                                        forage=MazeConfig(None, view="first_person", generate=N, gen_apples=n // 4,
                                                          pickups=kinds, gen_pickups=(n // 4,) * 3, **okw))
                        envs = dict((k, batched_maze_environment(B, 3, DEV, config=c, seed=1)) for k, c in cfgs.items())
                        us = dict(nav=[], forage=[])
                        for _ in range(2):
                            for what in ("nav", "forage"):
                                us[what].append(kernel_ms(envs[what], B, args.launches, A=6) * 1e3)
                        del envs
                        nav_us, forage_us = sum(us["nav"]) / 2, sum(us["forage"]) / 2
                        print(json.dumps(dict(what="forage_step_kernel", run=run, kind=kind, N=N, B=B,
                                              nav_us=round(nav_us, 2), forage_us=round(forage_us, 2),
                                              ratio=round(forage_us / nav_us, 3),
                                              passes=dict((k, [round(v, 2) for v in vs]) for k, vs in us.items()))),
                              flush=True)
        if not args.skip_trainer:
            lays = layouts(7, apples=NAV_APPLES[7])
            for what in ("nav", "forage"):
                name = "bench_forage_" + what
                if what == "nav":
                    Environment.register_maze_config(name, lays, view="first_person", **okw)
                else:
                    Environment.register_maze_config(name, [forage_layout(l) for l in lays], view="first_person",
                                                     pickups=kinds, **okw)
                ms, wall = trainer_ms(name, 4096, args.history, args.steps, args.warmup)
                print(json.dumps(dict(what="trainer_process", view="first_person_nav", forage=what == "forage", A=6,
                                      N=7, B=4096, history=args.history, ms_per_call=round(ms, 3),
                                      wall_ms_per_call=round(wall, 3))), flush=True)
        return
    if args.sense_only:
        for N in (7, 21):       # goal sense vs the same navigation block without it: same layouts, same process
            for B in (512, 4096):
                for kind in ("static", "generated"):
                    res = {}
                    for what in ("plain", "sense"):
                        okw = dict(kw, **nav_kw)
                        if what == "sense":
                            okw.update(goal_sense=True, progress_reward=1)
                        cfg = MazeConfig(layouts(N, apples=NAV_APPLES[N]), view="first_person", **okw) \
                            if kind == "static" else MazeConfig(None, view="first_person", generate=N, **okw)
                        env = batched_maze_environment(B, 3, DEV, config=cfg, seed=1)
                        res[what] = kernel_ms(env, B, args.launches, A=6) * 1e3
                        if what == "sense":
                            res["objective"] = kernel_ms(env, B, args.launches, A=6, entry="unreal_maze_objective") * 1e3
                        del env
                    print(json.dumps(dict(what="sense_step_kernel", kind=kind, N=N, B=B, plain_us=round(res["plain"], 2),
                                          sense_us=round(res["sense"], 2), ratio=round(res["sense"] / res["plain"], 3),
                                          objective_launch_us=round(res["objective"], 2))), flush=True)
        for B in (512, 4096):   # the search: a full-batch reset of a generated N = 21 maze
            res = {}
            for what in ("plain", "sense"):
                cfg = MazeConfig(None, view="first_person", generate=21, **dict(kw, goal_sense=what == "sense"))
                env = batched_maze_environment(B, 3, DEV, config=cfg, seed=1)
                res[what] = reset_ms(env, args.launches) * 1e3
                del env
            print(json.dumps(dict(what="sense_reset_kernel", kind="generated", N=21, B=B, plain_us=round(res["plain"], 2),
                                  sense_us=round(res["sense"], 2), bfs_us=round(res["sense"] - res["plain"], 2))),
                  flush=True)
        if not args.skip_trainer:
            for what in ("plain", "sense"):
                name = "bench_sense_" + what
                okw = dict(kw, **nav_kw)
                if what == "sense":
                    okw.update(goal_sense=True, progress_reward=1)
                Environment.register_maze_config(name, layouts(7, apples=NAV_APPLES[7]), view="first_person", **okw)
                ms, wall = trainer_ms(name, 4096, args.history, args.steps, args.warmup)
                print(json.dumps(dict(what="trainer_process", view="first_person_nav", goal_sense=what == "sense", A=6,
                                      N=7, B=4096, history=args.history, ms_per_call=round(ms, 3),
                                      wall_ms_per_call=round(wall, 3))), flush=True)
        return
    if args.style_only:
        for N in (7, 21):       # styled vs unstyled first person, same N, B and step limit, same process
            for B in (512, 4096):
                for kind in ("static", "generated"):
                    res = {}
                    for what in ("unstyled", "styled"):
                        skw = dict(wall_styles=STYLES) if what == "styled" else {}
                        if kind == "static":
                            lays = styled_layouts(N) if what == "styled" else layouts(N)
                            cfg = MazeConfig(lays, view="first_person", **dict(kw, **skw))
                        else:
                            if what == "styled":
                                skw["gen_landmark_density"] = 64
                            cfg = MazeConfig(None, view="first_person", generate=N, **dict(kw, **skw))
                        env = batched_maze_environment(B, 3, DEV, config=cfg, seed=1)
                        res[what] = kernel_ms(env, B, args.launches) * 1e3
                        del env
                    print(json.dumps(dict(what="style_step_kernel", kind=kind, N=N, B=B,
                                          unstyled_us=round(res["unstyled"], 2), styled_us=round(res["styled"], 2),
                                          ratio=round(res["styled"] / res["unstyled"], 3))), flush=True)
        return
    if args.gen_only:
        for N in (7, 21):       # generated vs static first person, same N, B and step limit, same process
            for B in (512, 4096):
                for limit in (200, 1):
                    res = {}
                    for what in ("static", "generated"):
                        okw = dict(kw, max_episode_steps=limit)
                        cfg = MazeConfig(layouts(N), view="first_person", **okw) if what == "static" else \
                            MazeConfig(None, view="first_person", generate=N, **okw)
                        env = batched_maze_environment(B, 3, DEV, config=cfg, seed=1)
                        res[what] = kernel_ms(env, B, args.launches) * 1e3
                        del env
                    print(json.dumps(dict(what="gen_step_kernel", N=N, B=B, max_episode_steps=limit,
                                          static_us=round(res["static"], 2), generated_us=round(res["generated"], 2),
                                          diff_us=round(res["generated"] - res["static"], 2),
                                          ratio=round(res["generated"] / res["static"], 3))), flush=True)
        if not args.skip_trainer:
            for name, N in (("bench_gen7", 7), ("bench_gen21", 21)):
                Environment.register_maze_config(name, None, view="first_person", generate=N, **kw)
                ms, wall = trainer_ms(name, 4096, args.history, args.steps, args.warmup)
                print(json.dumps(dict(what="trainer_process", view="first_person_generated", N=N, B=4096,
                                      history=args.history, ms_per_call=round(ms, 3), wall_ms_per_call=round(wall, 3))),
                      flush=True)
        return
    for N in (7, 21):       # navigation vs plain first person: same layouts (apples only in the nav block), same process
        for B in (512, 4096):
            res = {}
            for what in ("plain", "nav"):
                lays = layouts(N, apples=NAV_APPLES[N] if what == "nav" else 0)
                cfg = MazeConfig(lays, view="first_person", **dict(kw, **(nav_kw if what == "nav" else {})))
                env = batched_maze_environment(B, 3, DEV, config=cfg, seed=1)
                res[what] = kernel_ms(env, B, args.launches, A=cfg.action_size) * 1e3
                del env
            print(json.dumps(dict(what="nav_step_kernel", N=N, B=B, plain_us=round(res["plain"], 2),
                                  nav_us=round(res["nav"], 2), ratio=round(res["nav"] / res["plain"], 3))), flush=True)
    if args.nav_only:
        if not args.skip_trainer:
            name = "bench_nav"
            Environment.register_maze_config(name, layouts(7, apples=NAV_APPLES[7]), view="first_person",
                                             **dict(kw, **nav_kw))
            ms, wall = trainer_ms(name, 4096, args.history, args.steps, args.warmup)
            print(json.dumps(dict(what="trainer_process", view="first_person_nav", A=6, N=7, B=4096,
                                  history=args.history, ms_per_call=round(ms, 3), wall_ms_per_call=round(wall, 3))),
                  flush=True)
        return
    for N in (7, 21):
        lays = layouts(N)
        for view in ("top_down", "first_person"):
            cfg = MazeConfig(lays, view=view, **kw)
            for B in (512, 4096):
                env = batched_maze_environment(B, 3, DEV, config=cfg, seed=1)
                ms = kernel_ms(env, B, args.launches)
                print(json.dumps(dict(what="step_kernel", view=view, N=N, B=B, us_per_launch=round(ms * 1e3, 2),
                                      GBps=round(B * 21168 * (2 if view == "first_person" else 1) / ms / 1e6, 1))),
                      flush=True)
                del env
    if args.skip_trainer:
        return
    lays = layouts(7)
    for view in ("top_down", "first_person"):
        name = "bench_fp_" + view
        Environment.register_maze_config(name, lays, view=view, **kw)
        ms, wall = trainer_ms(name, 4096, args.history, args.steps, args.warmup)
        print(json.dumps(dict(what="trainer_process", view=view, N=7, B=4096, history=args.history,
                              ms_per_call=round(ms, 3), wall_ms_per_call=round(wall, 3))), flush=True)


if __name__ == "__main__":
    main()
