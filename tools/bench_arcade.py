#!/usr/bin/env python3
"""The device arcade next to the device mazes, in one process:

  * time per launch (HIP events around each launch, random actions) of the arcade step and of the arcade step with the
    policy fused into it, next to the static first-person maze step (N = 7) and the top-down maze step, at B = 512 and
    B = 4096.  The kernels are timed in turn and the whole table is printed --repeat times;
  * Trainer.process() ms for full UNREAL at B = 4096 (replay history --history, filled untimed) on the arcade and on the
    first-person maze.

  python tools/bench_arcade.py [--launches 200] [--steps 10] [--warmup 3] [--history 100] [--repeat 2] [--skip-trainer]
                               [--game breakout] [--action-repeat 1] [--mix breakout,duel,invaders,crossing] [--selfplay]
                               [--versus]

`--game duel` / `--game invaders` / `--game crossing` measures the two-paddle duel, invaders (§7n) or crossing
(§7x; with a walker 4 px wide, the tools' crossing config) on its default config instead
of Breakout; its lines then also hold the game's name.  `--game A,B[,C]` times the step and the fused step of these games in
turn in one process (lines of bench "arcade_games", keys <game>_us_<k> and <game>_fused_us_<k>; no maze kernels, no trainer).  `--action-repeat K` measures the game at K ticks per agent step; its lines then also hold
action_repeat and, for the arcade kernels, µs per game tick: the launch's time over K (a step runs fewer ticks only where
one ends the game, about once in a hundred steps on the default configs).  Prints one JSON line per measurement.
`--mix A,B[,C...]` measures game mixtures instead, on the games' default configs: (a) per distinct game, the
rollout entry of the mixture with that one task (unreal_arcade_mix_rollout_step, K = 1) against the plain entry on the same
config, the two alternating --repeat times in one process, at 4096 and at 64 actors, with the mix entry without its
statistics arrays and the two _tl forms beside them (lines of bench "arcade_mix_k1"); (b) the
K-task mixture's rollout step against each of its tasks' single-game steps and their mean (bench "arcade_mix_step") and,
unless --skip-trainer, Trainer.process() at 4096 actors on the mixture and on each task (bench "arcade_mix_process").
`--selfplay` measures the self-play duel instead, on the default config: its rollout step, plain
(unreal_arcade_selfplay_rollout_step) and with the policy fused into it, beside the duel's two in the same process, the four
alternating --repeat times, at 4096 and at 64 actors (lines of bench "arcade_selfplay_step") and, unless --skip-trainer,
Trainer.process() at 4096 actors on both (bench "arcade_selfplay_process").
`--versus` measures the versus step instead: unreal_arcade_versus_rollout_step, plain and fused, beside the
self-play and the duel steps, alternating --repeat times in one process at B = 4096 and 64 launched actors (a versus
launch of B actors steps B games, a self-play launch B / 2: the lines also hold µs per game), bench "arcade_versus_step";
and, unless --skip-trainer, Trainer.process() at 4096 actors on the self-play game with opponent_pool K = 0 (mirror
self-play), 1 and 4, the fill untimed (bench "arcade_versus_process", with the cost per slot)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_fp_maze import DEV, kernel_ms, layouts, trainer_ms as maze_trainer_ms    # noqa: E402


def fused_ms(env, B, launches, entry="unreal_arcade_policy_rollout_step"):
    """Mean HIP-event time of one policy-fused arcade step (random feature rows and weights, all actors active)."""
    from unreal_amd import ops
    rs = np.random.RandomState(0)
    dev = lambda a, dt: torch.from_numpy(np.asarray(a)).to(DEV, dt)
    net = type("Net", (), {"p": dict(W_base_fc_p=dev(rs.uniform(-.3, .3, 1024), torch.float32),
                                     b_base_fc_p=dev(rs.uniform(-.1, .1, 4), torch.float32),
                                     W_base_fc_v=dev(rs.uniform(-.3, .3, 256), torch.float32),
                                     b_base_fc_v=dev(rs.uniform(-.1, .1, 1), torch.float32))})
    X = dev(rs.uniform(-1, 1, B * 256), torch.float32)
    us = [dev(rs.uniform(0, 1, B), torch.float64) for _ in range(8)]
    z = lambda dt, n=B: torch.zeros(n, dtype=dt, device=DEV)
    pi, v, a, r, t = z(torch.float32, 4 * B), z(torch.float32), z(torch.int32), z(torch.float32), z(torch.int32)
    active, log, n, te = torch.ones(B, dtype=torch.int32, device=DEV), z(torch.int32), z(torch.int32), z(torch.int32)

    def step(k):
        active.fill_(1)
        env.policy_rollout_step(net, X, 256, us[k % 8], pi, v, a, r, t, active, log, n, te)
    for k in range(10):
        step(k)
    ops.kernel_timer_start(entry)
    for k in range(launches):
        step(k)
    res = ops.kernel_timer_stop()
    assert res["launches"] == launches, res
    return res["ms"] / launches


def rollout_ms(env, B, launches, entry):
    """Mean HIP-event time of one rollout step through `entry` (random actions, all actors re-armed before every step)."""
    from unreal_amd import ops
    rs = np.random.RandomState(0)
    acts = [torch.from_numpy(rs.randint(0, 4, B).astype(np.int32)).to(DEV) for _ in range(8)]
    z = lambda dt: torch.zeros(B, dtype=dt, device=DEV)
    r, t, active, log, n, te = z(torch.float32), z(torch.int32), z(torch.int32), z(torch.int32), z(torch.int32), z(torch.int32)

    def step(k):
        active.fill_(1)
        env.rollout_step(acts[k % 8], r, t, active, log, n, te)
    for k in range(10):
        step(k)
    ops.kernel_timer_start(entry)
    for k in range(launches):
        step(k)
    res = ops.kernel_timer_stop()
    assert res["launches"] == launches, res
    return res["ms"] / launches


def own_settings(game):
    """What the tools' default config of a game sets beside the game's own defaults: crossing's walker is 4 px wide."""
    return dict(paddle_width=4) if game == "crossing" else {}


def bench_mix(args):
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.arcade_environment import ArcadeMix, BatchedArcadeEnvironment
    games = args.mix.split(",")
    plain, mixed = "unreal_arcade_rollout_step", "unreal_arcade_mix_rollout_step"
    for g in sorted(set(games)):
        Environment.register_arcade_config("bench_" + g, game=g, **own_settings(g))
    conf = {g: Environment.ARCADE_CONFIG["bench_" + g] for g in set(games)}
    Environment.register_arcade_mix("bench_mix", ["bench_" + g for g in games])
    for B in (4096, 64):                                            # (a) one task through the mix entry against the plain entry
        for g in sorted(conf):
            # the plain entry, the mix entry, the mix entry without the statistics arrays, and the two _tl forms
            envs = [BatchedArcadeEnvironment(B, 3, DEV, config=c, final_obs=tl)
                    for c, tl in ((conf[g], False), (ArcadeMix([conf[g]]), False), (ArcadeMix([conf[g]]), False),
                                  (conf[g], True), (ArcadeMix([conf[g]]), True))]
            envs[2].ring.done_return = envs[2].ring.done_episodes = None
            row = dict(bench="arcade_mix_k1", game=g, B=B)
            for k in range(args.repeat):
                for key, env, entry in (("plain", envs[0], plain), ("mix", envs[1], mixed), ("mix_nostats", envs[2], mixed),
                                        ("plain_tl", envs[3], plain + "_tl"), ("mix_tl", envs[4], mixed + "_tl")):
                    row["%s_us_%d" % (key, k)] = round(1e3 * rollout_ms(env, B, args.launches, entry), 2)
            print(json.dumps(row), flush=True)
            del envs
            torch.cuda.empty_cache()
    for B in (4096, 64):                                            # (b) the mixture against its tasks
        envs = {g: BatchedArcadeEnvironment(B, 3, DEV, config=conf[g]) for g in sorted(conf)}
        mix_env = BatchedArcadeEnvironment(B, 3, DEV, config=Environment.ARCADE_CONFIG["bench_mix"])
        for k in range(args.repeat):
            row = dict(bench="arcade_mix_step", tasks=games, B=B, repeat=k)
            for g in envs:
                row[g + "_us"] = round(1e3 * rollout_ms(envs[g], B, args.launches, plain), 2)
            row["mix_us"] = round(1e3 * rollout_ms(mix_env, B, args.launches, mixed), 2)
            row["tasks_mean_us"] = round(sum(row[g + "_us"] for g in games) / len(games), 2)
            row["mix_over_mean"] = round(row["mix_us"] / row["tasks_mean_us"], 3)
            row["mix_over_slowest"] = round(row["mix_us"] / max(row[g + "_us"] for g in games), 3)
            print(json.dumps(row), flush=True)
        del envs, mix_env
        torch.cuda.empty_cache()
    if not args.skip_trainer:
        for k in range(args.repeat):
            row = dict(bench="arcade_mix_process", tasks=games, B=4096, history=args.history, repeat=k)
            for g in sorted(conf):
                row[g + "_ms"] = round(arcade_trainer_ms("bench_" + g, 4096, args.history, args.steps, args.warmup)[1], 2)
            row["mix_ms"] = round(arcade_trainer_ms("bench_mix", 4096, args.history, args.steps, args.warmup)[1], 2)
            row["tasks_mean_ms"] = round(sum(row[g + "_ms"] for g in games) / len(games), 2)
            row["mix_over_mean"] = round(row["mix_ms"] / row["tasks_mean_ms"], 3)
            print(json.dumps(row), flush=True)


def bench_selfplay(args):
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.arcade_environment import BatchedArcadeEnvironment
    Environment.register_arcade_selfplay("bench_selfplay")
    Environment.register_arcade_config("bench_duel", game="duel")
    plain, sp = "unreal_arcade%s_rollout_step", "unreal_arcade%s_policy_rollout_step"
    for B in (4096, 64):
        duel = BatchedArcadeEnvironment(B, 3, DEV, config=Environment.ARCADE_CONFIG["bench_duel"])
        selfplay = BatchedArcadeEnvironment(B, 3, DEV, config=Environment.ARCADE_CONFIG["bench_selfplay"])
        row = dict(bench="arcade_selfplay_step", B=B)
        for k in range(args.repeat):
            row["duel_us_%d" % k] = round(1e3 * rollout_ms(duel, B, args.launches, plain % ""), 2)
            row["selfplay_us_%d" % k] = round(1e3 * rollout_ms(selfplay, B, args.launches, plain % "_selfplay"), 2)
            row["duel_fused_us_%d" % k] = round(1e3 * fused_ms(duel, B, args.launches, sp % ""), 2)
            row["selfplay_fused_us_%d" % k] = round(1e3 * fused_ms(selfplay, B, args.launches, sp % "_selfplay"), 2)
        print(json.dumps(row), flush=True)
        del duel, selfplay
        torch.cuda.empty_cache()
    if not args.skip_trainer:
        for k in range(args.repeat):
            row = dict(bench="arcade_selfplay_process", B=4096, history=args.history, repeat=k)
            for name in ("bench_duel", "bench_selfplay"):
                row[name[6:] + "_ms"] = round(arcade_trainer_ms(name, 4096, args.history, args.steps, args.warmup)[1], 2)
            print(json.dumps(row), flush=True)


def bench_versus(args):
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.arcade_environment import BatchedArcadeEnvironment
    Environment.register_arcade_selfplay("bench_selfplay")
    Environment.register_arcade_config("bench_duel", game="duel")
    plain, fused = "unreal_arcade%s_rollout_step", "unreal_arcade%s_policy_rollout_step"
    for B in (4096, 64):
        conf = Environment.ARCADE_CONFIG["bench_selfplay"]
        envs = (("duel", "", BatchedArcadeEnvironment(B, 3, DEV, config=Environment.ARCADE_CONFIG["bench_duel"])),
                ("selfplay", "_selfplay", BatchedArcadeEnvironment(B, 3, DEV, config=conf)),
                ("versus", "_versus", BatchedArcadeEnvironment(B, 3, DEV, config=conf, versus=True)))
        envs[2][2].opponent.actions.copy_(torch.from_numpy(np.random.RandomState(1).randint(0, 4, B).astype(np.int32)))
        row = dict(bench="arcade_versus_step", B=B)
        for k in range(args.repeat):
            for key, family, env in envs:
                row["%s_us_%d" % (key, k)] = round(1e3 * rollout_ms(env, B, args.launches, plain % family), 2)
                row["%s_fused_us_%d" % (key, k)] = round(1e3 * fused_ms(env, B, args.launches, fused % family), 2)
        mean = lambda key: sum(row["%s_us_%d" % (key, k)] for k in range(args.repeat)) / args.repeat
        row["versus_over_selfplay"] = round(mean("versus") / mean("selfplay"), 3)                  # per launch of B workgroups
        row["versus_ns_per_game"] = round(1e3 * mean("versus") / B, 2)
        row["selfplay_ns_per_game"] = round(1e3 * mean("selfplay") / (B // 2), 2)
        print(json.dumps(row), flush=True)
        del envs
        torch.cuda.empty_cache()
    if not args.skip_trainer:
        for k in range(args.repeat):
            row = dict(bench="arcade_versus_process", B=4096, history=args.history, repeat=k)
            for K in (0, 1, 4):
                row["pool%d_ms" % K] = round(arcade_trainer_ms("bench_selfplay", 4096, args.history, args.steps, args.warmup,
                                                               opponent_pool=K)[1], 2)
            row["ms_per_slot"] = round((row["pool4_ms"] - row["pool1_ms"]) / 3.0, 2)
            print(json.dumps(row), flush=True)


def arcade_trainer_ms(env_name, B, history, steps, warmup, **options):
    import time
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.options import get_options
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer, log_uniform
    flags = get_options("training", preset="lab", argv=[])
    net = UnrealModel(4, 0, -1, flags.use_lstm, flags.use_pixel_change, flags.use_value_replay,
                      flags.use_reward_prediction, flags.pixel_change_lambda, flags.entropy_beta, DEV, seed=1)
    lr0 = log_uniform(flags.initial_alpha_low, flags.initial_alpha_high, flags.initial_alpha_log_rate)
    applier = RMSPropApplier(None, decay=flags.rmsp_alpha, momentum=0.0, epsilon=flags.rmsp_epsilon,
                             clip_norm=flags.grad_norm_clip, device=DEV)
    tr = Trainer(0, net, lr0, None, applier, "arcade", env_name, flags.use_lstm, flags.use_pixel_change,
                 flags.use_value_replay, flags.use_reward_prediction, flags.pixel_change_lambda, flags.entropy_beta,
                 flags.local_t_max, flags.n_step_TD, flags.gamma, flags.gamma_pc, history, flags.max_time_step, DEV,
                 batch_size=B, seed=0xA3C, **options)
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
    out = e0.elapsed_time(e1) / steps, (time.perf_counter() - t0) * 1e3 / steps
    del tr, net, applier
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--history", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--skip-trainer", action="store_true")
    ap.add_argument("--game", default="breakout", help="breakout, duel, invaders, crossing, or several of them joined by commas")
    ap.add_argument("--action-repeat", type=int, default=None, help="game ticks per agent step, 1..8 (DESIGN §7m)")
    ap.add_argument("--mix", default="", help="a game mixture (DESIGN §7u): a comma list of breakout, duel, invaders, crossing")
    ap.add_argument("--selfplay", action="store_true", help="the self-play duel beside the duel (DESIGN §7v)")
    ap.add_argument("--versus", action="store_true", help="the versus step beside self-play and the duel (DESIGN §7w)")
    args = ap.parse_args()
    if args.versus:
        return bench_versus(args)
    if args.selfplay:
        return bench_selfplay(args)
    if args.mix:
        return bench_mix(args)
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.arcade_environment import BatchedArcadeEnvironment
    from unreal_amd.environment.maze_environment import batched_maze_environment
    repeat = args.action_repeat
    games = args.game.split(",")
    if len(games) > 1:
        for g in games:
            Environment.register_arcade_config("bench_" + g, game=g, action_repeat=1 if repeat is None else repeat,
                                               **own_settings(g))
        for rep in range(args.repeat):
            for B in (512, 4096):
                envs = {g: BatchedArcadeEnvironment(B, 3, DEV, config=Environment.ARCADE_CONFIG["bench_" + g]) for g in games}
                row = dict(bench="arcade_games", B=B, repeat=rep, **({} if repeat is None else {"action_repeat": repeat}))
                for k in range(2):                              # the games in turn, twice
                    for g in games:
                        row["%s_us_%d" % (g, k)] = round(1e3 * kernel_ms(envs[g], B, args.launches, entry="unreal_arcade_step"), 2)
                        row["%s_fused_us_%d" % (g, k)] = round(1e3 * fused_ms(envs[g], B, args.launches), 2)
                print(json.dumps(row), flush=True)
                del envs
                torch.cuda.empty_cache()
        return
    arcade = "bench_" + args.game
    Environment.register_arcade_config(arcade, game=args.game, action_repeat=1 if repeat is None else repeat,
                                       **own_settings(args.game))
    tag = {} if args.game == "breakout" else {"game": args.game}
    if repeat is not None:
        tag["action_repeat"] = repeat
    kw = dict(random_start=True, random_goal=True, max_episode_steps=200)
    Environment.register_maze_config("bench_fp7", layouts(7), view="first_person", **kw)
    Environment.register_maze_config("bench_td7", layouts(7), **kw)
    for rep in range(args.repeat):
        for B in (512, 4096):
            envs = dict(arcade=BatchedArcadeEnvironment(B, 3, DEV, config=Environment.ARCADE_CONFIG[arcade]),
                        first_person=batched_maze_environment(B, 3, DEV, config=Environment.MAZE_CONFIG["bench_fp7"]),
                        top_down=batched_maze_environment(B, 3, DEV, config=Environment.MAZE_CONFIG["bench_td7"]))
            row = dict(bench="arcade_step", B=B, repeat=rep, **tag)
            for k in range(2):                                  # the kernels in turn, twice
                row["arcade_us_%d" % k] = round(1e3 * kernel_ms(envs["arcade"], B, args.launches, entry="unreal_arcade_step"), 2)
                row["arcade_fused_us_%d" % k] = round(1e3 * fused_ms(envs["arcade"], B, args.launches), 2)
                row["first_person_us_%d" % k] = round(1e3 * kernel_ms(envs["first_person"], B, args.launches), 2)
                row["top_down_us_%d" % k] = round(1e3 * kernel_ms(envs["top_down"], B, args.launches), 2)
            if repeat is not None:
                for key in [n for n in row if n.startswith("arcade_")]:
                    row[key.replace("_us_", "_tick_us_")] = round(row[key] / repeat, 2)
            print(json.dumps(row), flush=True)
            del envs
            torch.cuda.empty_cache()
    if not args.skip_trainer:
        for rep in range(args.repeat):
            for name, fn in ((arcade, arcade_trainer_ms), ("bench_fp7", maze_trainer_ms)):
                dev_ms, wall_ms = fn(name, 4096, args.history, args.steps, args.warmup)
                print(json.dumps(dict(bench="trainer_process", env=name, B=4096, history=args.history, repeat=rep,
                                      device_ms=round(dev_ms, 2), wall_ms=round(wall_ms, 2),
                                      env_steps_per_s=round(4096 * 20 / wall_ms * 1e3),
                                      **({"action_repeat": repeat} if repeat is not None and name == arcade else {}))),
                      flush=True)


if __name__ == "__main__":
    main()
