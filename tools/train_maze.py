#!/usr/bin/env python3
"""Train the maze agent with the batched Trainer and log episode returns (GPU box).

usage: python tools/train_maze.py [--actors 4096] [--groups 1] [--history 2000] [--steps 2e7] [--log-every 10]
                                  [--lr-scale 1.0] [--max-time-step 0] [--out curve.jsonl] [--arcade breakout|duel|invaders|crossing]
                                  [--arcade-mix breakout,duel,invaders,crossing] [--arcade-selfplay] [--knock-back K]
                                  [--opponent-pool K] [--snapshot-every N]
                                  [--opponent-speed N] [--action-repeat K] [--return-reward R] [--seed S]
                                  [--max-episode-steps N] [--bootstrap-timeouts] [--gae-lambda L]
                                  [--gen-maze N] [--depth-prediction] [--depth-lambda X]
                                  [--reuse-epochs E] [--ppo-clip X] [--reuse-minibatches M]
                                  [--explore-beta X] [--explore-cell C] [--explore-levels K] [--explore-bits N]
                                  [--optimizer rmsprop|adam] [--adam-beta1 X] [--adam-beta2 X] [--adam-epsilon X]
                                  [--weight-decay X] [--normalize-advantages]
`--groups G`: G sequential updates per process() call (update density x G, see Trainer).  One JSON line per
`--log-every` calls: global_t, episodes finished since the last line, their mean return, losses, entropy, steps/s.
`--arcade GAME`: train on the device arcade with that game's default config instead; a line then also holds
bricks_per_episode and lives_lost_per_episode (differences of the records' totals over the episodes of the line); on the
duel these are points_won_per_episode, points_lost_per_episode and matches_won_per_episode, and
`--opponent-speed` overrides the opponent's 2 px per step; on invaders aliens_per_episode, lives_lost_per_episode
and waves_cleared_per_episode; on crossing (the tool's config: a walker 4 px wide, timed episodes of 2000 steps
unless --max-episode-steps says otherwise) crossings_per_episode, hits_per_episode and targets_reached_per_episode, and
`--knock-back K` (1..70) is how far a hit throws the walker back: 8 is Freeway-like, 70 Frogger-like (back to the start).
`--action-repeat K` (1..8) and `--return-reward R` (0..100) are
the arcade config's settings of those names: K game ticks per agent step, R paid for every ball the agent's
paddle returns; steps, steps_per_s and episode lengths stay agent steps.  `--seed S` (arcade only) replaces the run's two
seeds, the network's initial weights (1) and the trainer's draws and serve key (0xA3C), by S.
`--max-episode-steps N` (arcade only) is the config's step limit.  `--bootstrap-timeouts` (arcade only) and `--gae-lambda L`
are the Trainer's rollout options of DESIGN §7o.
`--gen-maze N` trains on a generated first-person navigation maze of size N (a new layout per episode, 4 apples,
300-step episodes) instead of the reference's map; `--depth-prediction [--depth-lambda X]` (needs --gen-maze) adds the
depth-prediction head of DESIGN §7p, and a line then also holds depth_loss, depth_accuracy and depth_majority_rate (the
share of the most common class among the replay's labels: what a constant prediction would score).
`--reuse-epochs E [--ppo-clip X]` are the Trainer's sample-reuse options of DESIGN §7q (every environment of this tool): E
updates per rollout; a line then also holds clip_fraction and approx_kl, and its steps stay environment steps.
`--reuse-minibatches M` is the Trainer's option of DESIGN §7t: every rollout is consumed as E x M clipped-surrogate updates,
each on one block of actors / groups / M actors; a line then also holds updates, the optimiser steps of its last call.
`--explore-beta X [--explore-cell C] [--explore-levels K] [--explore-bits N]` are the Trainer's exploration-bonus options
of DESIGN §7r (`--arcade` and `--gen-maze`): a line then also holds explore_bonus and explore_first of its last call.  A
`--gen-maze` line always holds goals_per_episode and apples_per_episode (the actor records' totals over the line's episodes).
`--optimizer adam [--adam-beta1 X] [--adam-beta2 X] [--adam-epsilon X] [--weight-decay X]` steps with AdamApplier instead of
RMSPropApplier and `--normalize-advantages` is the Trainer's option of that name (every environment of this
tool); a line then also holds adv_mean and adv_std of its last call, and the head line the optimizer.
`--arcade-mix LIST` trains one agent on a game mixture: LIST is a comma list of breakout, duel, invaders and crossing with
their default configs, repeats allowed (a game listed twice gets twice the actors); actor g plays entry g mod len(LIST).  The
arcade's options apply to every entry (--return-reward not to invaders and crossing, which have no such event); a line then also holds
`tasks`, Trainer.task_scores() over the line's episodes: per entry its name, game, finished episodes and mean return.
`--arcade-selfplay` trains on the self-play duel with its default config (the arcade's options apply; --actors
and --actors / --groups must be even): actors 2 i and 2 i + 1 play game i against each other.  Before the first update and at
every logged line it runs Evaluate(net, arcade=name) on 64 actors, one episode each: seat 0 against the scripted opponent,
the transfer metric of the run; the line then also holds `scripted`, that evaluation's success_rate, losses, timeouts,
mean_return, mean_length and points_won_per_episode, and `versus_initial`, Evaluate(net, arcade=name, versus=<a copy of
the initial weights the tool keeps>) over 32 games head to head: the usual progress measure of a self-play run.
`--opponent-pool K [--snapshot-every N]` (with --arcade-selfplay) seats K frozen copies of the agent at the
other paddle, Trainer(opponent_pool=K, opponent_snapshot_every=N): every actor is a learner (odd counts are fine) and a line
then also holds `opponents`, Trainer.opponent_scores() over the line's matches with every slot's age in updates."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import build_trainer  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--actors", type=int, default=4096)
ap.add_argument("--groups", type=int, default=1)
ap.add_argument("--history", type=int, default=2000)
ap.add_argument("--steps", type=float, default=2e7)
ap.add_argument("--log-every", type=int, default=10)
ap.add_argument("--lr-scale", type=float, default=1.0)
ap.add_argument("--max-time-step", type=float, default=0)
ap.add_argument("--entropy-beta", type=float, default=None, help="override options_lab's 0.001 (a stated deviation)")
ap.add_argument("--out", default="")
ap.add_argument("--arcade", default="", help="a device arcade game (breakout, duel, invaders, crossing) instead of the maze")
ap.add_argument("--arcade-mix", default="", help="a game mixture: a comma list of breakout, duel, invaders, crossing (DESIGN 7u)")
ap.add_argument("--knock-back", type=int, default=None, help="crossing: px a hit throws the walker back, 1..70 (default 8)")
ap.add_argument("--arcade-selfplay", action="store_true", help="the self-play duel (DESIGN 7v)")
ap.add_argument("--opponent-pool", type=int, default=0, help="with --arcade-selfplay: K frozen copies of the agent play the other paddle (DESIGN 7w)")
ap.add_argument("--snapshot-every", type=int, default=100, help="optimiser updates between two snapshots into the pool")
ap.add_argument("--opponent-speed", type=int, default=None, help="the duel's opponent_speed (default: the game's)")
ap.add_argument("--action-repeat", type=int, default=1, help="arcade: game ticks per agent step, 1..8")
ap.add_argument("--return-reward", type=int, default=0, help="arcade: reward for a ball the agent's paddle returns, 0..100")
ap.add_argument("--seed", type=int, default=None, help="arcade: seed of the weights and of the trainer (default: 1 and 0xA3C)")
ap.add_argument("--max-episode-steps", type=int, default=None, help="arcade: the step limit (default: the game's 5000)")
ap.add_argument("--bootstrap-timeouts", action="store_true",
                help="arcade: an episode cut off at the step limit bootstraps from V(final observation) (DESIGN 7o)")
ap.add_argument("--gae-lambda", type=float, default=None, help="GAE(lambda) instead of the n-step return, 0..1 (DESIGN 7o)")
ap.add_argument("--gen-maze", type=int, default=0, help="a generated first-person maze of this size (7, 12, 14, 21)")
ap.add_argument("--depth-prediction", action="store_true", help="the depth-prediction head (DESIGN 7p); needs --gen-maze")
ap.add_argument("--depth-lambda", type=float, default=1.0, help="weight of the depth loss")
ap.add_argument("--reuse-epochs", type=int, default=1, help="updates per rollout, 1..16 (DESIGN 7q)")
ap.add_argument("--ppo-clip", type=float, default=0.2, help="the clip range of the reuse updates' surrogate (DESIGN 7q)")
ap.add_argument("--reuse-minibatches", type=int, default=1, help="updates per reuse epoch, each on 1/M of a group's actors (DESIGN 7t)")
ap.add_argument("--explore-beta", type=float, default=0.0, help="exploration bonus beta / sqrt(count) (DESIGN 7r); 0: off")
ap.add_argument("--explore-cell", type=int, default=7, help="pooling cell of the frame code: 4, 6, 7, 12, 14 or 21")
ap.add_argument("--explore-levels", type=int, default=8, help="quantisation levels of the frame code, 2..64")
ap.add_argument("--explore-bits", type=int, default=22, help="the count table has 2^bits entries, 10..26")
ap.add_argument("--optimizer", choices=("rmsprop", "adam"), default="rmsprop", help="the grad_applier (DESIGN 7s)")
ap.add_argument("--adam-beta1", type=float, default=0.9)
ap.add_argument("--adam-beta2", type=float, default=0.999)
ap.add_argument("--adam-epsilon", type=float, default=1e-8)
ap.add_argument("--weight-decay", type=float, default=0.0, help="AdamW's decoupled decay; 0: Adam")
ap.add_argument("--normalize-advantages", action="store_true",
                help="the policy loss reads per-rollout normalised advantages (DESIGN 7s)")
args = ap.parse_args()
MIX_GAMES = ("breakout", "duel", "invaders", "crossing")
mix = [g for g in args.arcade_mix.split(",")] if args.arcade_mix else []
if mix and (args.arcade or args.gen_maze):
    ap.error("--arcade-mix, --arcade and --gen-maze are three environments")
if mix and (not 1 <= len(mix) <= 16 or any(g not in MIX_GAMES for g in mix)):
    ap.error("--arcade-mix takes a comma list of 1..16 games out of %s, not %r" % (", ".join(MIX_GAMES), args.arcade_mix))
if mix:
    args.arcade = "mix:" + ",".join(mix)                  # the mixture's name; everything arcade below applies to it
if args.arcade_selfplay:
    if args.arcade or args.gen_maze:
        ap.error("--arcade-selfplay, --arcade-mix, --arcade and --gen-maze are four environments")
    if not args.opponent_pool and (args.actors % 2 or args.groups < 1 or args.actors % args.groups or
                                   (args.actors // args.groups) % 2):
        ap.error("--arcade-selfplay: actors come in pairs, --actors and --actors / --groups must be even")
    args.arcade = "selfplay"                              # the registered name; everything arcade below applies to it
if args.knock_back is not None and args.arcade != "crossing" and "crossing" not in mix:
    ap.error("--knock-back is a setting of --arcade crossing (or of a mixture that lists it)")
if args.opponent_pool and not args.arcade_selfplay:
    ap.error("--opponent-pool needs --arcade-selfplay")
if args.depth_prediction and not args.gen_maze:
    ap.error("--depth-prediction needs a first-person maze: --gen-maze N")
if args.gen_maze and args.arcade:
    ap.error("--gen-maze and --arcade are two environments")
if args.explore_beta > 0 and not (args.gen_maze or args.arcade):
    ap.error("--explore-beta needs --gen-maze N or --arcade GAME")
explore = dict(explore_beta=args.explore_beta, explore_cell=args.explore_cell, explore_levels=args.explore_levels,
               explore_bits=args.explore_bits)
if not args.arcade and (args.action_repeat != 1 or args.return_reward != 0 or args.seed is not None or
                        args.opponent_speed is not None or args.max_episode_steps is not None or
                        args.bootstrap_timeouts):
    ap.error("--action-repeat, --return-reward, --seed, --opponent-speed, --max-episode-steps and --bootstrap-timeouts "
             "are settings of --arcade GAME")
device = torch.device("cuda", 0)


def build_applier(args, flags, device):
    """The grad_applier --optimizer names, with the flags' clip norm."""
    if args.optimizer == "adam":
        from unreal_amd.train.adam_applier import AdamApplier
        return AdamApplier(None, beta1=args.adam_beta1, beta2=args.adam_beta2, epsilon=args.adam_epsilon,
                           weight_decay=args.weight_decay, clip_norm=flags.grad_norm_clip, device=device)
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    return RMSPropApplier(None, decay=flags.rmsp_alpha, momentum=0.0, epsilon=flags.rmsp_epsilon,
                          clip_norm=flags.grad_norm_clip, device=device)


def build_arcade_trainer(args, device):
    """bench.build_trainer for env_type 'arcade' (one rank)."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.options import get_options
    from unreal_amd.train.trainer import Trainer, log_uniform
    limit = {} if args.max_episode_steps is None else dict(max_episode_steps=args.max_episode_steps)
    if args.arcade_selfplay:
        Environment.register_arcade_selfplay(args.arcade, opponent_speed=args.opponent_speed,
                                             action_repeat=args.action_repeat, return_reward=args.return_reward, **limit)
    for game in [] if args.arcade_selfplay else sorted(set(mix)) or [args.arcade]:
        # the tool's crossing: a walker 4 px wide, a purely timed episode of 2000 steps (DESIGN §7x's baselines)
        own = dict(dict(paddle_width=4, max_episode_steps=2000, knock_back=args.knock_back), **limit) \
            if game == "crossing" else limit
        Environment.register_arcade_config(game, game=game, opponent_speed=args.opponent_speed if game == "duel" or not mix
                                           else None, action_repeat=args.action_repeat,
                                           return_reward=0 if mix and game in ("invaders", "crossing") else args.return_reward,
                                           **own)
    if mix:
        Environment.register_arcade_mix(args.arcade, mix)
    flags = get_options("training", preset="lab", argv=["--env_type", "arcade", "--env_name", args.arcade])
    net = UnrealModel(Environment.get_action_size("arcade", args.arcade), 0, -1, flags.use_lstm, flags.use_pixel_change,
                      flags.use_value_replay, flags.use_reward_prediction, flags.pixel_change_lambda, flags.entropy_beta,
                      device, seed=1 if args.seed is None else args.seed)
    lr0 = log_uniform(flags.initial_alpha_low, flags.initial_alpha_high, flags.initial_alpha_log_rate)
    applier = build_applier(args, flags, device)
    tr = Trainer(0, net, lr0, None, applier, "arcade", args.arcade, flags.use_lstm, flags.use_pixel_change,
                 flags.use_value_replay, flags.use_reward_prediction, flags.pixel_change_lambda, flags.entropy_beta,
                 flags.local_t_max, flags.n_step_TD, flags.gamma, flags.gamma_pc, args.history, flags.max_time_step, device,
                 batch_size=args.actors, seed=0xA3C if args.seed is None else args.seed, groups=args.groups,
                 bootstrap_timeouts=args.bootstrap_timeouts, gae_lambda=args.gae_lambda, reuse_epochs=args.reuse_epochs,
                 ppo_clip=args.ppo_clip, normalize_advantages=args.normalize_advantages,
                 reuse_minibatches=args.reuse_minibatches, opponent_pool=args.opponent_pool,
                 opponent_snapshot_every=args.snapshot_every, **explore)
    tr.prepare()
    return flags, net, tr


def build_gen_maze_trainer(args, device):
    """bench.build_trainer for a generated first-person navigation maze (one rank), with or without the depth head."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.options import get_options
    from unreal_amd.train.trainer import Trainer, log_uniform
    name = "gen_maze_%d" % args.gen_maze
    Environment.register_maze_config(name, view="first_person", generate=args.gen_maze, random_start=True,
                                     random_goal=True, max_episode_steps=300, gen_loops=2, gen_apples=4, goal_reward=10)
    flags = get_options("training", preset="lab", argv=["--env_type", "maze", "--env_name", name, "--use_depth_prediction",
                                                        str(args.depth_prediction), "--depth_lambda", str(args.depth_lambda)])
    net = UnrealModel(Environment.get_action_size("maze", name), 0, -1, flags.use_lstm, flags.use_pixel_change,
                      flags.use_value_replay, flags.use_reward_prediction, flags.pixel_change_lambda, flags.entropy_beta,
                      device, seed=1, use_depth_prediction=flags.use_depth_prediction)
    lr0 = log_uniform(flags.initial_alpha_low, flags.initial_alpha_high, flags.initial_alpha_log_rate)
    applier = build_applier(args, flags, device)
    tr = Trainer(0, net, lr0, None, applier, "maze", name, flags.use_lstm, flags.use_pixel_change,
                 flags.use_value_replay, flags.use_reward_prediction, flags.pixel_change_lambda, flags.entropy_beta,
                 flags.local_t_max, flags.n_step_TD, flags.gamma, flags.gamma_pc, args.history, flags.max_time_step, device,
                 batch_size=args.actors, seed=0xA3C, groups=args.groups, gae_lambda=args.gae_lambda,
                 use_depth_prediction=flags.use_depth_prediction, depth_lambda=flags.depth_lambda,
                 reuse_epochs=args.reuse_epochs, ppo_clip=args.ppo_clip, normalize_advantages=args.normalize_advantages,
                 reuse_minibatches=args.reuse_minibatches, **explore)
    tr.prepare()
    return flags, net, tr


def build_reuse_trainer(args, device):
    """bench.build_trainer (one rank, the reference's maze) with the sample-reuse, optimizer and normalisation options."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.options import get_options
    from unreal_amd.train.trainer import Trainer, log_uniform
    flags = get_options("training", preset="lab", argv=["--env_type", "maze", "--env_name", ""])
    Environment.action_size = -1
    net = UnrealModel(Environment.get_action_size("maze", ""), 0, -1, flags.use_lstm, flags.use_pixel_change,
                      flags.use_value_replay, flags.use_reward_prediction, flags.pixel_change_lambda, flags.entropy_beta,
                      device, seed=1)
    lr0 = log_uniform(flags.initial_alpha_low, flags.initial_alpha_high, flags.initial_alpha_log_rate)
    applier = build_applier(args, flags, device)
    tr = Trainer(0, net, lr0, None, applier, "maze", "", flags.use_lstm, flags.use_pixel_change, flags.use_value_replay,
                 flags.use_reward_prediction, flags.pixel_change_lambda, flags.entropy_beta, flags.local_t_max,
                 flags.n_step_TD, flags.gamma, flags.gamma_pc, args.history, flags.max_time_step, device,
                 batch_size=args.actors, seed=0xA3C, groups=args.groups, reuse_epochs=args.reuse_epochs,
                 ppo_clip=args.ppo_clip, normalize_advantages=args.normalize_advantages,
                 reuse_minibatches=args.reuse_minibatches)
    tr.prepare()
    return flags, net, tr


if args.arcade:
    flags, net, tr = build_arcade_trainer(args, device)
elif args.gen_maze:
    flags, net, tr = build_gen_maze_trainer(args, device)
elif args.reuse_epochs > 1 or args.reuse_minibatches > 1 or args.optimizer != "rmsprop" or args.normalize_advantages:
    flags, net, tr = build_reuse_trainer(args, device)
else:
    flags, net, tr = build_trainer(args, 0, 1, device)
if not args.arcade and not args.gen_maze:                        # (the reference's maze: the returns kernel is chosen per rollout, nothing is allocated)
    tr.gae_lambda = tr.check_rollout_options(flags.env_type, flags.env_name, False, args.gae_lambda)[1]
tr.initial_learning_rate *= args.lr_scale
if args.entropy_beta is not None:
    tr.entropy_beta = args.entropy_beta
if args.max_time_step:
    tr.max_global_time_step = int(args.max_time_step)
updates_total = tr.max_global_time_step / float(tr.Bg * flags.n_step_TD)
if updates_total < 5000:
    print("# WARNING: %.0f optimiser steps in the whole learning-rate schedule (max_time_step %d / (%d actors per update x "
          "%d steps)); the reference makes ~%d.  Use --groups to raise the update density." % (
              updates_total, tr.max_global_time_step, tr.Bg, flags.n_step_TD, tr.max_global_time_step // flags.n_step_TD),
          file=sys.stderr)
t_fill = time.time()
while not tr._full:
    tr.process(None, 0)
torch.cuda.synchronize()
t_fill = time.time() - t_fill
out = open(args.out, "w") if args.out else None
head = {"actors": args.actors, "groups": args.groups, "reuse_epochs": tr.reuse_epochs, "reuse_minibatches": tr.reuse_minibatches, "ppo_clip": tr.ppo_clip, "optimizer": tr.grad_applier.kind, "normalize_advantages": tr.normalize_advantages, "explore_beta": tr.explore_beta, "entropy_beta": tr.entropy_beta, "history": args.history, "lr0": tr.initial_learning_rate,
        "max_time_step": tr.max_global_time_step, "replay_fill_s": round(t_fill, 1)}
print(json.dumps(head), flush=True)
if out:
    out.write(json.dumps(head) + "\n")
scripted = None
if args.arcade_selfplay:
    from unreal_amd.evaluate import Evaluate
    from unreal_amd.model.model import UnrealModel
    scripted_eval = Evaluate(net, batch_size=64, device=device, arcade=args.arcade)
    # a copy of the initial weights, kept for the whole run: the head-to-head opponent of every logged line
    initial = UnrealModel(4, 0, -1, flags.use_lstm, flags.use_pixel_change, flags.use_value_replay,
                          flags.use_reward_prediction, flags.pixel_change_lambda, flags.entropy_beta, device)
    initial.sync_from(net)
    versus_eval = Evaluate(net, batch_size=64, device=device, arcade=args.arcade, versus=initial)


    def scripted():
        """Seat 0 against the scripted opponent, one episode of each of 64 actors."""
        res = scripted_eval.process(0, one_episode_per_actor=True)
        return {key: round(res[key], 4) for key in ("success_rate", "losses", "timeouts", "mean_return", "mean_length",
                                                    "points_won_per_episode")}


    def versus_initial():
        """Head to head against the initial weights, one match of each of 32 games."""
        res = versus_eval.process(0, one_episode_per_actor=True)
        return {key: round(res[key], 4) for key in ("success_rate", "losses", "timeouts", "points_won_per_episode",
                                                    "points_lost_per_episode")}
    line = json.dumps({"global_t": 0, "scripted": scripted(), "versus_initial": versus_initial()})
    print(line, flush=True)
    if out:
        out.write(line + "\n")
global_t, t0, k = 0, time.time(), 0
# the totals of the game's records (words 10 ..), never zeroed: per-line differences over the line's episodes
TOTALS = {"breakout": ("bricks_per_episode", "lives_lost_per_episode"),
          "duel": ("points_won_per_episode", "points_lost_per_episode", "matches_won_per_episode"),
          "invaders": ("aliens_per_episode", "lives_lost_per_episode", "waves_cleared_per_episode"),
          "crossing": ("crossings_per_episode", "hits_per_episode", "targets_reached_per_episode")}.get(args.arcade, ())
totals = tr.full_ring.actor_records[:, 10:10 + len(TOTALS)].sum(0).cpu() if args.arcade else None
nav_totals = tr.full_ring.actor_records[:, 3:5].sum(0).cpu() if args.gen_maze else None      # goals_total, apples_total
while global_t < args.steps:
    tr.process(None, global_t + k % args.log_every * args.actors * flags.n_step_TD, sync_stats=False)
    k += 1
    if k % args.log_every == 0:
        steps, episodes, score_sum = tr.read_stats()
        global_t += steps
        l = tr._publish_losses()
        rw = tr.rewards[:tr.Bg * flags.n_step_TD]          # the last group's rollout: what the policy currently does
        live = tr.active_log[:tr.Bg * flags.n_step_TD].float()
        n_live = float(live.sum().clamp(min=1))
        bump = float(((rw < 0).float() * live).sum()) / n_live
        goal = float(((rw > 0).float() * live).sum()) / n_live
        extra = {}
        if args.arcade:
            now = tr.full_ring.actor_records[:, 10:10 + len(TOTALS)].sum(0).cpu()
            d = (now - totals).tolist()
            totals = now
            extra = {key: round(v / episodes, 3) if episodes else None for key, v in zip(TOTALS, d)}
        if mix:
            extra.update(tasks=[dict(t, mean_return=None if t["mean_return"] is None else round(t["mean_return"], 4))
                                for t in tr.task_scores()])
        if scripted is not None:
            extra.update(scripted=scripted(), versus_initial=versus_initial())
        if args.opponent_pool:
            extra.update(opponents=[dict(o, age=a) for o, a in zip(tr.opponent_scores(), tr.opponent_ages())])
        if args.depth_prediction:
            # the yardstick of depth_accuracy: the share of the most common class among the labels the replay holds
            hist = torch.bincount(tr.full_ring.r_depth.long(), minlength=8).float()
            extra.update(depth_loss=round(l["depth_loss"], 4), depth_accuracy=round(l["depth_accuracy"], 4),
                         depth_majority_rate=round(float(hist.max() / hist.sum()), 4))
        if args.gen_maze:
            now = tr.full_ring.actor_records[:, 3:5].sum(0).cpu()
            d = (now - nav_totals).tolist()
            nav_totals = now
            extra.update(goals_per_episode=round(d[0] / episodes, 4) if episodes else None,
                         apples_per_episode=round(d[1] / episodes, 4) if episodes else None)
        if tr.explore_beta > 0:
            extra.update(explore_bonus=round(l["explore_bonus"], 6), explore_first=round(l["explore_first"], 6))
        if tr.reuse_epochs > 1 or tr.reuse_minibatches > 1:
            extra.update(clip_fraction=round(l["clip_fraction"], 4), approx_kl=round(l["approx_kl"], 6))
        if tr.reuse_minibatches > 1:
            extra.update(updates=l["updates"])
        if tr.normalize_advantages:
            extra.update(adv_mean=round(l["adv_mean"], 6), adv_std=round(l["adv_std"], 6))
        line = json.dumps({"global_t": global_t, "episodes": episodes, "bump_rate": round(bump, 5), "goal_rate": round(goal, 6),
                           "mean_return": (score_sum / episodes) if episodes else None,
                           "total_loss": round(l["total_loss"], 4), "entropy": round(l["entropy"], 4),
                           "grad_norm": round(l["grad_norm"], 3), "steps_per_s": round(global_t / (time.time() - t0)), **extra})
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
