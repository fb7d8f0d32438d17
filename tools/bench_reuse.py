#!/usr/bin/env python3
"""The cost of sample reuse, in one process: wall time of Trainer.process() with reuse_epochs E in {1, 2, 4},
full UNREAL (LSTM + pixel control + value replay + reward prediction) on the reference maze, at (B = 4096, G = 1) and
(B = 512, G = 64).  The trainers of a configuration are built once, their replays filled, and then timed in turn: --repeat
runs of --calls process() calls each (default 3 x 10), a device synchronisation before and after every run.  Per row:
ms per call, ms per update (a call makes G * E updates) and, for E > 1, the time of one reuse update = (ms(E) - ms(1)) /
(G * (E - 1)) next to that of a full update = ms(1) / G, both from the same repeat.

  python tools/bench_reuse.py [--calls 10] [--repeat 3] [--history 100] [--config 4096x1,512x64] [--epochs 1,2,4]
                              [--minibatches M]

`--minibatches M` adds, per configuration, a trainer with groups = 1, reuse_epochs = 1 and reuse_minibatches = M
on the same actors, timed in turn with the others: one call is ONE rollout of all the actors and M updates of actors / M
actors each.  Its row holds ms per call, ms per update = ms / M (the rollout's time included) and, when --epochs has an E >
1, the configuration's own reuse update of the same repeat beside it.  Every row holds env_steps_per_s, from the steps the
timed calls really took.

Prints one JSON line per measurement."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = torch.device("cuda", 0)


def build(actors, groups, history, reuse_epochs, ppo_clip=0.2, reuse_minibatches=1):
    """bench.build_trainer's trainer (one rank) with the reuse options, its replay filled."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.options import get_options
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer, log_uniform
    flags = get_options("training", preset="lab", argv=["--env_type", "maze", "--env_name", ""])
    Environment.action_size = -1
    A = Environment.get_action_size("maze", "")
    net = UnrealModel(A, 0, -1, flags.use_lstm, flags.use_pixel_change, flags.use_value_replay,
                      flags.use_reward_prediction, flags.pixel_change_lambda, flags.entropy_beta, DEV, seed=1)
    lr0 = log_uniform(flags.initial_alpha_low, flags.initial_alpha_high, flags.initial_alpha_log_rate)
    applier = RMSPropApplier(None, decay=flags.rmsp_alpha, momentum=0.0, epsilon=flags.rmsp_epsilon,
                             clip_norm=flags.grad_norm_clip, device=DEV)
    tr = Trainer(0, net, lr0, None, applier, "maze", "", flags.use_lstm, flags.use_pixel_change, flags.use_value_replay,
                 flags.use_reward_prediction, flags.pixel_change_lambda, flags.entropy_beta, flags.local_t_max,
                 flags.n_step_TD, flags.gamma, flags.gamma_pc, history, flags.max_time_step, DEV, batch_size=actors,
                 seed=0xA3C, groups=groups, reuse_epochs=reuse_epochs, ppo_clip=ppo_clip,
                 reuse_minibatches=reuse_minibatches)
    tr.prepare()
    while not tr._full:
        tr.process(None, 0)
    return tr


def run_ms(tr, calls, global_t):
    """(mean wall ms of `calls` process() calls, env-steps/s over them); the stats are left on the device: the call's only
    host sync is ours."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(calls):
        tr.process(None, global_t, sync_stats=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    steps = tr.read_stats()[0]
    return 1e3 * dt / calls, steps / dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--history", type=int, default=100)
    ap.add_argument("--config", default="4096x1,512x64", help="actors x groups, comma separated")
    ap.add_argument("--epochs", default="1,2,4")
    ap.add_argument("--minibatches", type=int, default=0, help="also time groups=1, reuse_minibatches=M on the same actors")
    args = ap.parse_args()
    epochs = [int(e) for e in args.epochs.split(",")]
    assert epochs[0] == 1, "the first entry is the baseline the reuse updates are measured against"
    for conf in args.config.split(","):
        B, G = (int(x) for x in conf.split("x"))
        M = args.minibatches
        trainers = {E: build(B, G, args.history, E) for E in epochs}
        if M > 1:
            trainers["mb"] = build(B, 1, args.history, 1, reuse_minibatches=M)
        for tr in trainers.values():                         # warm-up: lazy allocations, first-use paths
            run_ms(tr, 2, 0)
        for rep in range(args.repeat):
            ms, sps = {}, {}
            for key in trainers:                             # the trainers in turn
                ms[key], sps[key] = run_ms(trainers[key], args.calls, 0)
            reuse_ms = None
            for E in epochs:
                row = dict(bench="reuse", actors=B, groups=G, reuse_epochs=E, repeat=rep, calls=args.calls,
                           ms_per_call=round(ms[E], 3), ms_per_update=round(ms[E] / (G * E), 4),
                           full_update_ms=round(ms[1] / G, 4), env_steps_per_s=round(sps[E]))
                if E > 1:
                    row["reuse_update_ms"] = reuse_ms = round((ms[E] - ms[1]) / (G * (E - 1)), 4)
                    row["reuse_over_full"] = round(row["reuse_update_ms"] / row["full_update_ms"], 3)
                print(json.dumps(row), flush=True)
            if M > 1:
                row = dict(bench="reuse", actors=B, groups=1, reuse_epochs=1, reuse_minibatches=M, repeat=rep,
                           calls=args.calls, ms_per_call=round(ms["mb"], 3), ms_per_update=round(ms["mb"] / M, 4),
                           env_steps_per_s=round(sps["mb"]))
                if reuse_ms is not None:                     # the last E's reuse update at groups = G, same repeat
                    row["reuse_update_ms_groups_%d" % G] = reuse_ms
                print(json.dumps(row), flush=True)
        del trainers
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
