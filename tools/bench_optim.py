#!/usr/bin/env python3
"""The cost of the Adam applier and of advantage normalisation, in one process: wall time of
Trainer.process(), full UNREAL (LSTM + pixel control + value replay + reward prediction) on the reference maze, at
(B = 4096, G = 1) and (B = 512, G = 64), with the optimizer RMSProp / Adam and the normalisation off / on.  The four trainers
of a configuration are built once, their replays filled, and then timed in turn: --repeat runs of --calls process() calls
each (default 3 x 10), a device synchronisation before and after every run.  Per row: ms per call, ms per update (a call
makes G updates), the difference to the (rmsprop, off) trainer of the same repeat, and for the rows with the normalisation
on its cost per update = (ms(on) - ms(off)) / G under the same optimizer.

  python tools/bench_optim.py [--calls 10] [--repeat 3] [--history 100] [--config 4096x1,512x64] [--reverse]

`--reverse` builds and times the four trainers in the opposite order (normalisation on first): a difference that follows the
order and not the option belongs to where a trainer's buffers landed, not to what it launches.

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
VARIANTS = [("rmsprop", False), ("adam", False), ("rmsprop", True), ("adam", True)]


def build(actors, groups, history, optimizer, normalize):
    """bench.build_trainer's trainer (one rank) with the applier and the normalisation asked for, its replay filled."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.options import get_options
    from unreal_amd.train.adam_applier import AdamApplier
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer, log_uniform
    flags = get_options("training", preset="lab", argv=["--env_type", "maze", "--env_name", ""])
    Environment.action_size = -1
    A = Environment.get_action_size("maze", "")
    net = UnrealModel(A, 0, -1, flags.use_lstm, flags.use_pixel_change, flags.use_value_replay,
                      flags.use_reward_prediction, flags.pixel_change_lambda, flags.entropy_beta, DEV, seed=1)
    lr0 = log_uniform(flags.initial_alpha_low, flags.initial_alpha_high, flags.initial_alpha_log_rate)
    if optimizer == "adam":
        applier = AdamApplier(None, beta1=flags.adam_beta1, beta2=flags.adam_beta2, epsilon=flags.adam_epsilon,
                              weight_decay=flags.weight_decay, clip_norm=flags.grad_norm_clip, device=DEV)
    else:
        applier = RMSPropApplier(None, decay=flags.rmsp_alpha, momentum=0.0, epsilon=flags.rmsp_epsilon,
                                 clip_norm=flags.grad_norm_clip, device=DEV)
    tr = Trainer(0, net, lr0, None, applier, "maze", "", flags.use_lstm, flags.use_pixel_change, flags.use_value_replay,
                 flags.use_reward_prediction, flags.pixel_change_lambda, flags.entropy_beta, flags.local_t_max,
                 flags.n_step_TD, flags.gamma, flags.gamma_pc, history, flags.max_time_step, DEV, batch_size=actors,
                 seed=0xA3C, groups=groups, normalize_advantages=normalize)
    tr.prepare()
    while not tr._full:
        tr.process(None, 0)
    return tr


def run_ms(tr, calls, global_t):
    """Mean wall ms of `calls` process() calls (stats left on the device: the call's only host sync is ours)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(calls):
        tr.process(None, global_t, sync_stats=False)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0) / calls
    tr.read_stats()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--history", type=int, default=100)
    ap.add_argument("--config", default="4096x1,512x64", help="actors x groups, comma separated")
    ap.add_argument("--reverse", action="store_true", help="build and time the trainers in the opposite order")
    args = ap.parse_args()
    order = VARIANTS[::-1] if args.reverse else VARIANTS
    for conf in args.config.split(","):
        B, G = (int(x) for x in conf.split("x"))
        trainers = {v: build(B, G, args.history, *v) for v in order}
        for tr in trainers.values():                         # warm-up: lazy allocations, first-use paths
            run_ms(tr, 2, 0)
        for rep in range(args.repeat):
            ms = {}
            for v in order:                                  # the trainers in turn
                ms[v] = run_ms(trainers[v], args.calls, 0)
            for v in VARIANTS:
                optimizer, normalize = v
                row = dict(bench="optim", actors=B, groups=G, optimizer=optimizer, normalize_advantages=normalize,
                           repeat=rep, calls=args.calls, reverse=args.reverse, ms_per_call=round(ms[v], 3),
                           ms_per_update=round(ms[v] / G, 4),
                           ms_over_baseline=round(ms[v] - ms[VARIANTS[0]], 3))
                if normalize:
                    row["normalize_ms_per_update"] = round((ms[v] - ms[(optimizer, False)]) / G, 4)
                print(json.dumps(row), flush=True)
        del trainers
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
