#!/usr/bin/env python3
"""The cost of the exploration bonus, in one process.

1. unreal_frame_codes alone: 81,920 rows (20 steps of 4096 actors) whose frames are drawn at random from the replay ring of
   a 4096-actor trainer (--history 100: 8.7 GB of frames, far beyond the 256 MiB Infinity Cache), ungated, timed with
   device events over --launches launches with fresh indices each.  Reported: us per launch and GB/s of frame bytes
   (rows x 21168 B / time) next to the 8 TB/s HBM peak of profiles/*_kernel_roofline.md.
2. Trainer.process() with the option off and on, full UNREAL on the reference maze, at (B = 4096, G = 1) and (B = 512,
   G = 64): both trainers built once, their replays filled, then timed in turn, --repeat runs of --calls calls each
   (default 3 x 10), a device synchronisation before and after every run, as tools/bench_reuse.py does.

  python tools/bench_explore.py [--calls 10] [--repeat 3] [--history 100] [--config 4096x1,512x64] [--beta 0.05]
                                [--cell 7] [--launches 20]

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
HBM_PEAK_TBS = 8.0


def build(actors, groups, history, beta, cell):
    """bench.build_trainer's trainer (one rank) with the exploration options, its replay filled."""
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
                 seed=0xA3C, groups=groups, explore_beta=beta, explore_cell=cell)
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


def codes_kernel(tr, rows, launches):
    """unreal_frame_codes on `rows` random frames of the trainer's whole ring, `launches` times."""
    from unreal_amd import ops
    ring = tr.full_ring
    H, W = ring.frame_shape
    n_frames = ring.B * ring.H1
    codes = torch.zeros(rows, dtype=torch.int32, device=DEV)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    idx = [torch.randint(0, n_frames, (rows,), dtype=torch.int32, device=DEV, generator=gen) for _ in range(launches + 2)]
    args = (ring.frames, ring.frame_stride, n_frames, H, W)
    tail = (tr.explore_cell, tr.explore_levels, tr.explore_vmax, tr.explore_bits, tr.explore_mult, codes)
    for k in range(2):                                       # warm-up: the code object, the clocks
        ops.frame_codes(rows, *args, idx[k], *tail)
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    torch.cuda.synchronize()
    for k, (e0, e1) in enumerate(events):
        e0.record()
        ops.frame_codes(rows, *args, idx[k + 2], *tail)
        e1.record()
    torch.cuda.synchronize()
    us = sorted(1e3 * e0.elapsed_time(e1) for e0, e1 in events)
    nbytes = rows * H * W * 3
    med = us[len(us) // 2]
    return dict(bench="explore_codes", rows=rows, ring_frames=n_frames, ring_gb=round(n_frames * ring.frame_stride / 1e9, 2),
                launches=launches, us_median=round(med, 1), us_min=round(us[0], 1), us_max=round(us[-1], 1),
                gb_per_s=round(nbytes / med / 1e3, 1), share_of_hbm_peak=round(nbytes / med / 1e6 / HBM_PEAK_TBS, 3),
                mb_per_launch=round(nbytes / 1e6, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--history", type=int, default=100)
    ap.add_argument("--config", default="4096x1,512x64", help="actors x groups, comma separated")
    ap.add_argument("--beta", type=float, default=0.05)
    ap.add_argument("--cell", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rows", type=int, default=81920)
    args = ap.parse_args()
    for n, conf in enumerate(args.config.split(",")):
        B, G = (int(x) for x in conf.split("x"))
        trainers = {beta: build(B, G, args.history, beta, args.cell) for beta in (0.0, args.beta)}
        if n == 0:
            print(json.dumps(dict(codes_kernel(trainers[args.beta], args.rows, args.launches), actors=B)), flush=True)
        for tr in trainers.values():                         # warm-up: lazy allocations, first-use paths
            run_ms(tr, 2, 0)
        for rep in range(args.repeat):
            ms = {beta: run_ms(tr, args.calls, 0) for beta, tr in trainers.items()}      # the trainers in turn
            print(json.dumps(dict(bench="explore_process", actors=B, groups=G, repeat=rep, calls=args.calls,
                                  explore_beta=args.beta, explore_cell=args.cell, ms_off=round(ms[0.0], 3),
                                  ms_on=round(ms[args.beta], 3), cost_ms=round(ms[args.beta] - ms[0.0], 3),
                                  cost_per_update_us=round(1e3 * (ms[args.beta] - ms[0.0]) / G, 1),
                                  cost_share=round(ms[args.beta] / ms[0.0] - 1.0, 4))), flush=True)
        del trainers
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
