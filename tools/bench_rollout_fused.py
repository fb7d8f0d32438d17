#!/usr/bin/env python3
"""Same-process A/B of the rollout step that also encodes its next frame (unreal_maze_policy_rollout_step_encode,
Trainer.fuse_env_encoder) against the two launches it replaces, on bench.py's trainer.  GPU box.

  1. launches, interleaved: (a) unreal_maze_policy_rollout_step + unreal_encoder_fwd on next_idx, (b) the fused launch,
     on the trainer's own rows and ring -> us per rollout step (median and mean of HIP-event brackets);
  2. whole process() calls with the flag off and on, interleaved rounds -> ms per call.

usage: python tools/bench_rollout_fused.py [--actors 4096] [--history 2000] [--reps 200] [--calls 20] [--rounds 3]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from bench import build_trainer  # noqa: E402
from unreal_amd import ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--actors", type=int, default=4096)
ap.add_argument("--history", type=int, default=2000)
ap.add_argument("--groups", type=int, default=1)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
dev = torch.device("cuda", 0)
flags, net, tr = build_trainer(args, 0, 1, dev)
while not tr._full:
    tr.process(None, 0)
gt = 0
for _ in range(3):
    tr.process(None, gt, sync_stats=False); gt += args.actors * 20
torch.cuda.synchronize()
med = lambda v: sorted(v)[len(v) // 2]

# ---- 1. the launches ----------------------------------------------------------------------------------------------------
B, A, ws, env = tr.Bg, tr.action_size, tr.base_ws, tr.environment
assert env.fused_encoder_ok and ws.c1 is not None and ws.f2_bits is not None
net.begin_pass()
feat, ld = net.features(ws, 0)
s_f2, _, s_c1 = net.ws_slots(ws)
s = slice(0, B)
nxt = dict(next_idx=ws.frame_idx[B:2 * B])
if tr.use_lstm:
    nxt.update(next_lar=ws.xcat[B * ws.xld:], lar_ld=ws.xld, lar_col0=256, A=A)
step_args = (net, feat, ld, tr.u_act[s], tr.pi[:B * A], tr.v[s], tr.actions[s], tr.rewards[s], tr.terminals[s], tr.active,
             tr.active_log[s], tr.n_steps, tr.terminal_end)
enc_out = (ws.f2[B * net.F:], ws.c1[B * net.c1_dim:], ws.f2_bits[B * ops.RELU_WORDS:])


def two_launches():
    env.policy_rollout_step(*step_args, **dict(nxt))
    net.encoder_forward(tr.ring, ws.frame_idx[B:2 * B], enc_out[0], enc_out[1], relu_bits=enc_out[2], f2_max=s_f2,
                        c1_max=s_c1, ws=ws)


def one_launch():
    env.policy_rollout_step_encode(*step_args, *enc_out, s_f2, s_c1, **dict(nxt))


tr.draws.uniform(tr.u_act)
ev = {"two_launches": [], "fused": []}
for rep in range(args.reps + 5):
    for name, fn in (("two_launches", two_launches), ("fused", one_launch)):
        tr.active.fill_(1)                      # every actor steps, as at the start of a rollout
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        if rep >= 5:
            ev[name].append((e0, e1))
torch.cuda.synchronize()
us = {k: [a.elapsed_time(b) * 1e3 for a, b in v] for k, v in ev.items()}
for k, v in us.items():
    print("%-13s %7.1f us per rollout step (median of %d; mean %.1f, min %.1f)" % (k, med(v), len(v), sum(v) / len(v), min(v)),
          flush=True)

# ---- 2. whole process() calls -------------------------------------------------------------------------------------------
res = {"off": [], "on": []}
for r in range(args.rounds):
    for name, flag in (("off", False), ("on", True)):
        tr.fuse_env_encoder = flag
        tr.process(None, gt, sync_stats=False); gt += args.actors * 20
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(args.calls):
            tr.process(None, gt, sync_stats=False); gt += args.actors * 20
        torch.cuda.synchronize()
        res[name].append((time.perf_counter() - t0) / args.calls * 1e3)
        print("round %d fuse_env_encoder %-3s %.3f ms per process()" % (r, name, res[name][-1]), flush=True)
tr.read_stats()
losses = tr._publish_losses()
print(json.dumps({"actors": args.actors, "history": args.history, "us_two_launches": med(us["two_launches"]),
                  "us_fused": med(us["fused"]), "ms_process_off": res["off"], "ms_process_on": res["on"],
                  "delta_ms": med(res["on"]) - med(res["off"]), "total_loss": losses["total_loss"]}))
