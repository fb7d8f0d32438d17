#!/usr/bin/env python3
"""The library launches of Trainer.process(), recorded per call and compared between two trees.  GPU box.

Every launch goes through ops._call; inside `Trace` it is replaced (and restored on exit) by a wrapper that notes, per
launch: the entry name, the stream as an index by first appearance (ops.stream()), every argument include/unreal_hip.h
declares as a scalar by value, and every pointer argument as null (0) or non-null (*).  No kernel code is looked at and no
device memory is read.  Torch-level fills (zero_, fill_) are not launches of the library and are not in the trace.

Each configuration of CONFIGS is built with injected plain draws and fixed seeds, prepared (call 0 of its trace), filled
(one trace per fill call) and run for two learning process() calls.

  python tools/launch_trace.py --out FILE [--configs a_lstm,b_ff,...]          record
  python tools/launch_trace.py --compare FILE [--configs ...]                 exit 1 at the first difference, printed
  python tools/launch_trace.py --compare FILE --all [--configs ...]           every difference, counted per entry name

File format: per configuration the distinct launch records ("entry|stream|arg,arg,...") and, per call, the indices of
its launches into them."""
import argparse
import difflib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HEADER = os.path.join(ROOT, "include", "unreal_hip.h")
DEV = "cuda:0"
H, T = 40, 20


def header_scalars(path=HEADER):
    """-> {entry: [None for a pointer parameter, else float or int]} of every `int unreal_*(...)` prototype, the trailing
    `stream` dropped (the position of a parameter is its position among the arguments of ops._call)."""
    src = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(unreal_\w+)\s*\(([^)]*)\)\s*;", src):
        params = m.group(2).split(",")
        if re.findall(r"\w+", params[-1])[-1] == "stream":
            params.pop()
        out[m.group(1)] = [None if "*" in a else float if a.replace("const", "").split()[0] in ("float", "double") else int
                           for a in params]
    return out


class Trace(object):
    """Context manager: replaces ops._call (restored on exit); `calls` is a list of per-call lists of launch records."""

    def __init__(self):
        from unreal_amd import ops
        self.ops, self.kinds, self.streams, self.calls, self._orig = ops, header_scalars(), {}, [], None

    def __enter__(self):
        self._orig = self.ops._call
        self.ops._call = self._wrapped
        return self

    def __exit__(self, *exc):
        self.ops._call, self._orig = self._orig, None
        return False

    def next_call(self):
        self.calls.append([])

    def _wrapped(self, name, *a):
        s = self.streams.setdefault(self.ops.stream(), len(self.streams))
        args = [("*" if v else "0") if k is None else repr(k(v)) for k, v in zip(self.kinds[name], a)]
        self.calls[-1].append("%s|%d|%s" % (name[len("unreal_"):], s, ",".join(args)))
        return self._orig(name, *a)


# ---- the configurations --------------------------------------------------------------------------------------------------------
def _trainer(B, lstm=True, aux=True, env=("maze", ""), net_seed=3, frame_scale=None, **options):
    """aux: True / False for all three auxiliary tasks, or a (pixel_change, value_replay, reward_prediction) triple."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer, PhiloxDraws
    pc, vr, rp = (aux, aux, aux) if isinstance(aux, bool) else aux
    Environment.action_size = -1
    A = Environment.get_action_size(*env)
    net = UnrealModel(A, 0, -1, lstm, pc, vr, rp, 0.05, 0.001, DEV, seed=net_seed, frame_scale=frame_scale)
    applier = RMSPropApplier(None, decay=0.99, momentum=0.0, epsilon=0.1, clip_norm=40.0, device=DEV)
    return Trainer(0, net, 7.0711e-4, None, applier, env[0], env[1], lstm, pc, vr, rp, 0.05, 0.001, T, T, 0.99, 0.9, H,
                   10 ** 6, DEV, batch_size=B, draws=PhiloxDraws(0xA3C, 0), seed=21, **options)


def _lab(B, overlap):
    from unreal_amd.environment.synthetic_sim import SyntheticBatchSimulator
    sim = SyntheticBatchSimulator(B, seed=4, episode_len=7, reward_p=0.3, big_reward_p=0.1)
    return _trainer(B, env=("lab", ""), net_seed=9, frame_scale=1.0 / 255.0, simulator=sim, overlap_host=overlap)


def _fp_minibatch():
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.maze_environment import REFERENCE_MAP
    Environment.register_maze_config("launch_trace_fp7", [REFERENCE_MAP], view="first_person", random_start=True,
                                     random_goal=True, max_episode_steps=7)
    return _trainer(8, env=("maze", "launch_trace_fp7"), reuse_epochs=2, reuse_minibatches=2)


def _arcade_timelimit():
    from unreal_amd.environment.environment import Environment
    Environment.register_arcade_config("launch_trace_breakout", rows=1, lives=1, paddle_width=4, ball_speed=4, serve_wait=0,
                                       max_episode_steps=9)
    return _trainer(4, env=("arcade", "launch_trace_breakout"), bootstrap_timeouts=True)


# name -> (Trainer class attributes set while the trainer is built and run, builder)
CONFIGS = [
    ("a_lstm", {}, lambda: _trainer(4)),
    ("b_ff", {}, lambda: _trainer(4, lstm=False)),
    ("c_pc", {}, lambda: _trainer(4, aux=(True, False, False))),
    ("c_vr", {}, lambda: _trainer(4, aux=(False, True, False))),
    ("c_rp", {}, lambda: _trainer(4, aux=(False, False, True))),
    ("c_pc_rp", {}, lambda: _trainer(4, aux=(True, False, True))),
    ("d_unbatched", dict(batch_aux_default=False), lambda: _trainer(4)),
    ("e_groups2", {}, lambda: _trainer(8, groups=2)),
    ("f_lab_lockstep", {}, lambda: _lab(3, False)),
    ("f_lab_overlap", {}, lambda: _lab(4, True)),
    ("g_half_batch", dict(rollout_parts_default=2, ROLLOUT_SPLIT_MIN_ACTORS=2), lambda: _trainer(8)),
    ("h_fused_encoder", {}, lambda: _trainer(2048)),
    ("i_minibatch", {}, _fp_minibatch),
    ("j_arcade_timelimit", {}, _arcade_timelimit),
]


def run(name, patch, build):
    """-> the per-call traces of one configuration: prepare(), the replay fill, two learning calls."""
    import torch
    from unreal_amd.train.trainer import Trainer
    saved = dict((k, getattr(Trainer, k)) for k in patch)
    for k, v in patch.items():
        setattr(Trainer, k, v)
    try:
        with Trace() as trace:
            trace.next_call()
            tr = build()
            tr.prepare()
            g, learned = 0, 0
            while learned < 2:
                trace.next_call()
                learned += tr._full
                steps, _ = tr.process(None, g)
                g += steps
        torch.cuda.synchronize()
        tr.stop()
    finally:
        for k, v in saved.items():
            setattr(Trainer, k, v)
    del tr
    torch.cuda.empty_cache()
    return trace.calls


def pack(calls):
    index = {}
    packed = [[index.setdefault(r, len(index)) for r in call] for call in calls]
    records = sorted(index, key=index.get)
    return dict(records=records, calls=packed)


def unpack(doc):
    return [[doc["records"][i] for i in call] for call in doc["calls"]]


def write(path, doc):
    """One line per record and per call: the file diffs and greps like a text."""
    lines = ["{"]
    for n, (name, d) in enumerate(sorted(doc.items())):
        lines.append(' %s: {\n  "records": [' % json.dumps(name))
        lines += ["   %s%s" % (json.dumps(r), "," if k + 1 < len(d["records"]) else "") for k, r in enumerate(d["records"])]
        lines.append('  ],\n  "calls": [')
        lines += ["   %s%s" % (json.dumps(c, separators=(",", ":")), "," if k + 1 < len(d["calls"]) else "")
                  for k, c in enumerate(d["calls"])]
        lines.append("  ]\n }%s" % ("," if n + 1 < len(doc) else ""))
    lines.append("}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def first_difference(name, want, got):
    if len(want) != len(got):
        return "%s: %d calls recorded, %d now" % (name, len(want), len(got))
    for c, (w, g) in enumerate(zip(want, got)):
        for k in range(max(len(w), len(g))):
            a, b = (w[k] if k < len(w) else "<end of call>"), (g[k] if k < len(g) else "<end of call>")
            if a != b:
                return "%s: call %d, launch %d\n  recorded: %s\n  now:      %s" % (name, c, k, a, b)
    return None


def all_differences(want, got):
    """-> {(what, entry): count} over the calls: launches only recorded ('-'), only now ('+'), by entry name."""
    out = {}
    for w, g in zip(want, got):
        for tag, i0, i1, j0, j1 in difflib.SequenceMatcher(None, w, g, autojunk=False).get_opcodes():
            if tag == "equal":
                continue
            for what, recs in (("-", w[i0:i1]), ("+", g[j0:j1])):
                for r in recs:
                    key = (what, r.split("|")[0])
                    out[key] = out.get(key, 0) + 1
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="record the traces into this JSON file")
    ap.add_argument("--compare", help="compare the traces with this JSON file")
    ap.add_argument("--all", action="store_true", help="with --compare: list every difference instead of stopping")
    ap.add_argument("--configs", help="comma-separated configuration names (default: all)")
    args = ap.parse_args()
    if bool(args.out) == bool(args.compare):
        ap.error("one of --out FILE, --compare FILE")
    names = args.configs.split(",") if args.configs else [c[0] for c in CONFIGS]
    unknown = set(names) - set(c[0] for c in CONFIGS)
    if unknown:
        ap.error("unknown configuration(s) %s" % sorted(unknown))
    recorded = json.load(open(args.compare)) if args.compare else {}
    doc, differ = {}, 0
    for name, patch, build in CONFIGS:
        if name not in names:
            continue
        calls = run(name, patch, build)
        print("%s: %d calls, %d launches" % (name, len(calls), sum(len(c) for c in calls)), flush=True)
        if args.out:
            doc[name] = pack(calls)
            continue
        if name not in recorded:
            print("%s: not in %s" % (name, args.compare))
            return 1
        want = unpack(recorded[name])
        msg = first_difference(name, want, calls)
        if msg is None:
            continue
        differ += 1
        print(msg)
        if not args.all:
            return 1
        for (what, entry), n in sorted(all_differences(want, calls).items(), key=lambda kv: (kv[0][1], kv[0][0])):
            print("  %s %-28s x %d" % (what, entry, n))
    if args.out:
        write(args.out, doc)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
