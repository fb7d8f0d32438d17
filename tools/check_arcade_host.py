#!/usr/bin/env python3
"""The device arcade's own game functions, tick loop and render on the CPU, under AddressSanitizer and UBSan, against the
host models of tests/repeat_model.py (Breakout and the duel), tests/invaders_model.py (invaders, §7n),
tests/crossing_model.py (crossing, §7x: five random traces, two scripted ones) and
tests/selfplay_model.py (the self-play duel's two-action tick and mirror, §7v).  No GPU is used and nothing loaded into Python is sanitized.

The functions are cut unchanged out of unreal_amd/csrc/arcade.hip, one range from its constants to the last overload of
`SeatSide` (everything in front of `store_frame`: `load`, `step_game`, `step_ticks`, `game_ended`, `game_over`, `shown`,
`reset_episode`, `store_game`, `frame_dirty`, `diff_dword`, `frame_chunk`, ..., of all four games and of the two-seat duel),
and the Philox draw out of maze_common.h, and compiled with tools/arcade_host_main.cpp into a stand-alone program whose one
driver calls the overloads the kernels' one step body and one reset body call, in their order.  Over every trace of tests/repeat_model.py (six random ones of 200 actors x 300 agent steps, two scripted ones) and
of tests/invaders_model.py (four random ones, one scripted) it is compared on every record, reward, terminal, ep_steps and episode, on every frame byte of the traces' watched actors, and
inside the program every difference dword of the dirty-row path against the full byte-wise difference of the two frames.
The self-play functions (`mirror`, `step_game2`, `step_ticks2` and the overloads of `SeatSide`) lie in the same range; over
the four traces of tests/selfplay_model.py (64 seats x 300 steps) every seat steps its pair's game from its own
record as a workgroup does and is compared on the same words, and on the frames of the first three pairs.
The program's `versus` mode runs the one-workgroup two-view step over the same four traces as 32 games of one
learner each (even columns the learner's actions, odd ones the opponent's): records, rewards, terminals, ep_steps, episode
and the opponent's last action and reward of every game against HostSeat 2 i and 2 i + 1, both frames of the first three.

  python tools/check_arcade_host.py [--cxx clang++] [--keep DIR]"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CSRC = os.path.join(ROOT, "unreal_amd", "csrc")


def cut(path, first, last):
    """The lines of `path` from the one that starts with `first` up to, not including, the one that starts with `last`."""
    lines = open(path).read().split("\n")
    i = [n for n, l in enumerate(lines) if l.startswith(first)]
    j = [n for n, l in enumerate(lines) if l.startswith(last)]
    assert len(i) == 1 and len(j) == 1 and i[0] < j[0], (path, first, last)
    return "\n".join(lines[i[0]:j[0]]) + "\n"


def selfplay_traces(exe, work):
    """The four traces of tests/selfplay_model.py through the program's `selfplay` mode -> agent steps compared."""
    import selfplay_model as SM
    from unreal_amd.environment.arcade_environment import ArcadeSelfPlay
    total = n = 0
    B, S, F = SM.TRACE_B, SM.TRACE_STEPS, 2 * SM.TRACE_PAIR_FRAMES
    for k, kw in enumerate(SM.TRACE_SETTINGS):
        conf = ArcadeSelfPlay(**kw)
        acts, active = SM.trace_inputs(k)
        head = np.concatenate([conf.block(SM.TRACE_SEED), np.array([B, S, F, 0], np.int32)])
        fin, fout = os.path.join(work, "selfplay%d.in" % k), os.path.join(work, "selfplay%d.out" % k)
        np.concatenate([head, acts.reshape(-1), active.reshape(-1)]).astype(np.int32).tofile(fin)
        subprocess.check_call([exe, fin, fout, "selfplay"])  # a sanitizer report or a wrong difference dword ends it here
        raw = np.fromfile(fout, dtype=np.uint8).reshape(S, F * 21168 + B * 80)
        frames = raw[:, :F * 21168].reshape(S, F, 21168)
        words = np.ascontiguousarray(raw[:, F * 21168:]).view(np.int32).reshape(S, B, 20)
        seats = [SM.HostSeat(conf, b, SM.TRACE_SEED, frames=b < F) for b in range(B)]
        for s in range(S):
            out = SM.step_pairs(seats, acts[s], active[s])
            for b, (r, t, pc, stepped) in enumerate(out):
                if b < F:                                     # the frame before a reset; an idle seat's current frame
                    np.testing.assert_array_equal(frames[s, b], seats[b].frame.reshape(-1),
                                                  err_msg="frame of self-play trace %d step %d seat %d" % (k, s, b))
                if stepped and t:
                    seats[b].reset()
                want = list(seats[b].record()) + [r if stepped else -7, int(t) if stepped else -7, seats[b].ep_steps,
                                                  seats[b].episode]
                np.testing.assert_array_equal(words[s, b], want, err_msg="self-play trace %d step %d seat %d" % (k, s, b))
                total += int(stepped)
        np.testing.assert_array_equal(words[:, 1::2, :16], SM.mirror(words[:, 0::2, :16]))
        print("self-play trace %d (action_repeat %d, return_reward %d): %d agent steps, %d frames agree"
              % (k, conf.action_repeat, conf.return_reward, total - n, S * F), flush=True)
        n = total
    return total


def versus_traces(exe, work):
    """The four traces of tests/selfplay_model.py through the program's `versus` mode -> agent steps compared."""
    import selfplay_model as SM
    from unreal_amd.environment.arcade_environment import ArcadeSelfPlay
    total = 0
    B, S, F = SM.TRACE_B, SM.TRACE_STEPS, SM.TRACE_PAIR_FRAMES
    G = B // 2
    for k, kw in enumerate(SM.TRACE_SETTINGS):
        conf = ArcadeSelfPlay(**kw)
        acts, active = SM.trace_inputs(k)
        head = np.concatenate([conf.block(SM.TRACE_SEED), np.array([B, S, F, 0], np.int32)])
        fin, fout = os.path.join(work, "versus%d.in" % k), os.path.join(work, "versus%d.out" % k)
        np.concatenate([head, acts.reshape(-1), active.reshape(-1)]).astype(np.int32).tofile(fin)
        subprocess.check_call([exe, fin, fout, "versus"])    # a sanitizer report or a wrong difference dword ends it here
        raw = np.fromfile(fout, dtype=np.uint8).reshape(S, 2 * F * 21168 + G * 88)
        frames = raw[:, :2 * F * 21168].reshape(S, F, 2, 21168)
        words = np.ascontiguousarray(raw[:, 2 * F * 21168:]).view(np.int32).reshape(S, G, 22)
        seats = [SM.HostSeat(conf, b, SM.TRACE_SEED, frames=b < 2 * F) for b in range(B)]
        n = 0
        for s in range(S):
            out = SM.step_pairs(seats, acts[s], active[s])
            for i in range(G):
                r, t, pc, stepped = out[2 * i]
                if i < F:                                     # the learner's frame before a reset
                    np.testing.assert_array_equal(frames[s, i, 0], seats[2 * i].frame.reshape(-1),
                                                  err_msg="learner frame of versus trace %d step %d game %d" % (k, s, i))
                if stepped and t:
                    seats[2 * i].reset(); seats[2 * i + 1].reset()
                if i < F:                                     # the opponent's frame after it
                    np.testing.assert_array_equal(frames[s, i, 1], seats[2 * i + 1].frame.reshape(-1),
                                                  err_msg="opponent frame of versus trace %d step %d game %d" % (k, s, i))
                want = list(seats[2 * i].record()) + [r if stepped else -7, int(t) if stepped else -7, seats[2 * i].ep_steps,
                                                      seats[2 * i].episode, seats[2 * i + 1].last_action,
                                                      seats[2 * i + 1].last_reward]
                np.testing.assert_array_equal(words[s, i], want, err_msg="versus trace %d step %d game %d" % (k, s, i))
                n += int(stepped)
        print("versus trace %d (action_repeat %d, return_reward %d): %d agent steps of %d games, %d frames agree"
              % (k, conf.action_repeat, conf.return_reward, n, G, 2 * S * F), flush=True)
        total += n
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default=os.environ.get("CXX") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++")
    ap.add_argument("--keep", default="", help="work in this directory and keep it")
    args = ap.parse_args()
    import crossing_model as CM
    import invaders_model as IM
    import repeat_model as RM
    work = args.keep or tempfile.mkdtemp(prefix="arcade_host_")
    os.makedirs(work, exist_ok=True)
    src = open(os.path.join(CSRC, "arcade.hip")).read()
    begin = src.index("constexpr int kArcadeBreakout")
    end = src.index("template <class G, class R>\n__device__ __forceinline__ void store_frame")
    with open(os.path.join(work, "arcade_functions.inc"), "w") as f:
        f.write(cut(os.path.join(CSRC, "maze_common.h"), "// ---- Philox4x32-10", "// ---- maze configuration block"))
        f.write(src[begin:end])
    exe = os.path.join(work, "arcade_host_check")
    subprocess.check_call([args.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", work, os.path.join(ROOT, "tools", "arcade_host_main.cpp"), "-o", exe])
    total = 0
    traces = [(RM, k) for k in range(len(RM.TRACE_SETTINGS) + len(RM.SCRIPTED_SETTINGS))] + \
             [(IM, k) for k in range(IM.N_TRACES)] + [(CM, k) for k in range(CM.N_TRACES)]
    for n, (mod, k) in enumerate(traces):
        conf, tr = mod.trace_config(k), mod.run_trace(k)
        S, B = tr["acts"].shape
        F = tr["pc"].shape[1]
        head = np.concatenate([conf.block(mod.TRACE_SEED), np.array([B, S, F, 0], np.int32)])
        k = n
        fin, fout = os.path.join(work, "trace%d.in" % k), os.path.join(work, "trace%d.out" % k)
        np.concatenate([head, tr["acts"].reshape(-1), tr["active"].reshape(-1)]).astype(np.int32).tofile(fin)
        subprocess.check_call([exe, fin, fout])            # a sanitizer report or a wrong difference dword ends it here
        raw = np.fromfile(fout, dtype=np.uint8).reshape(S, F * 21168 + B * 80)
        frames = raw[:, :F * 21168].reshape(S, F, 21168)
        words = np.ascontiguousarray(raw[:, F * 21168:]).view(np.int32).reshape(S, B, 20)
        np.testing.assert_array_equal(words[:, :, :16], tr["records"], err_msg="records of trace %d" % k)
        np.testing.assert_array_equal(words[:, :, 16], np.where(tr["active"] != 0, tr["reward"], -7).astype(np.int32))
        np.testing.assert_array_equal(words[:, :, 17], tr["terminal"], err_msg="terminals of trace %d" % k)
        np.testing.assert_array_equal(words[:, :, 18], tr["ep_steps"], err_msg="ep_steps of trace %d" % k)
        np.testing.assert_array_equal(words[:, :, 19], tr["episode"], err_msg="episodes of trace %d" % k)
        for s in range(S):
            for b in range(F):
                rec = tr["pre_reset"][s, b] if tr["active"][s, b] else tr["records"][s, b]
                np.testing.assert_array_equal(frames[s, b], mod.frame_of(conf, rec).reshape(-1),
                                              err_msg="frame of trace %d step %d actor %d" % (k, s, b))
        total += int(tr["active"].sum())
        print("trace %d (%s, action_repeat %d, return_reward %d): %d agent steps, %d frames agree"
              % (k, conf.game, conf.action_repeat, conf.return_reward, int(tr["active"].sum()), S * F), flush=True)
    total += selfplay_traces(exe, work)
    total += versus_traces(exe, work)
    print("arcade host check ok: %d agent steps; the sanitizers reported nothing" % total)
    if not args.keep:
        shutil.rmtree(work)


if __name__ == "__main__":
    main()
