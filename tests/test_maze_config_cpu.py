"""Configured mazes on the host: validation of Environment.register_maze_config, the configuration block, and the host
model (tests/maze_model.py) against the reference maze's oracle and Philox's known answers."""
import os

import numpy as np
import pytest

from oracle import maze as OM
from unreal_amd.environment.environment import Environment
from unreal_amd.environment.maze_environment import MazeConfig, REFERENCE_MAP

try:
    import maze_model as MM
except ImportError:            # imported as tests.<module>
    from tests import maze_model as MM

OPEN7 = "S" + "-" * 47 + "G"


@pytest.mark.parametrize("layouts,kw,what", [
    ([], {}, "non-empty"),
    ("S-----G", {}, "non-empty"),
    (["S" + "-" * 34 + "G"], {}, "cells"),                               # 36 cells: N = 6 does not tile 84 px
    (["S" + "-" * 62 + "G"], {}, "cells"),                               # 8 x 8
    ([OPEN7, "S" + "-" * 142 + "G"], {}, "share"),                       # 7 x 7 and 12 x 12 in one config
    (["S" + "-" * 46 + "xG"], {}, "unknown"),
    (["--" + "-" * 46 + "G"], {}, "'S'"),                                # no S without random_start
    (["SS" + "-" * 46 + "G"], {}, "'S'"),
    (["S" + "-" * 48], {}, "'G'"),                                       # no G without random_goal
    (["S" + "-" * 46 + "GG"], {}, "'G'"),
    (["S-+" + "-" * 4 + "+" * 3 + "-" * 39], dict(random_goal=True), "4-connected"),
    ([["S--+---", "---+---", "---+---", "---+---", "---+---", "---+---", "---+--G"]], {}, "4-connected"),
    ([["S------"] * 6 + ["-----G"]], {}, "rows"),                        # a short row
    (["S" + "+" * 48], dict(random_start=True, random_goal=True), "at least 2"),
    (["+" * 48 + "G"], dict(random_start=True), "at least 2"),
    ([OPEN7] * 1025, {}, "at most"),
    ([OPEN7], dict(max_episode_steps=-1), "max_episode_steps"),
    ([OPEN7], dict(max_episode_steps=2.5), "max_episode_steps"),
    ([OPEN7], dict(max_episode_steps=2 ** 31), "max_episode_steps"),
])
def test_malformed_configs_are_rejected(layouts, kw, what):
    with pytest.raises(ValueError, match=what):
        Environment.register_maze_config("bad", layouts, **kw)
    assert "bad" not in Environment.MAZE_CONFIG


def test_well_formed_configs_register():
    rows = [REFERENCE_MAP[7 * i:7 * i + 7] for i in range(7)]
    for name, lay in (("ref_str", [REFERENCE_MAP]), ("ref_rows", [rows]), ("ref_lines", ["\n".join(rows)])):
        Environment.register_maze_config(name, lay)
        c = Environment.MAZE_CONFIG.pop(name)
        assert (c.N, c.L, c.start[0], c.goal[0]) == (7, 1, 14, 6)
    for N in MazeConfig.SIZES:
        rs = np.random.RandomState(N)
        c = MazeConfig([MM.random_layout(N, rs, marks="") for _ in range(3)], random_start=True, random_goal=True,
                       show_goal=True, max_episode_steps=37)
        assert (c.N, c.L, c.flags) == (N, 3, 7)
    MazeConfig([OPEN7] * 1024)
    assert MazeConfig([OPEN7], max_episode_steps=2 ** 31 - 1).block(0)[3] == 2 ** 31 - 1


def test_block_layout():
    c = MazeConfig.reference()
    blk = c.block(0x0123456789ABCDEF)
    rec = c.RECORD_HEADER + 49
    assert blk.dtype == np.int32 and blk.size == c.HEADER + rec
    assert list(blk[:8].view(np.uint32)) == [7, 1, 0, 0, 0x89ABCDEF, 0x01234567, rec, 0]
    r = blk[c.HEADER:]
    walls = int(r[0].view(np.uint32)) | (int(r[1].view(np.uint32)) << 32)
    assert walls == sum(1 << i for i, ch in enumerate(REFERENCE_MAP) if ch == "+")
    assert not r[2:14].any()
    free = [i for i, ch in enumerate(REFERENCE_MAP) if ch != "+"]
    assert list(r[14:18]) == [14, 6, len(free), free.index(6)]
    assert list(r[18:18 + len(free)]) == free
    # 21 x 21: bits 0..440 over seven uint64 words
    lay = "S" + "-" * 439 + "+"
    c = MazeConfig([lay], random_goal=True)
    r = c.block(1)[c.HEADER:]
    assert r[13].view(np.uint32) == 1 << (440 - 6 * 64 - 32)
    assert list(r[14:18]) == [0, -1, 440, -1]


def test_layout_assignment_is_contiguous_blocks():
    c = MazeConfig([OPEN7] * 5)
    ids = c.layout_ids(0, 200, 200)
    assert list(ids) == [g * 5 // 200 for g in range(200)]
    assert list(np.concatenate([c.layout_ids(0, 100, 200), c.layout_ids(100, 100, 200)])) == list(ids)


def test_numpy_philox_known_answers():
    """Random123 kat_vectors for philox4x32-10: counter = key = 0, and the pi-digit vector."""
    out = MM.philox4x32_10((0, 0, 0, 0), (0, 0))
    assert [int(w) for w in out] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    out = MM.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))
    assert [int(w) for w in out] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def _run_pair(env, orc, actions):
    for a in actions:
        _, r, t, pc = env.process(int(a))
        _, r_o, t_o, pc_o = orc.process(int(a))
        assert (env.x, env.y) == (orc.x, orc.y)
        assert (r, t) == (r_o, t_o)
        np.testing.assert_array_equal(pc, pc_o)
        np.testing.assert_array_equal(env.last_state['image'], orc.last_state['image'])
        if t:
            env.reset()
            orc.reset()
            np.testing.assert_array_equal(env.last_state['image'], orc.last_state['image'])


def test_host_model_is_the_reference_maze_on_a_random_trace():
    env, orc = MM.HostMaze(MazeConfig.reference()), OM.OracleMaze()
    assert (env.x, env.y) == OM.START and (env.gx, env.gy) == OM.GOAL
    _run_pair(env, orc, np.random.RandomState(5).randint(0, 4, 2000))


def test_host_model_replays_the_golden_trace(golden_dir):
    g = np.load(os.path.join(golden_dir, "maze_trace.npz"))
    env = MM.HostMaze(MazeConfig.reference())
    for i, a in enumerate(g["actions"]):
        _, r, t, pc = env.process(int(a))
        assert (env.x, env.y) == tuple(g["pos"][i])
        assert r == g["reward"][i] and bool(t) == bool(g["terminal"][i])
        assert pc.sum() == g["pc_sum"][i]
        if t:
            env.reset()


def test_reset_draws_do_not_depend_on_the_split():
    rs = np.random.RandomState(3)
    c = MazeConfig([MM.random_layout(12, rs, marks="") for _ in range(4)], random_start=True, random_goal=True,
                   max_episode_steps=9)
    B = 40
    whole = MM.host_batch(c, B, seed=77)
    halves = MM.host_batch(c, B // 2, 0, B, seed=77) + MM.host_batch(c, B // 2, B // 2, B, seed=77)
    acts = rs.randint(0, 4, (60, B))
    starts = set()
    for t in range(60):
        for b in range(B):
            for env in (whole[b], halves[b]):
                _, _, term, _ = env.process(acts[t, b])
                if term:
                    env.reset()
            assert (whole[b].x, whole[b].y, whole[b].gx, whole[b].gy, whole[b].episode) == \
                (halves[b].x, halves[b].y, halves[b].gx, halves[b].gy, halves[b].episode)
            starts.add((whole[b].layout, whole[b].x, whole[b].y))
    assert all(e.episode >= 5 for e in whole)          # the step limit of 9 ended at least 6 episodes per actor
    assert len(starts) > 40


def test_random_start_is_never_the_goal_and_covers_the_free_cells():
    c = MazeConfig(["S" + "-" * 47 + "G"], random_start=True)
    seen = set()
    for ep in range(2000):
        goal, start = MM.reset_cells(c, 0, 3, ep, 11)
        assert goal == 48 and start != goal
        seen.add(start)
    assert seen == set(range(48))
