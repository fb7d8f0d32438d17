"""Goal-sense first-person mazes without a GPU: MazeConfig's validation, block words and reward bound, the
record widths against the header's macros, the breadth-first search's known answers, the goal offset under turns, a
generated maze's field, and the new entry's argument checks."""
import os
import re

import numpy as np
import pytest

try:
    import goal_maze_model as GOAL
    import maze_model as MM
except ImportError:            # imported as tests.<module>
    from tests import goal_maze_model as GOAL
    from tests import maze_model as MM

from unreal_amd.environment.maze_environment import MazeConfig, REFERENCE_MAP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (7, 12, 14, 21)
FP_KW = dict(random_start=True, random_goal=True, view="first_person")


def _layout(N=7, seed=0, marks=""):
    return MM.random_layout(N, np.random.RandomState(seed), marks=marks)


def gen_config(N, **kw):
    return MazeConfig(None, generate=N, **dict(FP_KW, **kw))


# ---- surface -----------------------------------------------------------------------------------------------------------
def test_validation_errors():
    lay = _layout()
    ok = MazeConfig([lay], goal_sense=True, progress_reward=2, **FP_KW)
    assert ok.goal_sense and ok.nav and ok.progress_reward == 2
    assert not MazeConfig([lay], **FP_KW).goal_sense
    with pytest.raises(ValueError):                      # first person only
        MazeConfig([lay], random_start=True, random_goal=True, goal_sense=True)
    with pytest.raises(ValueError):
        MazeConfig([lay], random_start=True, random_goal=True, view="top_down", goal_sense=True)
    with pytest.raises(ValueError):                      # a progress reward pays for a distance: needs goal_sense
        MazeConfig([lay], progress_reward=1, **FP_KW)
    for bad in (True, False, 1.0, 0.5, "1", None, 101, -101, np.bool_(True), np.float32(1)):
        with pytest.raises(ValueError):
            MazeConfig([lay], goal_sense=True, progress_reward=bad, **FP_KW)
    for good in (-100, 100, 0, np.int32(7)):
        assert MazeConfig([lay], goal_sense=True, progress_reward=good, **FP_KW).progress_reward == int(good)
    with pytest.raises(ValueError):
        gen_config(7, view="top_down", goal_sense=True)
    assert gen_config(7, goal_sense=True).nav


def test_register_and_objective_size():
    from unreal_amd.environment.environment import Environment
    lay = _layout()
    try:
        Environment.register_maze_config("goal_cpu_on", [lay], goal_sense=True, progress_reward=-3, **FP_KW)
        Environment.register_maze_config("goal_cpu_off", [lay], **FP_KW)
        Environment.register_maze_config("goal_cpu_gen", None, generate=12, goal_sense=True, **FP_KW)
        assert Environment.MAZE_CONFIG["goal_cpu_on"].progress_reward == -3
        assert Environment.get_objective_size("maze", "goal_cpu_on") == 3
        assert Environment.get_objective_size("maze", "goal_cpu_gen") == 3
        assert Environment.get_objective_size("maze", "goal_cpu_off") == 0
        assert Environment.get_objective_size("maze", "never_registered") == 0
        assert Environment.get_objective_size("lab", "goal_cpu_on") == 0
        with pytest.raises(ValueError):
            Environment.register_maze_config("goal_cpu_bad", [lay], random_start=True, random_goal=True, goal_sense=True)
        assert "goal_cpu_bad" not in Environment.MAZE_CONFIG
    finally:
        for name in ("goal_cpu_on", "goal_cpu_off", "goal_cpu_gen"):
            Environment.MAZE_CONFIG.pop(name, None)


def test_block_words():
    """Without the options the block is what it was, word for word; with them flag 64 (and the navigation flag) and the
    progress word are the only difference from the navigation block of the same config."""
    lay = _layout(12, 3, marks="SG")
    seed = 0x1234567890
    plain = MazeConfig([lay], view="first_person")
    assert not plain.nav and not plain.flags & (MazeConfig.GOAL_SENSE | MazeConfig.NAV)
    np.testing.assert_array_equal(plain.block(seed), MazeConfig([lay], view="first_person", goal_sense=False,
                                                                progress_reward=0).block(seed))
    assert len(plain.block(seed)) == 8 + 18 + 144          # no extension at all
    nav = MazeConfig([lay], view="first_person", goal_reward=5)
    ext = 8 + 18 + 144
    nb = nav.block(seed)
    assert list(nb[ext:ext + 8]) == [5, 1, -1, 0, 0, 0, 0, 0] and not nb[2] & 64
    for p in (0, 7, -4):
        sense = MazeConfig([lay], view="first_person", goal_reward=5, goal_sense=True, progress_reward=p)
        sb = sense.block(seed)
        assert sb[2] == nb[2] | 64 and sb[2] & 8
        assert list(sb[ext:ext + 8]) == [5, 1, -1, 0, 0, 0, p, 0]
        same = np.ones(len(sb), dtype=bool)
        same[[2, ext + 6]] = False
        np.testing.assert_array_equal(sb[same], nb[same])
    # default rewards: still a navigation block (the rewards header is there)
    sb = MazeConfig([lay], view="first_person", goal_sense=True).block(seed)
    assert sb[2] & 72 == 72 and list(sb[ext:ext + 8]) == [1, 1, -1, 0, 0, 0, 0, 0] and len(sb) == ext + 8 + 65
    # generated: gen_loops / gen_apples keep words 4 / 5, the progress reward is word 6
    g0 = gen_config(14, gen_loops=3, gen_apples=5, wall_styles=[(1, 2, 3, 4)], gen_landmark_density=9)
    g1 = gen_config(14, gen_loops=3, gen_apples=5, wall_styles=[(1, 2, 3, 4)], gen_landmark_density=9, goal_sense=True,
                    progress_reward=-2)
    b0, b1 = g0.block(seed), g1.block(seed)
    assert list(b1[8:16]) == [1, 1, -1, 0, 3, 5, -2, 0] and list(b0[8:16]) == [1, 1, -1, 0, 3, 5, 0, 0]
    assert b1[2] == b0[2] | 64
    same = np.ones(len(b1), dtype=bool)
    same[[2, 14]] = False
    np.testing.assert_array_equal(b1[same], b0[same])


def test_reward_bound():
    lay = _layout()
    rb = lambda **kw: MazeConfig([lay], **dict(FP_KW, **kw)).reward_bound
    assert rb() == 1 and rb(goal_reward=10, apple_reward=2, hit_reward=-3) == 10        # today's values
    assert rb(goal_sense=True) == 1
    assert rb(goal_sense=True, progress_reward=1) == 2                                   # goal 1 + 1, apple 1 + 1
    assert rb(goal_sense=True, progress_reward=-1) == 2                                  # apple 1 + |-1|; goal 1 - 1 = 0
    assert rb(goal_sense=True, progress_reward=-1, apple_reward=0) == 1                  # hit -1, move +-1
    assert rb(goal_sense=True, progress_reward=3, goal_reward=0, apple_reward=0, hit_reward=0) == 3
    assert rb(goal_sense=True, progress_reward=-5, goal_reward=10, apple_reward=0, hit_reward=-7) == 7
    assert rb(goal_sense=True, progress_reward=2, goal_reward=10, apple_reward=-9, hit_reward=0) == 12


def test_record_widths_match_the_header():
    from unreal_amd import ops
    src = open(os.path.join(ROOT, "include", "unreal_hip.h")).read()
    macros = dict(re.findall(r"#define (UNREAL_MAZE_\w+)\(N\) (.+)", src))

    def expand(name, N):
        expr = macros[name]
        for other in macros:
            expr = re.sub(other + r"\(N\)", lambda m, o=other: "(%d)" % expand(o, N), expr)
        return eval(expr.replace("/", "//").replace("(N)", "(%d)" % N))
    want = {7: 25, 12: 72, 14: 98, 21: 221}
    for N in SIZES:
        assert expand("UNREAL_MAZE_DIST_WORDS", N) == want[N] == ops.dist_words(N) == MazeConfig.dist_words(N) == \
            GOAL.dist_words(N)
        assert expand("UNREAL_MAZE_SENSE_RECORD", N) == 8 + want[N] == ops.sense_record_words(N)
        lay = _layout(N)
        assert MazeConfig([lay], goal_sense=True, **FP_KW).record_words == 8 + want[N]
        assert MazeConfig([lay], goal_reward=2, **FP_KW).record_words == 8
        assert MazeConfig([lay], **FP_KW).record_words == 0
        assert gen_config(N, goal_sense=True).record_words == expand("UNREAL_MAZE_GEN_RECORD", N) + want[N]
        assert gen_config(N).record_words == expand("UNREAL_MAZE_GEN_RECORD", N) == ops.gen_record_words(N)
        styled = gen_config(N, goal_sense=True, wall_styles=[(1, 2, 3, 4)])
        assert styled.record_words == expand("UNREAL_MAZE_GEN_STYLED_RECORD", N) + want[N]
    assert "#define UNREAL_MAZE_FIRST_PERSON_SENSE 3" in src and "#define UNREAL_MAZE_FIRST_PERSON_GENERATED_SENSE 4" in src
    assert (ops.MAZE_FIRST_PERSON_SENSE, ops.MAZE_FIRST_PERSON_GENERATED_SENSE) == (3, 4)


# ---- the search ----------------------------------------------------------------------------------------------------------
def test_bfs_known_answer_on_the_reference_map():
    conf = MazeConfig.reference()
    goal, start = REFERENCE_MAP.index("G"), REFERENCE_MAP.index("S")
    X = GOAL.NO_PATH
    for d in (np.array(GOAL.bfs(conf.walls[0], 7, goal)).reshape(7, 7), conf.distance_field(0, goal).astype(np.int64)):
        assert d[start // 7, start % 7] == 20
        assert list(d[0]) == [22, 21, X, 3, 2, 1, 0]
        assert list(d[6]) == [16, 15, 14, 13, 12, X, X]
        assert (d == X).sum() == REFERENCE_MAP.count("+")
    np.testing.assert_array_equal(conf.distance_field("\n".join(REFERENCE_MAP[7 * y:7 * y + 7] for y in range(7)), goal),
                                  conf.distance_field(0, goal))


def test_serpentine_needs_sixteen_bits():
    rows = GOAL.serpentine_layout(21)
    conf = MazeConfig([rows], view="first_person", start_heading=0, goal_sense=True, progress_reward=2)
    m = GOAL.HostGoalMaze(conf, 0, 1, seed=0)
    assert (m.x, m.y, m.gx, m.gy) == (0, 0, 20, 20)
    assert m.distance() == 240 and max(v for v in m.dist if v != GOAL.NO_PATH) == 240 > 255 - 16
    np.testing.assert_array_equal(conf.distance_field(0, 440), m.distance_field())
    assert m.record()[5:8] == [20, 20, 240]
    np.testing.assert_array_equal(m.last_state["objective"], [20 / 32.0, 20 / 32.0, 240 / 512.0])
    _, r, t, _ = m.process(2)                                # a step along the corridor
    assert (r, t, m.distance()) == (2, False, 239)
    _, r, t, _ = m.process(3)
    assert (r, t, m.distance()) == (-2, False, 240)
    _, r, t, _ = m.process(3)                                # back into the border: a hit, no progress
    assert (r, m.distance()) == (-1, 240)
    words = m.actor_record()
    assert len(words) == 8 + 221 and words[8] == 240 | 239 << 16          # cells 0 and 1
    assert (int(words[-1]) & 0xFFFF, (int(words[-1]) >> 16) & 0xFFFF) == (0, GOAL.NO_PATH)


def test_four_turns_rotate_the_offset():
    """A quarter turn rotates (gf, gs).  With §7e's axes (r = DIRS[(h + 1) % 4], action 1 = h + 1) a RIGHT turn brings what
    was on the right ahead: (gf, gs) -> (gs, -gf) -> (-gf, -gs) -> (-gs, gf) -> (gf, gs).  The orbit (gf, gs) -> (-gs, gf)
    -> (-gf, -gs) -> (gs, -gf) -> (gf, gs) is the same cycle run the other way: four LEFT turns (action 0).  Both are
    checked, on the formula and through the model's actions."""
    for gf, gs in ((3, -2), (0, 5), (-4, -4)):
        # a goal gf ahead and gs to the right of a camera at (10, 10) heading +x: (gx, gy) = (10 + gf, 10 + gs)
        gx, gy = 10 + gf, 10 + gs
        right = [GOAL.goal_offset(10, 10, h, gx, gy) for h in (0, 1, 2, 3, 0)]
        assert right == [(gf, gs), (gs, -gf), (-gf, -gs), (-gs, gf), (gf, gs)]
        left = [GOAL.goal_offset(10, 10, h, gx, gy) for h in (0, 3, 2, 1, 0)]
        assert left == [(gf, gs), (-gs, gf), (-gf, -gs), (gs, -gf), (gf, gs)]
    lay = _layout(12, 5)
    m = GOAL.HostGoalMaze(MazeConfig([lay], goal_sense=True, **FP_KW), 0, 1, seed=4)
    gf, gs, d = m.sense()
    assert (gf, gs) != (0, 0)
    for action, want in ((1, [(gs, -gf), (-gf, -gs), (-gs, gf), (gf, gs)]), (0, [(-gs, gf), (-gf, -gs), (gs, -gf), (gf, gs)])):
        for k in range(4):
            _, r, _, _ = m.process(action)
            assert m.sense() == want[k] + (d,) and r == 0
            np.testing.assert_array_equal(m.last_state["objective"], [want[k][0] / 32.0, want[k][1] / 32.0, d / 512.0])
            assert m.last_state["objective"].dtype == np.float64


def test_static_fields_and_shaped_rewards_over_random_layouts():
    up = down = goals = 0
    for N in SIZES:
        rs = np.random.RandomState(N)
        conf = MazeConfig([MM.random_layout(N, rs, marks="A" * 4) for _ in range(3)], max_episode_steps=30,
                          goal_sense=True, progress_reward=3, goal_reward=10, **FP_KW)
        models = GOAL.host_batch(conf, 6, seed=N)
        for step in range(60):
            for m in models:
                np.testing.assert_array_equal(conf.distance_field(m.layout, m.goal_cell), m.distance_field())
                free = ~conf.walls[m.layout]
                assert ((m.distance_field().reshape(-1) != GOAL.NO_PATH) == free).all()      # connected: all reached
                d0, apples = m.distance(), m.apples_total
                a = rs.randint(0, 4)
                closer = [k for k in (2, 3) if m.dist[m.move(k)[1] * N + m.move(k)[0]] < d0]
                if closer and rs.uniform() < 0.5:          # half the steps head for the goal, so that some get there
                    a = closer[0]
                _, r, t, _ = m.process(a)
                base = 10 if m.at_goal else 1 if m.apples_total > apples else -1 if m.hit else 0
                assert r == base + 3 * (m.d_before - m.d_after) and m.d_before == d0
                assert abs(m.d_before - m.d_after) <= 1 and abs(r) <= conf.reward_bound
                up += m.d_after > m.d_before
                down += m.d_after < m.d_before
                goals += m.at_goal
                if m.at_goal:
                    assert r == 13 and m.d_after == 0
                if t:
                    m.reset()
    assert up and down and goals


def test_generated_field_matches_bfs_on_generated_layout():
    for N, styled in ((7, False), (12, True), (21, False), (14, True)):
        kw = dict(wall_styles=[(9, 8, 7, 6), (1, 2, 3, 4)], gen_landmark_density=64) if styled else {}
        conf = gen_config(N, gen_loops=2, gen_apples=3, goal_sense=True, progress_reward=1, **kw)
        seed = 77 + N
        for g, m in enumerate(GOAL.host_batch(conf, 3, seed=seed)):
            for ep in range(3):
                assert m.episode == ep
                lay = conf.generated_layout(seed, g, ep)
                np.testing.assert_array_equal(conf.distance_field(lay, m.goal_cell), m.distance_field())
                rec = m.actor_record()
                assert len(rec) == conf.record_words
                np.testing.assert_array_equal(rec[-GOAL.dist_words(N):], GOAL.field_words(N, m.dist))
                assert list(rec[5:8]) == list(m.sense()) and m.distance() >= 1
                m.reset()


# ---- the entry -------------------------------------------------------------------------------------------------------------
def test_objective_entry_refuses_bad_arguments_without_launch():
    """-EINVAL on the host, so these fake device pointers never reach a kernel."""
    from unreal_amd.build import build_library
    from unreal_amd import _lib
    build_library(verbose=False)
    L = _lib.lib()
    dev = 1 << 20
    fn = L._fn["unreal_maze_objective"]
    # (B, H1, count, records, record_words, r_objective, next_lar, lar_ld, lar_col0)
    for args in ([0, 3, dev, dev, 33, dev, None, 0, 0],            # B <= 0
                 [-1, 3, dev, dev, 33, dev, None, 0, 0],
                 [4, 0, dev, dev, 33, dev, None, 0, 0],            # H1 <= 0
                 [4, 3, dev, dev, 7, dev, None, 0, 0],             # a record shorter than the navigation words
                 [4, 3, None, dev, 33, dev, None, 0, 0],           # no count
                 [4, 3, dev, None, 33, dev, None, 0, 0],           # no records
                 [4, 3, dev, dev, 33, None, None, 0, 0],           # no ring
                 [4, 3, dev, dev, 33, dev, dev, 263, 261],         # the three columns do not fit the row
                 [4, 3, dev, dev, 33, dev, dev, 0, 0],
                 [4, 3, dev, dev, 33, dev, dev, 264, -1]):
        assert fn(*args, None) == -22, args
    with pytest.raises(_lib.UnrealLibError):
        L.call("unreal_maze_objective", 0, 3, dev, dev, 33, dev, None, 0, 0, None)
