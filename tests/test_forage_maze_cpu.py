"""Foraging first-person mazes without a GPU: MazeConfig's validation, the block words with and without
the options, the reward bound, generated layouts against the ranking rule, the goal-less start draw, and the record
widths and view ids against the header."""
import os
import re
import zlib

import numpy as np
import pytest

try:
    import forage_maze_model as FM
    import maze_model as MM
except ImportError:            # imported as tests.<module>
    from tests import forage_maze_model as FM
    from tests import maze_model as MM

from unreal_amd.environment.maze_environment import MazeConfig, _philox_words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (7, 12, 14, 21)
FP_KW = dict(random_start=True, random_goal=True, view="first_person")
NG_KW = dict(random_start=True, view="first_person", no_goal=True, max_episode_steps=50)
YELLOW, PINK = (255, 255, 0), (255, 0, 255)
LEMON, MELON = (-1, YELLOW, False), (20, PINK, True)
SEED = 0x1234567890


def _layout(N=7, seed=0, marks=""):
    return MM.random_layout(N, np.random.RandomState(seed), marks=marks)


def gen_config(N, **kw):
    return MazeConfig(None, generate=N, **dict(FP_KW, **kw))


# ---- surface -----------------------------------------------------------------------------------------------------------
def test_pickups_validation():
    lay = _layout(marks="ABC")
    ok = MazeConfig([lay], pickups=[LEMON, MELON], **FP_KW)
    assert ok.forage and ok.nav and ok.pickups == [LEMON, MELON] and not ok.no_goal
    assert not MazeConfig([_layout()], **FP_KW).forage
    assert MazeConfig([_layout(marks="B")], pickups=[(np.int32(3), np.array([1, 2, 3]), np.bool_(True))], **FP_KW).pickups == \
        [(3, (1, 2, 3), True)]
    bad_lists = [[], [LEMON] * 4, "B", 3, [LEMON, None], [(1, YELLOW)], [(1, YELLOW, True, 0)]]
    bad_rewards = [True, 1.0, 0.5, "1", None, 101, -101, np.float32(1)]
    bad_colours = [(1, 2), (1, 2, 3, 4), (256, 0, 0), (-1, 0, 0), (1.0, 2, 3), (True, 2, 3), "abc", 5]
    bad_ends = [0, 1, None, "True"]
    for bad in bad_lists:
        with pytest.raises(ValueError):
            MazeConfig([lay], pickups=bad, **FP_KW)
    for bad in bad_rewards:
        with pytest.raises(ValueError):
            MazeConfig([lay], pickups=[(bad, YELLOW, False)] * 2, **FP_KW)
    for bad in bad_colours:
        with pytest.raises(ValueError):
            MazeConfig([lay], pickups=[(1, bad, False)] * 2, **FP_KW)
    for bad in bad_ends:
        with pytest.raises(ValueError):
            MazeConfig([lay], pickups=[(1, YELLOW, bad)] * 2, **FP_KW)
    for good in (-100, 100, 0):
        assert MazeConfig([lay], pickups=[(good, YELLOW, False)] * 2, **FP_KW).pickups[0][0] == good
    with pytest.raises(ValueError):                      # 'C' is kind 2; one kind given
        MazeConfig([lay], pickups=[LEMON], **FP_KW)
    with pytest.raises(ValueError):                      # letters without pickups
        MazeConfig([lay], **FP_KW)
    with pytest.raises(ValueError):                      # 'D' beyond two kinds
        MazeConfig([_layout(marks="D")], pickups=[LEMON, MELON], **FP_KW)
    with pytest.raises(ValueError):                      # first person only
        MazeConfig([lay], random_start=True, random_goal=True, pickups=[LEMON, MELON])
    with pytest.raises(ValueError):
        MazeConfig([_layout()], random_start=True, random_goal=True, view="top_down", pickups=[LEMON])
    with pytest.raises(ValueError):                      # words 5..7 cannot serve both
        MazeConfig([lay], pickups=[LEMON, MELON], goal_sense=True, **FP_KW)
    # at most 64 pickups of all kinds together
    assert MazeConfig([_layout(21, 1, "A" * 30 + "B" * 34)], pickups=[LEMON], **FP_KW).forage
    with pytest.raises(ValueError):
        MazeConfig([_layout(21, 1, "A" * 31 + "B" * 34)], pickups=[LEMON], **FP_KW)
    with pytest.raises(ValueError):
        MazeConfig([_layout(21, 1, "B" * 65)], pickups=[LEMON], **FP_KW)


def test_gen_pickups_validation():
    ok = gen_config(7, pickups=[LEMON, MELON], gen_apples=6, gen_pickups=(6, 4))
    assert ok.gen_pickups == (6, 4) and ok.forage and ok.nav
    assert gen_config(7, pickups=[LEMON], gen_pickups=[np.int64(0)]).gen_pickups == (0,)
    assert gen_config(21, pickups=[LEMON], gen_apples=32, gen_pickups=(32,)).gen_pickups == (32,)
    with pytest.raises(ValueError):                      # 17 > 16 rooms
        gen_config(7, pickups=[LEMON, MELON], gen_apples=6, gen_pickups=(6, 5))
    with pytest.raises(ValueError):                      # 65 > 64 bits
        gen_config(21, pickups=[LEMON], gen_apples=32, gen_pickups=(33,))
    with pytest.raises(ValueError):                      # needs pickups
        gen_config(7, gen_pickups=(1,))
    with pytest.raises(ValueError):                      # needs generate
        MazeConfig([_layout(marks="B")], pickups=[LEMON], gen_pickups=(1,), **FP_KW)
    for bad in ((1,), (1, 2, 3), (1, -1), (1, 1.0), (True, 1), "12", 3):
        with pytest.raises(ValueError):
            gen_config(7, pickups=[LEMON, MELON], gen_pickups=bad)
    with pytest.raises(ValueError):
        MazeConfig(None, generate=7, random_start=True, random_goal=True, view="top_down", pickups=[LEMON], gen_pickups=(1,))


def test_no_goal_validation():
    lay = _layout(marks="SA")
    ok = MazeConfig([lay], **NG_KW)
    assert ok.no_goal and ok.forage and ok.nav and ok.pickups is None and ok.goal == [-1]
    assert MazeConfig([lay], view="first_person", no_goal=True, max_episode_steps=5).start == [lay.index("S")]
    with pytest.raises(ValueError):                      # layouts must hold no G
        MazeConfig([_layout(marks="SG")], **NG_KW)
    with pytest.raises(ValueError):                      # there is no goal to draw
        MazeConfig([lay], random_goal=True, **NG_KW)
    with pytest.raises(ValueError):                      # only the time-out ends every episode
        MazeConfig([lay], random_start=True, view="first_person", no_goal=True)
    for kw in (dict(show_goal=True), dict(goal_respawn=True), dict(goal_sense=True), dict(goal_reward=2),
               dict(goal_reward=0)):
        with pytest.raises(ValueError):
            MazeConfig([lay], **dict(NG_KW, **kw))
    with pytest.raises(ValueError):                      # first person only
        MazeConfig([lay], random_start=True, no_goal=True, max_episode_steps=50)
    for bad in (1, 0, None, "yes"):
        with pytest.raises(ValueError):
            MazeConfig([lay], **dict(NG_KW, no_goal=bad))
    with pytest.raises(ValueError):                      # without random_start a layout needs its S
        MazeConfig([_layout(marks="A")], view="first_person", no_goal=True, max_episode_steps=5)
    # generated: random_start alone
    g = MazeConfig(None, generate=12, gen_apples=3, **NG_KW)
    assert g.no_goal and not g.random_goal and g.forage
    with pytest.raises(ValueError):
        MazeConfig(None, generate=12, view="first_person", no_goal=True, max_episode_steps=50)
    with pytest.raises(ValueError):                      # a generated maze with a goal still needs random_goal
        MazeConfig(None, generate=12, random_start=True, view="first_person", max_episode_steps=50)


def test_register_passes_the_options_on():
    from unreal_amd.environment.environment import Environment
    try:
        Environment.register_maze_config("forage_cpu", [_layout(marks="SAB")], view="first_person", max_episode_steps=9,
                                         pickups=[LEMON], no_goal=True)
        Environment.register_maze_config("forage_cpu_gen", None, generate=7, random_start=True, view="first_person",
                                         max_episode_steps=9, gen_apples=2, pickups=[LEMON, MELON], gen_pickups=(3, 1),
                                         no_goal=True, action_set="lab")
        a, g = Environment.MAZE_CONFIG["forage_cpu"], Environment.MAZE_CONFIG["forage_cpu_gen"]
        assert a.forage and a.no_goal and a.pickups == [LEMON] and g.gen_pickups == (3, 1)
        assert Environment.get_action_size("maze", "forage_cpu_gen") == 6
        assert Environment.get_objective_size("maze", "forage_cpu") == 0
        with pytest.raises(ValueError):
            Environment.register_maze_config("forage_cpu_bad", [_layout(marks="SAB")], pickups=[LEMON])
        assert "forage_cpu_bad" not in Environment.MAZE_CONFIG
    finally:
        for name in ("forage_cpu", "forage_cpu_gen"):
            Environment.MAZE_CONFIG.pop(name, None)


# ---- blocks ------------------------------------------------------------------------------------------------------------
# (words, crc32 of the words' bytes) of blocks built with seed SEED before forage mazes existed
PINNED = {
    "reference": (75, 0x409AB8CC),
    "top_down_12": (332, 0x924FD022),
    "fp_plain_12": (170, 0x72959AFA),
    "nav_7": (148, 0x33C16D2A),
    "nav_apples_21": (540, 0x54026BFD),
    "gen_14": (16, 0x66C70BE5),
    "gen_styled_14": (32, 0x816E40A5),
    "styled_7": (98, 0x5D9919B2),
    "sense_12": (243, 0x4BFCACCB),
}


def _pinned_configs():
    return {
        "reference": MazeConfig.reference(),
        "top_down_12": MazeConfig([_layout(12, 3, "SG"), _layout(12, 4, "SG")], show_goal=True, max_episode_steps=50),
        "fp_plain_12": MazeConfig([_layout(12, 3, "SG")], view="first_person"),
        "nav_7": MazeConfig([_layout(7, 1, "SGAAAA")], view="first_person", goal_reward=10, apple_reward=2, hit_reward=-3,
                            goal_respawn=True, max_episode_steps=30, action_set="lab"),
        "nav_apples_21": MazeConfig([_layout(21, 2, "A" * 64)], **FP_KW),
        "gen_14": gen_config(14, gen_loops=3, gen_apples=5),
        "gen_styled_14": gen_config(14, gen_loops=3, gen_apples=5, wall_styles=[(1, 2, 3, 4)], gen_landmark_density=9),
        "styled_7": MazeConfig([_layout(7, 5, "SG").replace("+", "2", 3)], view="first_person",
                               wall_styles=[(200, 100, 50, 0xAA), (0, 255, 0, 0)]),
        "sense_12": MazeConfig([_layout(12, 3, "SG")], view="first_person", goal_reward=5, goal_sense=True,
                               progress_reward=-4),
    }


def test_blocks_without_the_options_are_what_they_were():
    """Length and CRC of nine blocks recorded before the options existed, and a few words by value."""
    for name, cfg in _pinned_configs().items():
        b = cfg.block(SEED)
        assert not cfg.forage and not b[2] & 128, name
        assert (len(b), zlib.crc32(b.tobytes())) == PINNED[name], name
    ref = MazeConfig.reference().block(0)
    assert list(ref[:8]) == [7, 1, 0, 0, 0, 0, 67, 0]
    assert list(ref[8 + 14:8 + 18]) == [14, 6, 34, 5] and len(ref) == 75      # G is the sixth free cell
    nav = _pinned_configs()["nav_7"].block(SEED)
    assert nav[2] == 8 and list(nav[8 + 67:8 + 67 + 8]) == [10, 2, -3, 3, 0, 0, 0, 0] and nav[8 + 67 + 8] == 4
    assert list(nav[4:6]) == [0x34567890, 0x12]
    gen = _pinned_configs()["gen_14"].block(SEED)
    assert list(gen[:4]) == [14, 0, 1 | 2 | 8 | 16, 0] and list(gen[8:16]) == [1, 1, -1, 0, 3, 5, 0, 0]
    # the new arguments at their defaults change nothing
    lay = _layout(7, 1, "SGAAAA")
    np.testing.assert_array_equal(MazeConfig([lay], view="first_person", pickups=None, gen_pickups=None, no_goal=False).block(3),
                                  MazeConfig([lay], view="first_person").block(3))


def test_forage_block_words():
    """Flag 128 with the navigation flag, the 16 section words after everything else, and the packed apple entries; the
    rest of the block is the navigation block's."""
    lay = list(_layout(7, 1, "SG"))
    free = [c for c, ch in enumerate(lay) if ch == "-"]
    for c, ch in zip(free[:5], "BACAD"):
        lay[c] = ch
    lay = "".join(lay)
    kinds = [LEMON, (5, (1, 2, 3), False), MELON]
    cfg = MazeConfig([lay], view="first_person", pickups=kinds, goal_reward=7)
    b = cfg.block(SEED)
    base = MazeConfig([lay.translate({ord(ch): "A" for ch in "BCD"})], view="first_person", goal_reward=7)
    nb = base.block(SEED)
    assert b[2] == nb[2] | 128 == 8 | 128 and len(b) == len(nb) + 16
    ext = 8 + 67
    assert list(b[ext:ext + 8]) == [7, 1, -1, 0, 0, 0, 0, 0]
    assert b[ext + 8] == 5 and list(b[ext + 9:ext + 14]) == [c | k << 16 for c, k in zip(free[:5], (1, 0, 2, 0, 3))]
    assert list(nb[ext + 9:ext + 14]) == free[:5] and not b[ext + 14:ext + 8 + 65].any()
    same = np.ones(len(nb), dtype=bool)
    same[[2] + list(range(ext + 9, ext + 14))] = False
    np.testing.assert_array_equal(b[:len(nb)][same], nb[same])
    sec = list(b[-16:])
    assert sec == [3, 0, 0, 0, -1, 5, 20, 0, 255 | 255 << 8, 1 | 2 << 8 | 3 << 16, 255 | 255 << 16 | 1 << 24, 0, 0, 0, 0, 0]
    np.testing.assert_array_equal(b[-16:], FM.forage_section(cfg))
    assert cfg.record_words == 8 and list(cfg.apples[0]) == [free[1], free[3]]
    # no goal, one kind: mode 1, G = -1 in the layout record
    ng = MazeConfig([lay.replace("G", "-").replace("C", "-").replace("D", "-")], view="first_person", no_goal=True,
                    max_episode_steps=9, pickups=[LEMON])
    nb = ng.block(SEED)
    assert nb[2] == 8 | 128 and nb[3] == 9 and nb[8 + 15] == -1 and nb[8 + 17] == -1 and nb[8 + 14] == lay.index("S")
    assert list(nb[-16:]) == [1, 1, 0, 0, -1, 0, 0, 0, 255 | 255 << 8, 0, 0, 0, 0, 0, 0, 0]
    # no_goal alone: no kinds, the apples are kind 0
    alone = MazeConfig([lay.replace("G", "-").translate({ord(ch): "A" for ch in "BCD"})], view="first_person", no_goal=True,
                       max_episode_steps=9)
    ab = alone.block(SEED)
    assert ab[2] == 8 | 128 and list(ab[-16:]) == [0, 1] + [0] * 14 and list(ab[ext + 9:ext + 14]) == free[:5]


def test_forage_section_follows_the_style_section():
    styles = [(200, 100, 50, 0xAA), (0, 255, 0, 0)]
    lay = _layout(12, 5, "SGAB").replace("+", "2", 3)
    plain = MazeConfig([lay.replace("B", "A")] * 2, view="first_person", wall_styles=styles).block(SEED)
    b = MazeConfig([lay] * 2, view="first_person", wall_styles=styles, pickups=[MELON]).block(SEED)
    assert b[2] == 8 | 32 | 128 and len(b) == len(plain) + 16
    sw = (144 + 7) // 8
    np.testing.assert_array_equal(b[-16 - 2 * sw:-16], plain[-2 * sw:])           # the nibble words, then the section
    assert list(b[-16:]) == [1, 0, 0, 0, 20, 0, 0, 0, 255 | 255 << 16 | 1 << 24] + [0] * 7
    # generated + styled: header, 8 navigation words, 16 style words, 16 forage words
    g = gen_config(14, gen_loops=3, gen_apples=5, wall_styles=styles, gen_landmark_density=9, pickups=[LEMON, MELON],
                   gen_pickups=(4, 2))
    gb = g.block(SEED)
    assert len(gb) == 8 + 8 + 16 + 16 and gb[2] == 1 | 2 | 8 | 16 | 32 | 128
    assert list(gb[8:16]) == [1, 1, -1, 0, 3, 5, 0, 0] and list(gb[16:18]) == [2, 9]
    assert list(gb[-16:]) == [2, 0, 0, 0, -1, 20, 0, 0, 255 | 255 << 8, 255 | 255 << 16 | 1 << 24, 0, 0, 4, 2, 0, 0]
    # gen_pickups all zero: the forage flag and section aside, the generated block is the plain one
    z = gen_config(14, gen_loops=3, gen_apples=5, pickups=[LEMON], gen_pickups=(0,)).block(SEED)
    p = gen_config(14, gen_loops=3, gen_apples=5).block(SEED)
    assert z[2] == p[2] | 128 and list(z[3:16]) == list(p[3:]) and list(z[-4:]) == [0, 0, 0, 0]


def test_reward_bound():
    lay = _layout(marks="SABC")
    rb = lambda **kw: MazeConfig([lay], **dict(FP_KW, **kw)).reward_bound
    assert MazeConfig([_layout()], **FP_KW).reward_bound == 1
    assert rb(pickups=[LEMON, (1, PINK, True)]) == 1
    assert rb(pickups=[LEMON, MELON]) == 20 and rb(pickups=[(-30, YELLOW, False), MELON]) == 30
    assert rb(pickups=[LEMON, MELON], goal_reward=50) == 50
    ng = lambda **kw: MazeConfig([lay], **dict(NG_KW, **kw)).reward_bound
    assert ng(pickups=[LEMON, (1, PINK, True)]) == 1
    assert ng(pickups=[LEMON, (1, PINK, True)], apple_reward=0, hit_reward=0) == 1
    assert ng(pickups=[(0, YELLOW, False), (0, PINK, True)], apple_reward=0, hit_reward=0) == 0     # goal_reward left out
    assert ng(pickups=[LEMON, (2, PINK, True)]) == 2 and ng(pickups=[LEMON, (1, PINK, True)], hit_reward=-4) == 4


# ---- generated layouts -------------------------------------------------------------------------------------------------
def test_generated_layout_letters_follow_the_ranking_rule():
    for N, counts in ((7, (4, 4, 4, 4)), (12, (3, 0, 5, 1)), (14, (0, 2, 0, 3)), (21, (24, 20, 12, 8))):
        cfg = MazeConfig(None, generate=N, gen_loops=2, gen_apples=counts[0], pickups=[LEMON, (5, (1, 2, 3), False), MELON],
                         gen_pickups=counts[1:], **NG_KW)
        R = (N + 1) // 2
        for g, ep in ((0, 0), (5, 3), (199, 17)):
            s = cfg.generated_layout(SEED, g, ep)
            w = _philox_words(SEED, g, ep, MazeConfig.APPLE_STREAM, R * R)
            ranked = sorted(range(R * R), key=lambda r: (int(w[r]) << 8) | r)
            want, first = {}, 0
            for kind, n in enumerate(counts):
                for r in ranked[first:first + n]:
                    want[2 * (r // R) * N + 2 * (r % R)] = "ABCD"[kind]
                first += n
            assert {c: ch for c, ch in enumerate(s) if ch in "ABCD"} == want, (N, g, ep)
            cells, kinds = FM.generate_pickups(N, counts, SEED, g, ep)
            assert [(c, "ABCD"[k]) for c, k in zip(cells, kinds)] == sorted(want.items())
            # the walls are those of the same config without pickups
            plain = MazeConfig(None, generate=N, gen_loops=2, **FP_KW).generated_layout(SEED, g, ep)
            assert s.translate({ord(ch): "-" for ch in "ABCD"}) == plain
            lc = cfg.layout_config(s)
            assert lc.forage and lc.no_goal and lc.pickups == cfg.pickups
            assert list(lc.pickup_cells[0]) == cells and list(lc.pickup_kinds[0]) == kinds
    # gen_pickups all zero: the layout of the same config without the option
    a = gen_config(12, gen_loops=1, gen_apples=7, pickups=[LEMON], gen_pickups=(0,)).generated_layout(SEED, 3, 4)
    assert a == gen_config(12, gen_loops=1, gen_apples=7).generated_layout(SEED, 3, 4)


def test_no_goal_start_draw_by_hand():
    """free cell number (word 1 of the reset draw) % n_free; word 0 is unused; the heading is word 2 mod 4."""
    lay = _layout(7, 2, "SAB")
    cfg = MazeConfig([lay], pickups=[LEMON], **NG_KW)
    free = [c for c, ch in enumerate(lay) if ch != "+"]
    assert list(cfg.free[0]) == free
    for g, ep in ((0, 0), (3, 1), (77, 12)):
        w = _philox_words(SEED, g, ep, 0x4D415A45, 4)                # the reset stream, counter word 3 = 0
        m = FM.HostForageMaze(cfg, g, 100, seed=SEED)
        while m.episode < ep:
            m.reset()
        assert m.y * 7 + m.x == free[int(w[1]) % len(free)] and m.h == int(w[2]) % 4 and (m.gx, m.gy) == (-1, -1)
    # the S cell without random_start
    m = FM.HostForageMaze(MazeConfig([lay], view="first_person", no_goal=True, max_episode_steps=5, pickups=[LEMON]), 0, 1)
    assert m.y * 7 + m.x == lay.index("S")
    starts = set()
    for g in range(200):
        m = FM.HostForageMaze(cfg, g, 200, seed=1)
        starts.add(m.y * 7 + m.x)
    assert starts == set(free)                                         # every free cell, pickups' and S included


def test_host_model_semantics_on_a_corridor():
    """One corridor S A B C: +1, -1, then the melon's +20 ends the episode; a second visit pays nothing; the totals run on."""
    rows = ["+++++++", "+++++++", "+++++++", "SAB-C--", "+++++++", "+++++++", "+++++++"]
    cfg = MazeConfig([rows], view="first_person", start_heading=0, no_goal=True, max_episode_steps=9, hit_reward=-3,
                     pickups=[LEMON, MELON])
    m = FM.HostForageMaze(cfg, 0, 1)
    out = [m.process(a)[1:3] for a in (2, 3, 2, 2, 3, 2, 2)]       # A, back, A again (gone), B, back, B again, free
    assert out == [(1, False), (0, False), (0, False), (-1, False), (0, False), (0, False), (0, False)]
    assert m.process(2)[1:3] == (20, True) and m.ended_by_pickup and not m.timed_out
    assert m.record() == [0, 0b111, 0, 0, 1, 1, 1, 0]
    m.reset()
    assert m.record() == [0, 0, 0, 0, 1, 1, 1, 0] and m.episode == 1
    assert m.process(3)[1:3] == (-3, False)                            # a hit
    for _ in range(7):
        assert m.process(0)[1:3] == (0, False)
    assert m.process(0)[1:3] == (0, True) and m.timed_out              # the time-out at step 9
    # the frame shows each kind's colour, and a collected pickup is gone
    m.reset()
    seen = lambda colour: bool((m.frame == np.array(colour, np.uint8)).all(2).any())
    assert seen((40, 255, 40)) and seen(YELLOW) and seen(PINK)
    m.process(2); m.process(2)
    assert not seen((40, 255, 40)) and not seen(YELLOW) and seen(PINK)


# ---- header ------------------------------------------------------------------------------------------------------------
def test_record_widths_and_view_ids_match_the_header():
    from unreal_amd import ops
    src = open(os.path.join(ROOT, "include", "unreal_hip.h")).read()
    macros = dict(re.findall(r"#define (UNREAL_MAZE_\w+)\(N\) (.+)", src))

    def expand(name, N):
        expr = macros[name]
        for other in macros:
            expr = re.sub(other + r"\(N\)", lambda m, o=other: "(%d)" % expand(o, N), expr)
        return eval(expr.replace("/", "//").replace("(N)", "(%d)" % N))
    nav = int(re.search(r"#define UNREAL_MAZE_NAV_RECORD (\d+)", src).group(1))
    for N in SIZES:
        assert MazeConfig([_layout(N, 0, "SAB")], pickups=[LEMON], **NG_KW).record_words == nav == ops.NAV_RECORD == 8
        g = MazeConfig(None, generate=N, gen_apples=2, pickups=[LEMON], gen_pickups=(2,), **NG_KW)
        assert g.record_words == expand("UNREAL_MAZE_GEN_RECORD", N) == ops.gen_record_words(N)
        gs = MazeConfig(None, generate=N, gen_apples=2, pickups=[LEMON], gen_pickups=(2,), wall_styles=[(1, 2, 3, 4)], **NG_KW)
        assert gs.record_words == expand("UNREAL_MAZE_GEN_STYLED_RECORD", N) == ops.gen_record_words(N, True)
    ids = dict((k, int(v)) for k, v in re.findall(r"#define (UNREAL_MAZE_[A-Z_]+) (\d+)\n", src))
    assert ids["UNREAL_MAZE_FIRST_PERSON_FORAGE"] == ops.MAZE_FIRST_PERSON_FORAGE == 5
    assert ids["UNREAL_MAZE_FIRST_PERSON_GENERATED_FORAGE"] == ops.MAZE_FIRST_PERSON_GENERATED_FORAGE == 6
    assert (ids["UNREAL_MAZE_TOP_DOWN"], ids["UNREAL_MAZE_FIRST_PERSON"], ids["UNREAL_MAZE_FIRST_PERSON_GENERATED"],
            ids["UNREAL_MAZE_FIRST_PERSON_SENSE"], ids["UNREAL_MAZE_FIRST_PERSON_GENERATED_SENSE"]) == \
        (ops.MAZE_TOP_DOWN, ops.MAZE_FIRST_PERSON, ops.MAZE_FIRST_PERSON_GENERATED, ops.MAZE_FIRST_PERSON_SENSE,
         ops.MAZE_FIRST_PERSON_GENERATED_SENSE) == (0, 1, 2, 3, 4)
    assert MazeConfig.FORAGE == FM.FORAGE_FLAG == 128 and MazeConfig.FORAGE_WORDS == FM.FORAGE_WORDS == 16
