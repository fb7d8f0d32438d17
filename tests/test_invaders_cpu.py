"""CPU tests of the device arcade's invaders game: config validation with the cross-game keywords in both
directions, the block by value, the header's constants, the entries' host check, and the rules on the host model of
tests/invaders_model.py, worked by hand; then the events of the traces tests/test_invaders_gpu.py compares."""
import os
import re

import numpy as np
import pytest

try:
    import arcade_model as AM
    import invaders_model as IM
    from philox_model import philox4x32_10_raw as philox_ref
except ImportError:            # imported as tests.<module>
    from tests import arcade_model as AM
    from tests import invaders_model as IM
    from tests.philox_model import philox4x32_10_raw as philox_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOOP, FIRE, RIGHT, LEFT = AM.NOOP, AM.FIRE, AM.RIGHT, AM.LEFT


def _conf(**kw):
    from unreal_amd.environment.arcade_environment import ArcadeConfig
    kw.setdefault("game", "invaders")
    return ArcadeConfig(**kw)


def _model(seed=0, g=0, **kw):
    return IM.HostInvaders(_conf(**kw), g, seed)


def _count(frame, colour):
    return int((frame == colour).all(2).sum())


# ---- config ---------------------------------------------------------------------------------------------------------------
INV_BAD = [dict(alien_rows=0), dict(alien_rows=5), dict(alien_rows=True), dict(alien_rows=3.0), dict(alien_rows="3"),
           dict(alien_rewards=(1, 1)), dict(alien_rewards=(1, 1, 101)), dict(alien_rewards=(1, 1, -1)),
           dict(alien_rewards=(1, 1, True)), dict(alien_rewards=(1, 1, 1.0)), dict(alien_rewards="111"), dict(alien_rewards=1),
           dict(march_period=0), dict(march_period=17), dict(march_period=True), dict(march_period=4.0),
           dict(descend=0), dict(descend=9), dict(descend=False), dict(descend=4.0),
           dict(bomb_period=0), dict(bomb_period=65), dict(bomb_period=True), dict(bomb_period=12.0),
           dict(bomb_speed=0), dict(bomb_speed=5), dict(bomb_speed=True), dict(bomb_speed=1.0),
           dict(lives=0), dict(lives=6), dict(lives=True), dict(lives=3.0),
           dict(life_reward=1), dict(life_reward=-101), dict(life_reward=False), dict(life_reward=-1.0),
           # the shared settings keep Breakout's ranges
           dict(paddle_width=2), dict(paddle_width=26), dict(paddle_width=11), dict(paddle_width=True),
           dict(paddle_speed=0), dict(paddle_speed=9), dict(paddle_speed=1.0),
           dict(ball_speed=0), dict(ball_speed=5), dict(ball_speed=True),
           dict(serve_wait=-1), dict(serve_wait=256), dict(serve_wait=8.0),
           dict(max_episode_steps=0), dict(max_episode_steps=2 ** 31), dict(max_episode_steps=None),
           dict(action_repeat=0), dict(action_repeat=9), dict(action_repeat=True),
           # no paddle returns a ball here
           dict(return_reward=1), dict(return_reward=100), dict(return_reward=-1), dict(return_reward=False),
           dict(return_reward=0.0),
           # Breakout's and the duel's own settings, even at their defaults
           dict(rows=6), dict(rows=3), dict(row_rewards=(1,) * 3), dict(points=5), dict(opponent_width=12),
           dict(opponent_speed=2), dict(win_reward=1), dict(lose_reward=-1)]
OWN = [dict(alien_rows=3), dict(alien_rewards=(1, 1, 1)), dict(march_period=4), dict(descend=4), dict(bomb_period=12),
       dict(bomb_speed=1)]
BAD = [dict(game="invaders", **kw) for kw in INV_BAD] + \
      [dict(game="pong"), dict(game="Invaders"), dict(game=5), dict(game="Duel"), dict(game=3)] + \
      [dict(game=g, **kw) for g in ("breakout", "duel") for kw in OWN] + OWN + \
      [dict(game="duel", lives=3), dict(game="duel", life_reward=0)]          # shared by Breakout and invaders only


@pytest.mark.parametrize("kw", BAD, ids=[repr(sorted(k.items())) for k in BAD])
def test_a_setting_outside_its_range_or_of_another_game_is_a_value_error(kw):
    from unreal_amd.environment.environment import Environment
    with pytest.raises(ValueError):
        Environment.register_arcade_config("invaders_bad", **kw)
    assert "invaders_bad" not in Environment.ARCADE_CONFIG


def test_the_edges_of_every_range_are_accepted_and_registered():
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.arcade_environment import ArcadeConfig, GAMES, GAME_IDS, GAME_SETTINGS
    from unreal_amd import ops
    # GAMES stays the dictionary tests/test_duel_cpu.py pins; GAME_IDS is every game
    assert GAME_IDS == {"breakout": 1, "duel": 3, "invaders": 5} and ops.ARCADE_INVADERS == 5
    assert GAMES == {"breakout": 1, "duel": 3} and sorted(GAME_SETTINGS) == sorted(GAME_IDS)
    assert GAME_SETTINGS["invaders"] == dict(alien_rows=3, alien_rewards=None, lives=3, life_reward=0, march_period=4,
                                             descend=4, bomb_period=12, bomb_speed=1)
    for kw in (dict(alien_rows=1, alien_rewards=(0,), lives=1, life_reward=-100, march_period=1, descend=1, bomb_period=1,
                    bomb_speed=1, paddle_width=4, paddle_speed=1, ball_speed=1, serve_wait=0, max_episode_steps=1,
                    action_repeat=1, return_reward=0),
               dict(alien_rows=4, alien_rewards=(100,) * 4, lives=5, life_reward=0, march_period=16, descend=8,
                    bomb_period=64, bomb_speed=4, paddle_width=24, paddle_speed=8, ball_speed=4, serve_wait=255,
                    max_episode_steps=2 ** 31 - 1, action_repeat=8),
               dict(alien_rows=np.int64(2), alien_rewards=[np.int32(3), 4], descend=np.int32(6))):
        ArcadeConfig(game="invaders", **kw)
    try:
        Environment.register_arcade_config("invaders_ok", game="invaders")
        conf = Environment.ARCADE_CONFIG["invaders_ok"]
        assert isinstance(conf, ArcadeConfig) and conf.game == "invaders" and conf.action_size == 4
        assert (conf.alien_rows, conf.alien_rewards, conf.lives, conf.life_reward, conf.march_period, conf.descend,
                conf.bomb_period, conf.bomb_speed, conf.paddle_width, conf.paddle_speed, conf.ball_speed, conf.serve_wait,
                conf.max_episode_steps, conf.action_repeat, conf.return_reward) == \
            (3, (1, 1, 1), 3, 0, 4, 4, 12, 1, 12, 3, 2, 8, 5000, 1, 0)
        assert not hasattr(conf, "rows") and not hasattr(conf, "points")
        assert Environment.get_action_size("arcade", "invaders_ok") == 4
        assert Environment.get_objective_size("arcade", "invaders_ok") == 0
        # lives and life_reward stay Breakout's too, and the other games' defaults are untouched
        conf = ArcadeConfig(lives=2, life_reward=-3)
        assert (conf.game, conf.rows, conf.lives, conf.life_reward) == ("breakout", 6, 2, -3) and not hasattr(conf, "alien_rows")
        assert ArcadeConfig(game="breakout", return_reward=100).return_reward == 100
        assert not hasattr(ArcadeConfig(game="duel"), "lives")
    finally:
        Environment.ARCADE_CONFIG.pop("invaders_ok", None)


def test_the_block_by_value():
    c = _conf(alien_rows=2, alien_rewards=(9, 4), max_episode_steps=123456, paddle_width=16, paddle_speed=5, ball_speed=3,
              lives=4, serve_wait=20, life_reward=-9, march_period=7, descend=6, bomb_period=33, bomb_speed=2, action_repeat=4)
    b = c.block(0xFEDCBA9876543210)
    assert b.dtype == np.int32 and b.shape == (24,)
    want = [5, 3, 2, 123456, 0x76543210, np.int32(-0x01234568), 16, 5, 3, 4, 20, -9, 9, 4, 0, 0, 7, 6, 0, 33, 2, 0, 0, 0]
    assert b.tolist() == [int(w) for w in want]
    assert _conf().block(5).tolist() == [5, 0, 3, 5000, 5, 0, 12, 3, 2, 3, 8, 0, 1, 1, 1, 0, 4, 4, 0, 12, 1, 0, 0, 0]
    # the other games' blocks are what they were
    assert _conf(game="breakout").block(5).tolist() == [1, 0, 6, 5000, 5, 0, 12, 3, 2, 3, 8, 0, 1, 1, 1, 1, 1, 1] + [0] * 6
    assert _conf(game="duel").block(5).tolist() == [3, 0, 5, 5000, 5, 0, 12, 3, 2, 12, 8, -1, 1, 2] + [0] * 10


def test_header_constants_and_documents():
    from unreal_amd import ops
    src = open(os.path.join(ROOT, "include", "unreal_hip.h")).read()
    defs = dict(re.findall(r"#define (UNREAL_ARCADE_\w+) (\w+)", src))
    assert int(defs["UNREAL_ARCADE_INVADERS"]) == ops.ARCADE_INVADERS == 5
    assert int(defs["UNREAL_ARCADE_BREAKOUT"]) == 1 and int(defs["UNREAL_ARCADE_DUEL"]) == 3
    assert int(defs["UNREAL_ARCADE_CFG_WORDS"]) == ops.ARCADE_CFG_WORDS == 24 == len(_conf().block(0))
    assert int(defs["UNREAL_ARCADE_RECORD"]) == ops.ARCADE_RECORD == 16 == len(_model().record())
    assert int(defs["UNREAL_ARCADE_BOMB_STREAM"], 16) == ops.ARCADE_BOMB_STREAM == IM.BOMB_STREAM
    assert IM.BOMB_STREAM != AM.SERVE_STREAM
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("UNREAL_ARCADE_INVADERS", "alien_rows", "bomb_period"):
        assert word in text and word in src, word
    kernel = open(os.path.join(ROOT, "unreal_amd", "csrc", "arcade.hip")).read()
    assert "kArcadeInvaders = 5" in kernel and "0x%08Xu" % IM.BOMB_STREAM in kernel
    assert ("%du | %du << 8 | %du << 16" % IM.BOMB) in kernel


def test_entries_refuse_bad_arguments_without_a_launch():
    """Fake device pointers (the block is device memory the host check never reads: every game's calls pass the same
    check): the calls below are refused, so none reaches a kernel.  A = 6 stays refused with a third game."""
    from unreal_amd.build import build_library
    from unreal_amd import _lib
    build_library(verbose=False)
    f = _lib.lib()._fn
    dev = 1 << 20
    tail = [dev, 0, dev, dev, dev]                       # cfg, actor_base, ep_steps, episode, records
    reset = [4, 3, None, None, dev, dev, dev, dev]
    ring = [None] + [dev] * 10 + [None, None] + [dev] * 3
    step = [4, 3, dev, None] + ring + [1, 1]
    roll = [4, 3, dev] + ring + [dev] * 4 + [None, None, 0, 0, 4, 0]
    pol = [4, 3, dev, 256] + [dev] * 8 + ring + [dev] * 4 + [None, None, 0, 0, 4, 0]
    for t in ([None, 0, dev, dev, dev], [dev + 2, 0, dev, dev, dev], [dev, -1, dev, dev, dev], [dev, 0, dev, dev, None]):
        assert f["unreal_arcade_reset"](*reset, *t, None) == -22, t
        assert f["unreal_arcade_step"](*step, *t, None) == -22, t
        assert f["unreal_arcade_rollout_step"](*roll, *t, None) == -22, t
        assert f["unreal_arcade_policy_rollout_step"](*pol, *t, None) == -22, t
    for A in (3, 6, 18):
        assert f["unreal_arcade_rollout_step"](*roll[:-2], A, 0, *tail, None) == -22, A
        assert f["unreal_arcade_policy_rollout_step"](*pol[:-2], A, 0, *tail, None) == -22, A


# ---- the rules, by hand ------------------------------------------------------------------------------------------------------
def test_the_reset_state_and_record():
    m = _model()
    assert (m.px, m.sx, m.sy, m.gx, m.gy, m.dir, m.lives, m.mask) == (36, 0, 0, 10, 10, 1, 3, 0xFFFFFF)
    assert (m.march, m.bomb, m.grace, m.draw_index, m.bombs, m.totals, m.episode) == (0, 0, 8, 0, [None] * 3, [0, 0, 0], 0)
    assert m.record().tolist() == [36, 0, 0, 10, 10, 1, 3, 0xFFFFFF, 8 << 16, 0, 0, 0, 0, 0, 0, 0]
    m = _model(alien_rows=4)
    assert m.mask == 0xFFFFFFFF and m.record()[7] == -1
    m.march, m.bomb, m.grace, m.bombs = 15, 63, 256, [(81, 82), None, (2, 14)]
    assert m.record().tolist()[8:] == [15 | 63 << 8 | 256 << 16, 0, 0, 0, 0, 81 | 82 << 8, 0, 2 | 14 << 8]


def test_the_cannon_moves_and_is_clamped():
    m = _model(paddle_speed=8)
    seen = []
    for _ in range(6):
        m.process(RIGHT)
        seen.append(m.px)
    assert seen == [44, 52, 60, 68, 70, 70]               # 82 - 12
    m = _model(paddle_speed=8)
    seen = []
    for _ in range(6):
        m.process(LEFT)
        seen.append(m.px)
    assert seen == [28, 20, 12, 4, 2, 2]


def test_a_march_to_each_edge_with_descent_and_flip():
    m = _model(march_period=1, bomb_period=64)
    seen = []
    for _ in range(18):
        m.process(NOOP)
        seen.append((m.gx, m.gy, m.dir))
    assert seen[:5] == [(12, 10, 1), (14, 10, 1), (16, 10, 1), (18, 10, 1), (20, 10, 1)]
    assert seen[5] == (20, 14, -1) and "descent" in m.events | {"descent"}           # 22 > 20: down, no x move
    assert seen[6:15] == [(18 - 2 * k, 14, -1) for k in range(9)]
    assert seen[15] == (2, 18, 1) and seen[16] == (4, 18, 1)
    # every march_period ticks: the counter counts from 0 and the grid moves in the tick in which it reaches the period
    m = _model(march_period=4, descend=8)
    moves = []
    for k in range(12):
        m.process(NOOP)
        moves.append(m.gx)
        assert m.march == (k + 1) % 4
    assert moves == [10, 10, 10, 12, 12, 12, 12, 14, 14, 14, 14, 16]
    m.gx, m.march = 20, 3
    m.process(NOOP)
    assert (m.gx, m.gy, m.dir) == (20, 18, -1) and m.events == {"descent"}
    m.gy, m.gx, m.dir, m.march, m.lives = 80, 2, -1, 3, 0      # an ended game marches on; gy stops at 84
    m.process(NOOP)
    assert (m.gx, m.gy, m.dir) == (2, 84, 1)
    m.dir, m.march = -1, 3
    m.process(NOOP)
    assert m.gy == 84


def test_fire_a_hit_on_the_lowest_overlapping_bit_and_a_second_fire_ignored():
    # the shot starts at (px + w/2 - 1, 76) = (41, 76) and moves in the tick it is fired: ball_speed = 2 -> y 74
    m = _model(march_period=16, bomb_period=64, alien_rewards=(5, 3, 2))
    _, r, t, _ = m.process(FIRE)
    assert (m.sx, m.sy, r, t) == (41, 74, 0, False) and m.events == {"fire"}
    m.process(FIRE)
    assert (m.sx, m.sy) == (41, 72) and m.events == {"fire_ignored"}
    # grid at (10, 10): column 3 covers x 34..39, column 4 x 42..47; a box on x 40, 41 flies through the gap between them
    m = _model(march_period=16, bomb_period=64, ball_speed=4)
    m.sx, m.sy = 40, 40
    seen = set()
    for _ in range(9):
        m.process(NOOP)
        seen |= m.events
    assert m.sy == 0 and m.mask == 0xFFFFFF and m.totals == [0, 0, 0] and seen == {"shot_out"}
    # from x 39 (box 39, 40) it touches column 3; bottom row 2 spans y 22..25: the box (y, y+1) first overlaps at y = 25
    m = _model(march_period=16, bomb_period=64, alien_rewards=(5, 3, 2), ball_speed=1)
    m.sx, m.sy = 39, 27
    m.process(NOOP)
    assert (m.sy, m.mask) == (26, 0xFFFFFF)
    _, r, _, _ = m.process(NOOP)
    assert (m.sx, m.sy, r) == (0, 0, 2) and m.mask == 0xFFFFFF & ~(1 << 19) and m.totals == [1, 0, 0]
    assert m.events == {"alien_shot"}
    # aliens lie 2 px apart in both directions, so the 2 x 2 box never overlaps two of them: "the lowest overlapping bit"
    # only ever chooses between equal bits (the model still visits all four corners, as Breakout's brick test does)
    m = _model(ball_speed=1, march_period=16, bomb_period=64)
    m.mask = 1 << 19 | 1 << 11                                  # rows 2 and 1 of column 3
    m.sx, m.sy = 36, 27
    m.process(NOOP); m.process(NOOP)
    assert m.mask == 1 << 11 and m.totals == [1, 0, 0]          # the lower alien shields the upper one
    # a shot at speed 4 stops at the micro-step that hits: y 29 -> 28, 27, 26, 25 (hit at 25, the fourth micro-step)
    m = _model(ball_speed=4, march_period=16, bomb_period=64)
    m.sx, m.sy = 36, 29
    _, r, _, _ = m.process(NOOP)
    assert (r, m.sy, m.totals[0]) == (1, 0, 1)


def test_a_shot_leaves_the_field_above_y_6():
    m = _model(ball_speed=1, march_period=16, bomb_period=64)
    m.mask = 1                                                   # one alien far to the left
    m.sx, m.sy = 70, 7
    m.process(NOOP)
    assert (m.sx, m.sy) == (70, 6) and not m.events
    m.process(NOOP)
    assert (m.sx, m.sy) == (0, 0) and m.events == {"shot_out"}
    m.process(FIRE)                                              # and the cannon can fire again
    assert m.sy == 75 and m.events == {"fire"}


def test_a_bomb_drops_from_a_live_column_below_its_lowest_alien():
    seed = 0x1234567890
    for g in range(6):
        m = _model(seed=seed, g=g, serve_wait=0, bomb_period=3, march_period=16)
        m.mask = 0b00100100 | 0b00000100 << 8 | 0b10000000 << 16      # columns 2 and 5 in row 0, 2 in row 1, 7 in row 2
        m.process(NOOP); m.process(NOOP)
        assert m.bombs == [None] * 3 and m.bomb == 2
        m.process(NOOP)
        u = philox_ref((g, 0, IM.BOMB_STREAM, 0), (seed & 0xFFFFFFFF, seed >> 32))
        col = [2, 5, 7][int(u[0]) % 3]
        row = {2: 1, 5: 0, 7: 2}[col]
        assert m.bombs == [(10 + 8 * col + 2, 10 + 6 * row + 4), None, None] and m.events == {"drop"}
        assert (m.bomb, m.draw_index) == (0, 1)
        m.process(NOOP)                                          # it first moves in the next tick
        assert m.bombs[0][1] == 10 + 6 * row + 5
    # the second draw of an episode uses draw index 1, and the episode is counter word 1
    m = _model(seed=seed, g=3, serve_wait=0, bomb_period=1, march_period=16)
    m.reset()
    m.process(NOOP); m.process(NOOP)
    u = philox_ref((3, 1, IM.BOMB_STREAM, 1), (seed & 0xFFFFFFFF, seed >> 32))
    col = int(u[0]) % 8
    assert m.bombs[1] == (10 + 8 * col + 2, 10 + 6 * 2 + 4) and m.draw_index == 2


def test_the_draws_key_layout_against_the_philox_model():
    """key = seed (lo, hi), counter = (actor, episode, stream constant, draw index): the model's draw is the reference
    Philox of tests/philox_model.py on those words, and differs from the serve draw's."""
    try:
        from maze_model import philox4x32_10
    except ImportError:
        from tests.maze_model import philox4x32_10
    seed = 0xFEDCBA9876543210
    for ctr in ((0, 0, IM.BOMB_STREAM, 0), (199, 7, IM.BOMB_STREAM, 3), (2 ** 31, 2 ** 31, IM.BOMB_STREAM, 2 ** 31)):
        a = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
        b = philox_ref(ctr, (seed & 0xFFFFFFFF, seed >> 32))
        assert [int(x) for x in a] == [int(x) for x in b]
        c = philox_ref(ctr[:2] + (AM.SERVE_STREAM,) + ctr[3:], (seed & 0xFFFFFFFF, seed >> 32))
        assert [int(x) for x in b] != [int(x) for x in c]


def test_three_bombs_at_the_most_and_a_bomb_removed_at_the_floor():
    m = _model(serve_wait=0, bomb_period=1, march_period=16, paddle_width=4)
    m.px = 2                                                     # out of every column's way: column 0's bombs fall at x 12
    seen = []
    for _ in range(5):
        m.process(NOOP)
        seen.append((sum(b is not None for b in m.bombs), "drop_refused" in m.events, m.draw_index))
    assert seen == [(1, False, 1), (2, False, 2), (3, False, 3), (3, True, 3), (3, True, 3)]
    # the floor: y + 1 > 83 removes it, and the free slot is taken again at once (step 5 follows step 4)
    m.bombs[1] = (50, 81)
    m.process(NOOP)
    assert m.bombs[1] == (50, 82) and "floor" not in m.events
    m.process(NOOP)
    assert "floor" in m.events and "drop" in m.events and m.bombs[1] is not None and m.bombs[1][1] < 40 and m.draw_index == 4
    # bomb_speed = 4: 1-px micro-steps, removed by the one that crosses the floor
    m = _model(serve_wait=0, bomb_period=64, bomb_speed=4, march_period=16)
    m.bombs[2] = (60, 70)
    m.process(NOOP)
    assert m.bombs[2] == (60, 74)
    m.process(NOOP); m.process(NOOP)
    assert m.bombs[2] == (60, 82)
    m.process(NOOP)
    assert m.bombs == [None] * 3 and m.events == {"floor"}


@pytest.mark.parametrize("x,hit", [(34, False), (35, True), (36, True), (47, True), (48, False)])
def test_a_bomb_on_the_cannons_first_and_last_pixel_and_a_miss_by_one(x, hit):
    # cannon x 36..47 on rows 78..79; the bomb's box is x .. x + 1, and reaches row 78 with y = 77
    m = _model(serve_wait=5, bomb_period=64, march_period=16, life_reward=-2)
    m.grace = 0
    m.bombs = [(60, 30), (x, 76), (20, 50)]
    m.sx, m.sy = 70, 40
    _, r, t, _ = m.process(NOOP)
    if hit:
        assert (m.lives, r, t, m.totals) == (2, -2, False, [0, 1, 0]) and m.events == {"life_lost"}
        assert m.bombs == [None] * 3 and (m.sx, m.sy) == (0, 0)          # the shot and every bomb are removed
        assert m.grace == 5                                        # serve_wait + 1, less this tick's step 5
        assert _count(m.frame, AM.WHITE) == 8 and _count(m.frame, IM.BOMB) == 0
    else:
        assert (m.lives, r, m.bombs) == (3, 0, [(60, 31), (x, 77), (20, 51)]) and m.sy == 38 and not m.events
        for _ in range(5):                                         # beside the cannon it falls on to the floor
            m.process(NOOP)
        assert m.lives == 3 and m.bombs[1] == (x, 82)


def test_a_bomb_passes_a_cannon_that_is_not_there_and_bombs_move_in_slot_order():
    # slot 0 hits: slot 1 and 2 are removed where they were, not moved
    m = _model(serve_wait=0, bomb_period=64, march_period=16)
    m.bombs = [(40, 76), (10, 81), (10, 82)]
    m.process(NOOP)
    assert m.events == {"life_lost"} and m.lives == 2
    # slot 2 hits: slot 0 reached the floor first in the same tick
    m = _model(serve_wait=0, bomb_period=64, march_period=16)
    m.bombs = [(10, 82), None, (40, 76)]
    m.process(NOOP)
    assert m.events == {"floor", "life_lost"}
    # the shot and the bombs do not interact
    m = _model(serve_wait=0, bomb_period=64, march_period=16, ball_speed=1)
    m.bombs = [(41, 60), None, None]
    m.sx, m.sy = 41, 62
    m.process(NOOP)
    assert m.bombs[0] == (41, 61) and m.sy == 61
    m.process(NOOP)
    assert m.bombs[0] == (41, 62) and m.sy == 60


def test_the_grace_after_a_reset_and_after_a_lost_life():
    m = _model(serve_wait=3, bomb_period=1, march_period=16, paddle_width=4)
    m.px = 2
    seen = []
    for _ in range(5):
        m.process(NOOP)
        seen.append((m.grace, sum(b is not None for b in m.bombs), "drop_graced" in m.events))
    assert seen == [(2, 0, True), (1, 0, True), (0, 0, True), (0, 1, False), (0, 2, False)]
    m.bombs = [(3, 76), None, None]                              # a hit: no drop in its tick nor in the three after it
    seen = []
    for _ in range(5):
        m.process(NOOP)
        seen.append((m.grace, sum(b is not None for b in m.bombs)))
    assert seen == [(3, 0), (2, 0), (1, 0), (0, 0), (0, 1)] and m.lives == 2
    # serve_wait = 0: a reset allows the first drop at once; the tick of a hit still drops nothing
    m = _model(serve_wait=0, bomb_period=1, march_period=16, paddle_width=4)
    m.px = 2
    m.process(NOOP)
    assert m.bombs[0] is not None
    m.bombs = [(3, 76), None, None]
    m.process(NOOP)
    assert m.bombs == [None] * 3 and m.events == {"life_lost", "drop_graced"}
    m.process(NOOP)
    assert m.bombs[0] is not None


def test_the_last_life_the_last_alien_the_invasion_and_the_time_out():
    m = _model(serve_wait=0, bomb_period=64, march_period=16, lives=1, life_reward=-4)
    m.bombs[0] = (40, 76)
    _, r, t, _ = m.process(NOOP)
    assert (m.lives, r, t, m.success) == (0, -4, True, False) and m.events == {"life_lost", "end_lives"}
    m.reset()
    assert (m.lives, m.episode, m.totals, m.ep_steps, m.grace) == (1, 1, [0, 1, 0], 0, 0)
    # the last alien
    m = _model(ball_speed=1, march_period=16, bomb_period=64, alien_rewards=(1, 1, 6))
    m.mask = 1 << 19
    m.sx, m.sy = 36, 26
    _, r, t, _ = m.process(NOOP)
    assert (m.mask, r, t, m.success, m.totals) == (0, 6, True, True, [1, 0, 1])
    assert m.events == {"alien_shot", "wave_cleared", "end_clear"}
    # invasion: the lowest pixel row of the lowest live alien >= 76 after a march.  Rows 0..2 at gy = 57: row 2 ends at
    # 57 + 12 + 3 = 72; a descent of 4 makes it 76
    m = _model(march_period=1, descend=4, bomb_period=64, life_reward=-5, serve_wait=0)
    m.gx, m.gy, m.dir = 20, 56, 1
    m.process(NOOP)
    assert (m.gy, m.lives) == (60, 3) and m.events == {"descent"}                  # 60 + 15 = 75: not yet
    m.gx, m.dir, m.gy = 20, 1, 57
    _, r, t, _ = m.process(NOOP)
    assert (m.gy, m.lives, r, t, m.success) == (61, 0, -5, True, False)            # paid once, all lives lost
    assert m.totals == [0, 3, 0] and m.events == {"descent", "invasion", "end_lives"}
    # only the lowest LIVE alien counts: with row 2 shot the same state is no invasion (61 + 6 + 3 = 70)
    m = _model(march_period=1, descend=4, bomb_period=64, serve_wait=0)
    m.gx, m.dir, m.gy, m.mask = 20, 1, 57, 0xFFFF
    assert not m.process(NOOP)[2] and m.lives == 3
    # no march, no invasion: the test is made in a tick that marched
    m = _model(march_period=16, bomb_period=64, serve_wait=0)
    m.gy = 70
    assert not m.process(NOOP)[2]
    # the time-out
    m = _model(max_episode_steps=3)
    out = [m.process(NOOP)[1:3] for _ in range(3)]
    assert out == [(0, False), (0, False), (0, True)] and m.events == {"end_timeout"} and not m.success
    m.reset()
    assert m.ep_steps == 0 and not m.process(NOOP)[2]
    # the last alien in the last allowed step is a cleared wave
    m = _model(ball_speed=1, march_period=16, bomb_period=64, max_episode_steps=1)
    m.mask = 1 << 19
    m.sx, m.sy = 36, 26
    assert m.process(NOOP)[2] and m.success and "end_clear" in m.events


def test_a_step_past_a_terminal():
    m = _model(serve_wait=0, bomb_period=64, march_period=16, lives=1, life_reward=-4)
    m.bombs[0] = (40, 76)
    assert m.process(NOOP)[2]
    _, r, t, _ = m.process(FIRE)                                 # the game goes on: the cannon still fires
    assert (m.sy, r, t, m.lives) == (74, 0, True, 0) and m.events == {"fire", "end_lives"}
    m.bombs[0] = (40, 76)
    _, r, t, _ = m.process(NOOP)
    assert (m.lives, r, t, m.totals[1]) == (-1, -4, True, 2)     # lives fall below 0
    assert _count(m.frame, AM.WHITE) == 0                        # no life block, and the hit removed the shot
    # an invaded game marches on and is not invaded again
    m = _model(march_period=1, descend=8, bomb_period=64, life_reward=-5, serve_wait=0)
    m.gx, m.gy = 20, 60
    assert m.process(NOOP)[1:3] == (-5, True) and m.totals == [0, 3, 0]
    m.gx, m.dir = 20, 1
    assert m.process(NOOP)[1:3] == (0, True) and m.totals == [0, 3, 0] and m.gy == 76
    # a cleared wave stays cleared: no draw, no drop
    m = _model(ball_speed=1, march_period=16, bomb_period=1, serve_wait=0)
    m.mask = 1 << 19
    m.sx, m.sy = 36, 26
    assert m.process(NOOP)[2] and m.bombs == [None] * 3
    for _ in range(3):
        _, r, t, _ = m.process(FIRE)
        assert (r, t) == (0, True) and m.bombs == [None] * 3 and m.draw_index == 0 and m.totals == [1, 0, 1]


# ---- frames -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(), dict(alien_rows=1, lives=5, paddle_width=4), dict(alien_rows=4, lives=1, paddle_width=24)])
def test_reset_frame_pixel_counts(kw):
    m = _model(**kw)
    c = m.c
    assert _count(m.frame, AM.WHITE) == 4 * c.lives
    assert _count(m.frame, AM.BORDER) == 816 - 4 * c.lives
    assert _count(m.frame, AM.PADDLE) == 2 * c.paddle_width + 8 * 24          # alien row 0 has the cannon's colour
    for r in range(1, c.alien_rows):
        assert _count(m.frame, AM.ROW_COLOURS[r]) == 8 * 24
    assert _count(m.frame, IM.BOMB) == 0
    assert _count(m.frame, (0, 0, 0)) == 84 * 84 - 816 - 2 * c.paddle_width - 8 * 24 * c.alien_rows
    assert (m.frame[78:80, 42 - c.paddle_width // 2:42 + c.paddle_width // 2] == AM.PADDLE).all()
    assert (m.frame[10:14, 10:16] == AM.ROW_COLOURS[0]).all() and (m.frame[10:14, 16:18] == 0).all()
    assert (m.frame[14:16, 10:16] == 0).all()
    last = c.alien_rows - 1
    assert (m.frame[10 + 6 * last:14 + 6 * last, 66:72] == AM.ROW_COLOURS[last]).all()


def test_draw_order():
    m = _model()
    m.gy = 70                                                    # aliens over the cannon's rows: the cannon is in front
    m.bombs = [(40, 78), (41, 78), None]                         # bombs in front of the cannon, slot 0 in front of slot 1
    m.sx, m.sy = 41, 79                                          # the shot in front of the bombs
    f = m.render()
    assert (f[78:80, 36:40] == AM.PADDLE).all() and (f[76:78, 34:40] == AM.ROW_COLOURS[1]).all()
    assert (f[78, 40:43] == IM.BOMB).all() and (f[79, 40] == IM.BOMB).all()
    assert (f[79:81, 41:43] == AM.WHITE).all()


def test_pixel_change_of_one_march_step_and_of_one_cannon_move():
    # one row of 8 aliens (200 + 72 + 72 = 344 per pixel) moves 2 px to the right: per alien 2 columns x 4 rows vanish on
    # the left and appear on the right
    m = _model(alien_rows=1, march_period=1, bomb_period=64)
    _, _, _, pc = m.process(NOOP)
    assert m.gx == 12
    want = np.zeros((20, 20), np.float64)
    for col in range(8):
        for x in (10 + 8 * col, 11 + 8 * col, 16 + 8 * col, 17 + 8 * col):
            for y in range(10, 14):
                want[(y - 2) // 4, (x - 2) // 4] += 344
    np.testing.assert_array_equal(pc, (want / 12240.0).astype(np.float32))
    assert pc.dtype == np.float32 and (pc > 0).sum() == 16
    # one cannon move, as Breakout's paddle: x 36..38 go black, x 48..50 appear on rows 78, 79
    m = _model(march_period=16, bomb_period=64)
    _, _, _, pc = m.process(RIGHT)
    want = np.zeros((20, 20), np.float32)
    want[19, 8] = want[19, 11] = np.float32(4 * 344 / 12240.0)
    want[19, 9] = want[19, 12] = np.float32(2 * 344 / 12240.0)
    np.testing.assert_array_equal(pc, want)


# ---- action repeat ------------------------------------------------------------------------------------------------------------
def test_an_agent_step_at_action_repeat_4_is_four_model_ticks_with_the_rewards_summed():
    kw = dict(IM.TRACE_SETTINGS[1])
    one, four = _conf(**kw), _conf(action_repeat=4, **kw)
    rs = np.random.RandomState(5)
    cut = paid = 0
    for g in range(12):
        a, b = IM.HostInvaders(four, g, 3), IM.HostInvaders(one, g, 3)
        for step in range(120):
            act = int(rs.randint(0, 4))
            _, r, t, pc = a.process(act)
            reward, ticks, before = 0, 0, b.frame
            for _ in range(4):
                reward += b.process(act)[1]
                ticks += 1
                if b.ended():
                    break
            b.ep_steps = a.ep_steps                                # the step limit counts agent steps
            assert (r, a.ticks) == (reward, ticks) and (a.record() == b.record()).all(), (g, step)
            assert t == (b.ended() or a.ep_steps >= one.max_episode_steps)
            np.testing.assert_array_equal(pc, AM.pixel_change(b.frame, before))      # the states between ticks are not drawn
            cut += ticks < 4
            paid += r not in (0, 7, -1)
            assert ("cut_short" in a.events) == (ticks < 4)
            if t:
                a.reset(); b.reset()
    assert cut > 0 and paid > 0                                    # steps cut short, and steps whose ticks paid more than once
    # past a terminal one tick per step
    m = IM.HostInvaders(_conf(action_repeat=4, lives=1, serve_wait=0, bomb_period=64), 0, 0)
    m.bombs[0] = (40, 76)
    assert m.process(NOOP)[2] and m.ticks == 1
    m.process(FIRE)
    assert m.ticks == 1 and m.sy == 74


# ---- the traces of the GPU test -------------------------------------------------------------------------------------------------
def test_the_traces_hold_the_events_the_gpu_tests_rely_on():
    """The conditions tests/test_invaders_gpu.py relies on, on the model alone: a trace cannot silently stop covering a
    branch.  (The traces are computed once, invaders_model.run_trace, and shared with the GPU tests.)"""
    random = [IM.run_trace(k) for k in range(3)]
    for k, tr in enumerate(random):
        a0, act0 = AM.trace_inputs(k)
        assert (tr["acts"] == a0).all() and (tr["active"] == act0).all()          # the same input construction
        assert not tr["active"].all() and tr["active"].mean() > 0.8
        assert tr["events"] & IM.TRACE_EVENTS
    together = set().union(*[tr["events"] for tr in random])
    assert {"alien_shot", "life_lost", "floor", "descent", "drop_refused"} <= together
    assert IM.TRACE_EVENTS <= together, IM.TRACE_EVENTS - together
    # every watched actor's frame changes, and rewards of both signs are paid in the small setting
    assert set(np.unique(random[1]["reward"])) >= {-7.5, -1.0, 0.0, 7.0}
    assert (random[0]["pc"] > 0).any() and (random[0]["records"][:, :, 13:] != 0).any()
    assert IM.REPEAT_EVENTS <= IM.run_trace(3)["events"], IM.REPEAT_EVENTS - IM.run_trace(3)["events"]
    scripted = IM.run_trace(4)
    assert IM.SCRIPTED_EVENTS <= scripted["events"], IM.SCRIPTED_EVENTS - scripted["events"]
    assert {"wave_cleared", "invasion", "end_timeout"} <= scripted["events"]
    assert IM.trace_config(4).max_episode_steps < IM.SCRIPTED_STEPS


def test_random_play_is_rewarded_often():
    """The figure the game was added for, on a small sample (DESIGN §7n has 1,000 episodes): a random policy shoots
    aliens by the dozen per episode, where Breakout's gets 0.7 bricks."""
    conf = _conf()
    rs = np.random.RandomState(0)
    aliens = []
    for g in range(20):
        m = IM.HostInvaders(conf, g, 0, frames=False)
        while not m.process(int(rs.randint(0, 4)))[2]:
            pass
        aliens.append(m.totals[0])
    assert np.mean(aliens) > 3
