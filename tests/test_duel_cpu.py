"""CPU tests of the device arcade's duel: config validation with the cross-game keywords, both blocks, the
header's constants, and the rules on the host model of tests/duel_model.py, worked by hand."""
import os
import re

import numpy as np
import pytest

try:
    import arcade_model as AM
    import duel_model as DM
    from maze_model import philox4x32_10
except ImportError:            # imported as tests.<module>
    from tests import arcade_model as AM
    from tests import duel_model as DM
    from tests.maze_model import philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _conf(**kw):
    from unreal_amd.environment.arcade_environment import ArcadeConfig
    kw.setdefault("game", "duel")
    return ArcadeConfig(**kw)


def _model(seed=0, g=0, **kw):
    return DM.HostDuel(_conf(**kw), g, seed)


def _fly(m, bx, by, vx, vy):
    m.bx, m.by, m.vx, m.vy, m.wait = bx, by, vx, vy, -1
    m.frame = m.render()
    return m


def _count(frame, colour):
    return int((frame == colour).all(2).sum())


# ---- config ---------------------------------------------------------------------------------------------------------------
DUEL_BAD = [dict(points=0), dict(points=10), dict(points=True), dict(points=5.0), dict(points="5"),
            dict(opponent_width=2), dict(opponent_width=26), dict(opponent_width=11), dict(opponent_width=True),
            dict(opponent_width=12.0),
            dict(opponent_speed=-1), dict(opponent_speed=9), dict(opponent_speed=False), dict(opponent_speed=2.0),
            dict(win_reward=-1), dict(win_reward=101), dict(win_reward=True), dict(win_reward=1.0),
            dict(lose_reward=1), dict(lose_reward=-101), dict(lose_reward=False), dict(lose_reward=-1.0),
            # the shared settings keep Breakout's ranges
            dict(paddle_width=2), dict(paddle_width=26), dict(paddle_width=11), dict(paddle_width=True),
            dict(paddle_speed=0), dict(paddle_speed=9), dict(paddle_speed=1.0),
            dict(ball_speed=0), dict(ball_speed=5), dict(ball_speed=True),
            dict(serve_wait=-1), dict(serve_wait=256), dict(serve_wait=8.0),
            dict(max_episode_steps=0), dict(max_episode_steps=2 ** 31), dict(max_episode_steps=None),
            dict(max_episode_steps=100.0),
            # Breakout's own settings, even at Breakout's defaults
            dict(rows=6), dict(rows=2), dict(row_rewards=(1,) * 6), dict(lives=3), dict(life_reward=0), dict(life_reward=-1)]
BAD = [dict(game="duel", **kw) for kw in DUEL_BAD] + \
      [dict(game="pong"), dict(game="Duel"), dict(game=3),
       # the duel's own settings with game="breakout" (given or by default), even at the duel's defaults
       dict(game="breakout", points=5), dict(points=5), dict(opponent_width=12), dict(opponent_speed=2), dict(win_reward=1),
       dict(lose_reward=-1), dict(game="breakout", lose_reward=0)]


@pytest.mark.parametrize("kw", BAD, ids=[repr(sorted(k.items())) for k in BAD])
def test_a_setting_outside_its_range_or_of_the_other_game_is_a_value_error(kw):
    from unreal_amd.environment.environment import Environment
    with pytest.raises(ValueError):
        Environment.register_arcade_config("duel_bad", **kw)
    assert "duel_bad" not in Environment.ARCADE_CONFIG


def test_the_edges_of_every_range_are_accepted_and_registered():
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.arcade_environment import ArcadeConfig, GAMES
    assert GAMES == {"breakout": 1, "duel": 3}
    for kw in (dict(points=1, opponent_width=4, opponent_speed=0, win_reward=0, lose_reward=-100, paddle_width=4,
                    paddle_speed=1, ball_speed=1, serve_wait=0, max_episode_steps=1),
               dict(points=9, opponent_width=24, opponent_speed=8, win_reward=100, lose_reward=0, paddle_width=24,
                    paddle_speed=8, ball_speed=4, serve_wait=255, max_episode_steps=2 ** 31 - 1),
               dict(points=np.int64(3), opponent_width=np.int32(6))):
        ArcadeConfig(game="duel", **kw)
    try:
        Environment.register_arcade_config("duel_ok", game="duel")
        conf = Environment.ARCADE_CONFIG["duel_ok"]
        assert isinstance(conf, ArcadeConfig) and conf.game == "duel"
        assert (conf.points, conf.paddle_width, conf.paddle_speed, conf.ball_speed, conf.serve_wait, conf.opponent_width,
                conf.opponent_speed, conf.win_reward, conf.lose_reward, conf.max_episode_steps) == \
            (5, 12, 3, 2, 8, 12, 2, 1, -1, 5000)
        Environment.action_size = 18                       # another environment's cached count is not the arcade's
        assert Environment.get_action_size("arcade", "duel_ok") == 4
        assert Environment.action_size == 18
        assert Environment.get_objective_size("arcade", "duel_ok") == 0
        assert Environment.get_image_shape("arcade", "duel_ok") == [84, 84]
        # Breakout's defaults are untouched by the new keywords
        Environment.register_arcade_config("duel_ok")
        conf = Environment.ARCADE_CONFIG["duel_ok"]
        assert (conf.game, conf.rows, conf.row_rewards, conf.lives, conf.life_reward) == ("breakout", 6, (1,) * 6, 3, 0)
        assert not hasattr(conf, "points")
    finally:
        Environment.ARCADE_CONFIG.pop("duel_ok", None)
        Environment.action_size = -1


def test_both_blocks_by_value():
    c = _conf(points=7, max_episode_steps=123456, paddle_width=16, paddle_speed=5, ball_speed=3, opponent_width=20,
              serve_wait=20, lose_reward=-9, win_reward=11, opponent_speed=6)
    b = c.block(0xFEDCBA9876543210)
    assert b.dtype == np.int32 and b.shape == (24,)
    want = [3, 0, 7, 123456, 0x76543210, np.int32(-0x01234568), 16, 5, 3, 20, 20, -9, 11, 6] + [0] * 10
    assert b.tolist() == [int(w) for w in want]
    assert _conf().block(5).tolist() == [3, 0, 5, 5000, 5, 0, 12, 3, 2, 12, 8, -1, 1, 2] + [0] * 10
    assert _conf(max_episode_steps=2 ** 31 - 1).block(0)[3] == 2 ** 31 - 1
    # Breakout's block is what it was
    c = _conf(game="breakout", rows=3, row_rewards=(7, 4, 1), paddle_width=16, paddle_speed=5, ball_speed=3, lives=4,
              serve_wait=20, life_reward=-9, max_episode_steps=123456)
    want = [1, 0, 3, 123456, 0x76543210, np.int32(-0x01234568), 16, 5, 3, 4, 20, -9, 7, 4, 1] + [0] * 9
    assert c.block(0xFEDCBA9876543210).tolist() == [int(w) for w in want]
    assert _conf(game="breakout").block(5).tolist() == [1, 0, 6, 5000, 5, 0, 12, 3, 2, 3, 8, 0, 1, 1, 1, 1, 1, 1] + [0] * 6


def test_header_constants_are_the_python_ones():
    from unreal_amd import ops
    src = open(os.path.join(ROOT, "include", "unreal_hip.h")).read()
    defs = dict(re.findall(r"#define (UNREAL_ARCADE_\w+) (\w+)", src))
    assert int(defs["UNREAL_ARCADE_DUEL"]) == ops.ARCADE_DUEL == 3
    assert int(defs["UNREAL_ARCADE_BREAKOUT"]) == ops.ARCADE_BREAKOUT == 1
    assert int(defs["UNREAL_ARCADE_CFG_WORDS"]) == ops.ARCADE_CFG_WORDS == 24 == len(_conf().block(0))
    assert int(defs["UNREAL_ARCADE_RECORD"]) == ops.ARCADE_RECORD == 16 == len(_model().record())
    assert int(defs["UNREAL_ARCADE_SERVE_STREAM"], 16) == ops.ARCADE_SERVE_STREAM == DM.SERVE_STREAM
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("UNREAL_ARCADE_DUEL", "opponent_width", "opponent_speed"):
        assert word in text and word in src, word


# ---- the rules, by hand ------------------------------------------------------------------------------------------------------
def test_serve_by_fire_in_both_directions_and_at_serve_wait():
    seed = 0x1234567890
    ups = set()
    for g in range(8):
        m = _model(seed=seed, g=g)
        assert (m.px, m.ox, m.wait, m.mine, m.theirs, m.episode) == (36, 36, 0, 0, 0, 0)
        _, r, t, _ = m.process(AM.FIRE)
        u = philox4x32_10((g, 0, DM.SERVE_STREAM, 0), (seed & 0xFFFFFFFF, seed >> 32))
        assert (m.bx, m.by, m.wait, m.serve_index) == (2 + 2 * (int(u[0]) % 39), 40, -1, 1)
        assert m.vx == (1 if int(u[1]) & 1 else -1) and m.vy == (1 if int(u[2]) & 1 else -1)
        assert (r, t) == (0, False) and m.events == {"serve_fire"} and m.bx % 2 == 0 and 2 <= m.bx <= 78
        ups.add(m.vy)
        # the ball did not move in the serving step; in the next it makes ball_speed = 2 micro-steps
        bx, vy = m.bx, m.vy
        m.process(AM.NOOP)
        assert m.by == 40 + 2 * vy and abs(m.bx - bx) <= 2
    assert ups == {-1, 1}
    # serve_wait = 3: three steps count, the fourth serves; the second serve of an episode uses serve index 1
    m = _model(seed=seed, g=5, serve_wait=3)
    for k in range(3):
        m.process(AM.NOOP)
        assert m.wait == k + 1 and not m.events
    m.serve_index = 1
    m.process(AM.LEFT)
    u = philox4x32_10((5, 0, DM.SERVE_STREAM, 1), (seed & 0xFFFFFFFF, seed >> 32))
    assert m.events == {"serve_auto"} and (m.wait, m.bx, m.px, m.serve_index) == (-1, 2 + 2 * (int(u[0]) % 39), 33, 2)
    assert m.vy == (1 if int(u[2]) & 1 else -1)
    # serve_wait = 0: only fire serves
    m = _model(serve_wait=0)
    for _ in range(300):
        m.process(AM.NOOP)
    assert m.wait == 300 and m.serve_index == 0


def test_side_walls_and_no_top_wall():
    m = _fly(_model(ball_speed=1), 2, 50, -1, -1)
    m.process(AM.NOOP)
    assert (m.bx, m.by, m.vx, m.vy) == (2, 49, 1, -1) and m.events == {"wall_left"}
    m = _fly(_model(ball_speed=1), 80, 50, 1, 1)
    m.process(AM.NOOP)
    assert (m.bx, m.by, m.vx, m.vy) == (80, 51, -1, 1) and m.events == {"wall_right"}
    m = _fly(_model(ball_speed=1), 79, 50, 2, 1)           # two pixels at a time: 81 is outside too
    m.process(AM.NOOP)
    assert (m.bx, m.by, m.vx) == (79, 51, -2) and m.events == {"wall_right"}
    m = _fly(_model(ball_speed=1), 3, 50, -2, 1)
    m.process(AM.NOOP)
    assert (m.bx, m.vx) == (3, 2) and m.events == {"wall_left"}
    # the third wall of Breakout, the top, is the opponent's end of the field: the ball does not come back
    m = _fly(_model(ball_speed=1), 40, 6, 1, -1)
    _, r, t, _ = m.process(AM.NOOP)
    assert (m.bx, m.by, m.vx, m.vy, m.wait) == (41, 6, 1, -1, 0) and m.events == {"point_won"} and (r, t) == (1, False)


SEGMENTS = [(35, -2), (37, -2), (38, -1), (40, -1), (41, 1), (43, 1), (44, 2), (47, 2)]


@pytest.mark.parametrize("bx,vx", SEGMENTS)
def test_the_four_segments_of_the_agents_paddle(bx, vx):
    # paddle x 36..47, middle 42: d = bx + 1 - 42
    m = _fly(_model(ball_speed=1), bx - 1, 76, 1, 1)
    _, r, t, _ = m.process(AM.NOOP)
    assert (m.bx, m.by, m.vx, m.vy) == (bx, 76, vx, -1) and (r, t) == (0, False)
    assert m.events == {"paddle_%d" % ((-2, -1, 1, 2).index(vx))}


@pytest.mark.parametrize("bx,vx", SEGMENTS)
def test_the_four_segments_of_the_opponents_paddle(bx, vx):
    # a standing opponent, x 36..47 on rows 8..9: the ball at by = 10 moving up touches it (ty == 9)
    m = _fly(_model(ball_speed=1, opponent_speed=0), bx - 1, 10, 1, -1)
    _, r, t, _ = m.process(AM.NOOP)
    assert (m.bx, m.by, m.vx, m.vy, m.ox) == (bx, 10, vx, 1, 36) and (r, t) == (0, False)
    assert m.events == {"opp_%d" % ((-2, -1, 1, 2).index(vx))}


def test_a_paddle_collides_only_on_its_line_and_the_ball_passes_beside_it():
    for bx in (34, 48):                                   # beside the agent's paddle: on it goes
        m = _fly(_model(ball_speed=1), bx - 1, 76, 1, 1)
        m.process(AM.NOOP)
        assert (m.bx, m.by, m.vy) == (bx, 77, 1) and not m.events
    m = _fly(_model(ball_speed=1), 40, 77, 1, 1)          # already below the top line: it passes through
    m.process(AM.NOOP)
    assert (m.by, m.vy) == (78, 1) and not m.events
    for bx in (34, 48):                                   # beside the opponent's
        m = _fly(_model(ball_speed=1, opponent_speed=0), bx - 1, 10, 1, -1)
        m.process(AM.NOOP)
        assert (m.bx, m.by, m.vy) == (bx, 9, -1) and not m.events
    m = _fly(_model(ball_speed=1, opponent_speed=0), 40, 9, 1, -1)
    m.process(AM.NOOP)
    assert (m.by, m.vy) == (8, -1) and not m.events
    # the agent's paddle does not stop a ball moving up, nor the opponent's one moving down
    m = _fly(_model(ball_speed=1), 40, 78, 1, -1)
    m.process(AM.NOOP)
    assert (m.by, m.vy) == (77, -1) and not m.events
    m = _fly(_model(ball_speed=1, opponent_speed=0), 40, 8, 1, 1)
    m.process(AM.NOOP)
    assert (m.by, m.vy) == (9, 1) and not m.events
    # the opponent moves before the ball: at speed 2 it reaches a ball one pixel beside it (ox 36 -> 34..45 meets x 34, 35)
    m = _fly(_model(ball_speed=1), 33, 10, 1, -1)
    m.process(AM.NOOP)
    assert (m.ox, m.bx, m.by, m.vy, m.vx) == (34, 34, 10, 1, -2) and m.events == {"opp_0"}


def test_a_point_of_each_sign():
    m = _fly(_model(lose_reward=-5), 10, 82, 1, 1)
    _, r, t, _ = m.process(AM.NOOP)
    assert (m.theirs, m.mine, m.wait, r, t) == (1, 0, 0, -5, False) and m.events == {"point_lost"} and m.totals == [0, 1, 0]
    assert (m.bx, m.by, m.vx, m.vy) == (11, 82, 1, 1)      # the second micro-step did not run; the ball's words stay
    assert _count(m.frame, AM.WHITE) == 0                  # no ball
    assert _count(m.frame, DM.OPPONENT) == 2 * 12 + 4 and (m.frame[2:4, 78:80] == DM.OPPONENT).all()
    m.process(AM.NOOP)
    assert m.wait == 1
    m = _fly(_model(win_reward=4), 10, 6, 1, -1)
    _, r, t, _ = m.process(AM.NOOP)
    assert (m.mine, m.theirs, m.wait, r, t) == (1, 0, 0, 4, False) and m.events == {"point_won"} and m.totals == [1, 0, 0]
    assert (m.bx, m.by, m.vx, m.vy) == (11, 6, 1, -1)
    assert m.ox == 34                                      # the opponent followed the ball of the state before the step
    assert _count(m.frame, AM.WHITE) == 4 and (m.frame[2:4, 4:6] == AM.WHITE).all()


def test_the_match_point_of_each_side_and_the_reset():
    m = _fly(_model(), 10, 6, 1, -1)
    m.mine = 4
    _, r, t, _ = m.process(AM.NOOP)
    assert (m.mine, r, t, m.success) == (5, 1, True, True) and m.events == {"point_won", "end_win"} and m.totals == [1, 0, 1]
    m.reset()
    assert (m.mine, m.theirs, m.episode, m.totals, m.ep_steps) == (0, 0, 1, [1, 0, 1], 0)
    assert (m.px, m.ox, m.bx, m.by, m.vx, m.vy, m.wait, m.serve_index) == (36, 36, 0, 0, 0, 0, 0, 0)
    m = _fly(_model(), 10, 82, 1, 1)
    m.theirs = 4
    _, r, t, _ = m.process(AM.NOOP)
    assert (m.theirs, r, t, m.success) == (5, -1, True, False) and m.events == {"point_lost", "end_lose"}
    assert m.totals == [0, 1, 0]


def test_time_out_and_a_point_in_the_last_step():
    m = _model(max_episode_steps=3)
    out = [m.process(AM.NOOP)[1:3] for _ in range(3)]
    assert out == [(0, False), (0, False), (0, True)] and m.events == {"end_timeout"} and not m.success
    m.reset()
    assert m.ep_steps == 0 and not m.process(AM.NOOP)[2]
    # a point and the step limit in one step: a time-out unless it is the match point
    m = _fly(_model(max_episode_steps=1), 10, 6, 1, -1)
    _, r, t, _ = m.process(AM.NOOP)
    assert (r, t, m.success) == (1, True, False) and m.events == {"point_won", "end_timeout"}
    m = _fly(_model(max_episode_steps=1), 10, 6, 1, -1)
    m.mine = 4
    _, r, t, _ = m.process(AM.NOOP)
    assert (r, t, m.success) == (1, True, True) and m.events == {"point_won", "end_win"} and m.totals == [1, 0, 1]
    m = _fly(_model(max_episode_steps=1), 10, 82, 1, 1)
    m.theirs = 4
    _, r, t, _ = m.process(AM.NOOP)
    assert (r, t, m.success) == (-1, True, False) and m.events == {"point_lost", "end_lose"}


def test_the_opponent_follows_a_rising_ball_to_both_edges_and_returns_to_the_centre():
    m = _fly(_model(ball_speed=1, opponent_speed=8), 2, 70, -1, -1)
    seen = []
    for _ in range(6):
        m.process(AM.NOOP)
        seen.append(m.ox)
    assert seen == [28, 20, 12, 4, 2, 2]                  # clamped at the field's left edge
    m = _fly(_model(ball_speed=1, opponent_speed=8), 80, 70, 1, -1)
    seen = []
    for _ in range(6):
        m.process(AM.NOOP)
        seen.append(m.ox)
    assert seen == [44, 52, 60, 68, 70, 70]               # 82 - 12
    m.by, m.vy = 20, 1                                    # the ball turns down: back to the middle, 42 - 6
    seen = []
    for _ in range(6):
        m.process(AM.NOOP)
        seen.append(m.ox)
    assert seen == [62, 54, 46, 38, 36, 36]
    # it moves while the ball waits too
    m = _model(serve_wait=0)
    m.ox = 2
    for k in range(3):
        m.process(AM.NOOP)
        assert (m.ox, m.wait) == (4 + 2 * k, k + 1)


def test_a_standing_opponent():
    m = _fly(_model(ball_speed=1, opponent_speed=0), 2, 70, -1, -1)
    for _ in range(20):
        m.process(AM.RIGHT)
        assert m.ox == 36
    m.ox = 10                                             # nor does it return to the middle
    m.by, m.vy = 20, 1
    m.process(AM.NOOP)
    assert m.ox == 10


def test_scores_run_past_points_without_a_reset():
    m = _fly(_model(points=1, opponent_speed=0), 10, 6, 1, -1)
    assert m.process(AM.NOOP)[2] and m.totals == [1, 0, 1] and m.events == {"point_won", "end_win"}
    _, r, t, _ = m.process(AM.FIRE)                        # the game goes on: the waiting ball is served again
    assert (m.wait, m.serve_index, r, t) == (-1, 1, 0, True) and m.events == {"serve_fire", "end_win"}
    _fly(m, 10, 6, 1, -1)
    _, r, t, _ = m.process(AM.NOOP)
    assert (m.mine, r, t) == (2, 1, True) and m.totals == [2, 0, 1]       # the match is counted once
    m.mine, m.theirs = 11, 12                              # nine blocks a side at the most
    _fly(m, 10, 6, 1, -1)
    m.process(AM.NOOP)
    assert m.mine == 12 and _count(m.frame, AM.WHITE) == 4 * 9 and _count(m.frame, DM.OPPONENT) == 4 * 9 + 2 * 12
    assert (m.frame[2:4, 36:38] == AM.WHITE).all() and (m.frame[2:4, 46:48] == DM.OPPONENT).all()
    assert (m.frame[2:4, 38:46] == AM.BORDER).all()
    m = _fly(_model(points=1), 10, 82, 1, 1)
    assert m.process(AM.NOOP)[2] and m.events == {"point_lost", "end_lose"}
    _fly(m, 10, 82, 1, 1)
    _, r, t, _ = m.process(AM.NOOP)
    assert (m.theirs, r, t, m.success) == (2, -1, True, False) and m.totals == [0, 2, 0]


@pytest.mark.parametrize("kw", [dict(), dict(paddle_width=24, opponent_width=4), dict(paddle_width=4, opponent_width=24)])
def test_reset_frame_pixel_counts(kw):
    m = _model(**kw)
    c = m.c
    assert _count(m.frame, AM.BORDER) == 816
    assert _count(m.frame, AM.WHITE) == 0                                  # no points, no ball
    assert _count(m.frame, AM.PADDLE) == 2 * c.paddle_width
    assert _count(m.frame, DM.OPPONENT) == 2 * c.opponent_width
    assert _count(m.frame, (0, 0, 0)) == 84 * 84 - 816 - 2 * c.paddle_width - 2 * c.opponent_width
    assert (m.frame[78:80, 42 - c.paddle_width // 2:42 + c.paddle_width // 2] == AM.PADDLE).all()
    assert (m.frame[8:10, 42 - c.opponent_width // 2:42 + c.opponent_width // 2] == DM.OPPONENT).all()


def test_pixel_change_of_one_paddle_move_by_hand():
    m = _model()
    _, _, _, pc = m.process(AM.RIGHT)                   # x 36..38 go black, x 48..50 appear: 344 per pixel, rows 78, 79
    want = np.zeros((20, 20), np.float32)
    # crop coordinates x - 2 = 34, 35 | 36 and 46, 47 | 48; y - 2 = 76, 77: block row 19
    want[19, 8] = want[19, 11] = np.float32(4 * 344 / 12240.0)
    want[19, 9] = want[19, 12] = np.float32(2 * 344 / 12240.0)
    np.testing.assert_array_equal(pc, want)
    assert (m.px, m.ox) == (39, 36) and pc.dtype == np.float32
    # the opponent's: from x 33 three pixels back to the middle; 66 + 72 + 200 = 338 per pixel, rows 8, 9
    m = _model(opponent_speed=3, serve_wait=0)
    m.ox = 33
    m.frame = m.render()
    _, _, _, pc = m.process(AM.NOOP)                    # x 33..35 go black, x 45..47 appear
    want = np.zeros((20, 20), np.float32)
    # crop coordinates x - 2 = 31 | 32, 33 and 43 | 44, 45; y - 2 = 6, 7: block row 1
    want[1, 7] = want[1, 10] = np.float32(2 * 338 / 12240.0)
    want[1, 8] = want[1, 11] = np.float32(4 * 338 / 12240.0)
    np.testing.assert_array_equal(pc, want)
    assert m.ox == 36


# ---- the traces of the GPU test -------------------------------------------------------------------------------------------------
def _events_of(models, steps, choose):
    seen = set()
    for s in range(steps):
        for b, m in enumerate(models):
            a = choose(s, b, m)
            if a is None:
                continue
            terminal = m.process(a)[2]
            seen |= m.events
            if terminal:
                m.reset()
    return seen


@pytest.mark.parametrize("k", range(len(DM.TRACE_SETTINGS)))
def test_the_random_traces_hold_the_events_the_gpu_test_asserts(k):
    acts, active = DM.trace_inputs(k)
    a0, act0 = AM.trace_inputs(k)
    assert (acts == a0).all() and (active == act0).all()            # the same input construction
    models = DM.host_batch(_conf(**DM.TRACE_SETTINGS[k]), DM.TRACE_B, DM.TRACE_SEED, frames=False)
    seen = _events_of(models, DM.TRACE_STEPS, lambda s, b, m: acts[s, b] if active[s, b] else None)
    assert DM.TRACE_EVENTS[k] <= seen, DM.TRACE_EVENTS[k] - seen
    assert not active.all() and active.mean() > 0.8


def test_the_traces_together_hold_every_event():
    models = DM.host_batch(_conf(**DM.SCRIPTED_SETTING), DM.SCRIPTED_B, DM.TRACE_SEED, frames=False)
    seen = _events_of(models, DM.SCRIPTED_STEPS, lambda s, b, m: AM.follow_ball(m))
    assert DM.SCRIPTED_EVENTS <= seen, DM.SCRIPTED_EVENTS - seen
    assert set().union(*DM.TRACE_EVENTS) == DM.EVERY_EVENT - {"end_timeout"}
    assert set().union(DM.SCRIPTED_EVENTS, *DM.TRACE_EVENTS) == DM.EVERY_EVENT
