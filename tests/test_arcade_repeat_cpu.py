"""CPU tests of the device arcade's action repeat and paddle-return reward: validation of the two settings, both
blocks, the header's text, the rules of an agent step worked by hand on the host models of tests/repeat_model.py, and that
the traces of tests/test_arcade_repeat_gpu.py hold their events on the models alone."""
import os

import numpy as np
import pytest

try:
    import arcade_model as AM
    import repeat_model as RM
    from maze_model import philox4x32_10
except ImportError:            # imported as tests.<module>
    from tests import arcade_model as AM
    from tests import repeat_model as RM
    from tests.maze_model import philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMES = ("breakout", "duel")


def _conf(**kw):
    from unreal_amd.environment.arcade_environment import ArcadeConfig
    return ArcadeConfig(**kw)


def _model(seed=0, g=0, **kw):
    conf = _conf(**kw)
    return RM.model_class(conf)(conf, g, seed)


def _fly(m, bx, by, vx, vy):
    m.bx, m.by, m.vx, m.vy, m.wait = bx, by, vx, vy, -1
    m.frame = m.render()
    return m


# ---- config, block, header -------------------------------------------------------------------------------------------------
BAD = [dict(action_repeat=0), dict(action_repeat=9), dict(action_repeat=-1), dict(action_repeat=True),
       dict(action_repeat=4.0), dict(action_repeat="4"), dict(action_repeat=None), dict(action_repeat=np.bool_(True)),
       dict(return_reward=-1), dict(return_reward=101), dict(return_reward=False), dict(return_reward=1.0),
       dict(return_reward="1"), dict(return_reward=None)]


@pytest.mark.parametrize("game", GAMES)
@pytest.mark.parametrize("kw", BAD, ids=[repr(sorted(k.items())) for k in BAD])
def test_a_setting_outside_its_range_is_a_value_error(game, kw):
    from unreal_amd.environment.environment import Environment
    with pytest.raises(ValueError):
        Environment.register_arcade_config("repeat_bad", game=game, **kw)
    assert "repeat_bad" not in Environment.ARCADE_CONFIG
    with pytest.raises(ValueError):
        _conf(game=game, **kw)


@pytest.mark.parametrize("game", GAMES)
def test_the_edges_of_both_ranges_are_accepted_and_registered(game):
    from unreal_amd.environment.environment import Environment
    for kw in (dict(action_repeat=1, return_reward=0), dict(action_repeat=8, return_reward=100),
               dict(action_repeat=np.int64(4), return_reward=np.int32(2))):
        c = _conf(game=game, **kw)
        assert (c.action_repeat, c.return_reward) == (int(kw["action_repeat"]), int(kw["return_reward"]))
        assert type(c.action_repeat) is int and type(c.return_reward) is int
    try:
        Environment.register_arcade_config("repeat_ok", game=game, action_repeat=4, return_reward=2)
        conf = Environment.ARCADE_CONFIG["repeat_ok"]
        assert (conf.game, conf.action_repeat, conf.return_reward) == (game, 4, 2)
        Environment.register_arcade_config("repeat_ok", game=game)
        conf = Environment.ARCADE_CONFIG["repeat_ok"]
        assert (conf.action_repeat, conf.return_reward) == (1, 0)
    finally:
        Environment.ARCADE_CONFIG.pop("repeat_ok", None)


def test_both_blocks_by_value():
    seed = 0xFEDCBA9876543210
    lo, hi = 0x76543210, int(np.int32(-0x01234568))
    c = _conf(game="duel", points=7, max_episode_steps=123456, paddle_width=16, paddle_speed=5, ball_speed=3,
              opponent_width=20, serve_wait=20, lose_reward=-9, win_reward=11, opponent_speed=6, action_repeat=4,
              return_reward=13)
    b = c.block(seed)
    assert b.dtype == np.int32 and b.shape == (24,)
    assert b.tolist() == [3, 3, 7, 123456, lo, hi, 16, 5, 3, 20, 20, -9, 11, 6, 0, 0, 0, 0, 13, 0, 0, 0, 0, 0]
    c = _conf(rows=3, row_rewards=(7, 4, 1), paddle_width=16, paddle_speed=5, ball_speed=3, lives=4, serve_wait=20,
              life_reward=-9, max_episode_steps=123456, action_repeat=8, return_reward=100)
    assert c.block(seed).tolist() == [1, 7, 3, 123456, lo, hi, 16, 5, 3, 4, 20, -9, 7, 4, 1, 0, 0, 0, 100, 0, 0, 0, 0, 0]
    assert _conf(rows=6, row_rewards=(1, 2, 3, 4, 5, 6), return_reward=9).block(0)[12:20].tolist() == [1, 2, 3, 4, 5, 6, 9, 0]


def test_the_blocks_at_the_defaults_are_byte_for_byte_what_they_were():
    """The words as tests/test_duel_cpu.py pins them for the blocks before words 1 and 18 had a meaning."""
    was = {"duel": [3, 0, 5, 5000, 5, 0, 12, 3, 2, 12, 8, -1, 1, 2] + [0] * 10,
           "breakout": [1, 0, 6, 5000, 5, 0, 12, 3, 2, 3, 8, 0, 1, 1, 1, 1, 1, 1] + [0] * 6}
    for game in GAMES:
        want = np.array(was[game], dtype=np.int32).tobytes()
        assert _conf(game=game).block(5).tobytes() == want
        assert _conf(game=game, action_repeat=1, return_reward=0).block(5).tobytes() == want


def test_the_header_names_words_1_and_18_and_the_agent_step():
    """Both games' block layouts name the two words, and the rules of an agent step are written out after them."""
    src = open(os.path.join(ROOT, "include", "unreal_hip.h")).read()
    assert src.count("[1] action_repeat - 1") == 2 and src.count("[18] return_reward 0..100") == 2
    for words in ("An agent step", "sum over its ticks", "the record after the last tick", "agent steps, not ticks",
                  "the opponent's returns pay nothing", "(seed, global actor, episode, serve_index)"):
        assert words in src, words


# ---- the rules of an agent step, by hand -------------------------------------------------------------------------------------
@pytest.mark.parametrize("game", GAMES)
def test_four_ticks_from_a_waiting_ball(game):
    """Fire: tick 1 serves, ticks 2..4 are 3 x ball_speed micro-steps of flight; the paddle moves in every tick; one step."""
    seed = 0x1234567890
    ups = set()
    for g in range(8):
        m = _model(seed=seed, g=g, game=game, action_repeat=4)
        _, r, t, pc = m.process(AM.FIRE)
        u = philox4x32_10((g, 0, AM.SERVE_STREAM, 0), (seed & 0xFFFFFFFF, seed >> 32))
        vy = 1 if game == "breakout" or int(u[2]) & 1 else -1
        ups.add(vy)
        assert (m.by, m.vy, m.wait, m.serve_index, m.ep_steps, m.ticks) == (40 + 6 * vy, vy, -1, 1, 1, 4)
        assert abs(m.bx - (2 + 2 * (int(u[0]) % 39))) <= 6 and (r, t) == (0, False)
        assert {"serve_fire", "serve_and_fly"} <= m.events and "cut_short" not in m.events
        assert pc.sum() > 0 and (m.frame == RM.frame_of(m.c, m.record())).all()
    assert ups == ({1} if game == "breakout" else {-1, 1})
    # a repeated move: 4 x paddle_speed, clamped; wait advances once per tick and the ball serves itself within the step
    m = _model(game=game, action_repeat=4, serve_wait=2)
    m.process(AM.RIGHT)
    assert (m.px, m.wait, m.by, m.serve_index, m.ticks) == (36 + 12, -1, 40 + 2 * m.vy, 1, 4)
    assert {"serve_auto", "serve_and_fly"} <= m.events
    m = _model(game=game, action_repeat=8, serve_wait=0)
    m.process(AM.LEFT)
    assert (m.px, m.wait, m.ep_steps) == (36 - 24, 8, 1) and not m.events
    m.process(AM.LEFT)
    assert (m.px, m.wait, m.ep_steps) == (2, 16, 2)


def test_the_duels_opponent_moves_in_every_tick():
    m = _fly(_model(game="duel", action_repeat=4, ball_speed=1, opponent_speed=2), 60, 50, 1, -1)
    m.process(AM.NOOP)          # targets 61, 62, 63, 64 of a paddle whose middle starts at 42
    assert (m.ox, m.bx, m.by) == (36 + 8, 64, 46)


@pytest.mark.parametrize("game", GAMES)
def test_the_last_life_or_point_on_tick_2_of_4_cuts_the_step_short(game):
    own = dict(lives=1, life_reward=-4) if game == "breakout" else dict(points=1, lose_reward=-4)
    m = _fly(_model(game=game, action_repeat=4, ball_speed=1, **own), 10, 81, 1, 1)
    _, r, t, _ = m.process(AM.RIGHT)
    # tick 1: by 82; tick 2: ty + 1 = 84 > 83; ticks 3 and 4 do not run: the paddle made two moves
    assert (m.ticks, m.px, m.wait, m.ep_steps) == (2, 36 + 6, 0, 1) and (r, t) == (-4, True)
    assert m.events >= {"cut_short", "end_lives" if game == "breakout" else "end_lose"} and not m.success
    # the batch-1 case: stepped on without a reset the state stays ended, and every step is one tick
    for k in range(1, 4):
        _, r, t, _ = m.process(AM.RIGHT)
        assert (m.ticks, m.px, m.wait, m.ep_steps) == (1, 42 + 3 * k, k, 1 + k) and (r, t) == (0, True)
        assert "cut_short" in m.events
    _, r, t, _ = m.process(AM.FIRE)
    assert (m.ticks, m.wait, m.by) == (1, -1, 40) and t and "serve_and_fly" not in m.events


def test_the_duels_match_point_on_tick_2_of_4():
    m = _fly(_model(game="duel", action_repeat=4, ball_speed=1, points=1, win_reward=9, opponent_speed=0), 70, 7, 1, -1)
    _, r, t, _ = m.process(AM.LEFT)
    assert (m.ticks, m.px, m.mine, m.totals, m.wait) == (2, 30, 1, [1, 0, 1], 0) and (r, t) == (9, True)
    assert m.events >= {"cut_short", "point_won", "end_win"} and m.success
    _, r, t, _ = m.process(AM.LEFT)
    assert (m.ticks, m.px, m.totals) == (1, 27, [1, 0, 1]) and (r, t) == (0, True)


def test_breakouts_last_brick_on_tick_2_of_4():
    m = _model(action_repeat=4, ball_speed=1, rows=1, row_rewards=(5,))
    m.bricks = 1 << 3                                      # x 26..33, y 18..20
    _fly(m, 30, 22, 1, -1)
    _, r, t, _ = m.process(AM.NOOP)                        # tick 1: by 21; tick 2: ty = 20 overlaps the brick
    assert (m.ticks, m.bricks, m.vy, m.totals) == (2, 0, 1, [1, 0, 1]) and (r, t) == (5, True)
    assert m.events >= {"cut_short", "brick_y", "end_clear"} and m.success


@pytest.mark.parametrize("game", GAMES)
def test_a_step_at_the_step_limit_still_runs_every_tick(game):
    m = _model(game=game, action_repeat=4, max_episode_steps=2)
    _, r, t, _ = m.process(AM.NOOP)
    assert (m.ticks, m.wait, m.ep_steps, t) == (4, 4, 1, False)
    _, r, t, _ = m.process(AM.FIRE)                        # the last allowed step: a serve and three ticks of flight
    assert (m.ticks, m.wait, m.by, m.ep_steps, t) == (4, -1, 40 + 6 * m.vy, 2, True)
    assert m.events >= {"end_timeout", "serve_and_fly"} and "cut_short" not in m.events and not m.success
    # a point that is no match point in the last allowed step: a time-out, after all four ticks
    own = dict(lives=3, life_reward=-2) if game == "breakout" else dict(points=3, lose_reward=-2)
    m = _fly(_model(game=game, action_repeat=4, ball_speed=1, max_episode_steps=1, serve_wait=1, **own), 10, 82, 1, 1)
    _, r, t, _ = m.process(AM.NOOP)                        # lost, wait 0 -> 1, served by itself, one tick of flight
    assert (m.ticks, m.wait, m.serve_index, m.by) == (4, -1, 1, 40 + m.vy) and (r, t) == (-2, True)
    assert m.events >= {"end_timeout", "lost_then_wait", "serve_auto", "serve_and_fly"}


SEGMENTS = [(35, -2), (37, -2), (38, -1), (40, -1), (41, 1), (43, 1), (44, 2), (47, 2)]


@pytest.mark.parametrize("game", GAMES)
@pytest.mark.parametrize("bx,vx", SEGMENTS)
def test_return_reward_on_each_segment_of_the_agents_paddle(game, bx, vx):
    # paddle x 36..47, middle 42 (tests/test_duel_cpu.py's segments)
    m = _fly(_model(game=game, ball_speed=1, return_reward=5), bx - 1, 76, 1, 1)
    _, r, t, _ = m.process(AM.NOOP)
    assert (m.bx, m.by, m.vx, m.vy) == (bx, 76, vx, -1) and (r, t) == (5, False)
    assert m.events == {"paddle_%d" % ((-2, -1, 1, 2).index(vx)), "returned"}
    # at four ticks of four micro-steps the return is paid once, in its tick, and the ball flies on
    m = _fly(_model(game=game, ball_speed=4, action_repeat=4, return_reward=5), bx - 1, 76, 1, 1)
    _, r, t, _ = m.process(AM.NOOP)
    assert (m.by, m.vy, m.ticks) == (76 - 15, -1, 4) and (r, t) == (5, False) and "two_rewards" not in m.events
    # beside the paddle nothing is paid
    m = _fly(_model(game=game, ball_speed=1, return_reward=5), 48 - 1, 76, 1, 1)
    assert m.process(AM.NOOP)[1] == 0 and m.by == 77 and "returned" not in m.events


@pytest.mark.parametrize("bx,vx", SEGMENTS)
def test_the_opponents_returns_pay_nothing(bx, vx):
    m = _fly(_model(game="duel", ball_speed=1, opponent_speed=0, return_reward=5), bx - 1, 10, 1, -1)
    _, r, t, _ = m.process(AM.NOOP)
    assert (m.bx, m.by, m.vx, m.vy) == (bx, 10, vx, 1) and (r, t) == (0, False)
    assert m.events == {"opp_%d" % ((-2, -1, 1, 2).index(vx))}


def test_two_ticks_of_one_step_pay_and_the_sum_is_not_clipped():
    m = _model(action_repeat=2, ball_speed=1, rows=2, row_rewards=(70, 50))
    m.bricks = 1 << 13 | 1 << 2 | 1 << 9       # (row 1, col 3): x 26..33, y 21..23; (row 0, col 2): x 18..25, y 18..20
    _fly(m, 24, 22, 1, -1)
    _, r, t, _ = m.process(AM.NOOP)
    # tick 1: the box at tx = 25 overlaps (1, 3): 50, vx = -1; by 21.  tick 2: bx 23; the box at ty = 20 overlaps (0, 2): 70
    assert (m.bx, m.by, m.vx, m.vy, m.bricks) == (23, 21, -1, 1, 1 << 9) and (r, t) == (120, False)
    assert m.events >= {"two_rewards", "brick_x", "brick_y"} and m.last_reward == 120 and m.ticks == 2


def test_the_frame_and_the_pixel_change_are_those_of_the_end_records():
    """Only the two end records of a step are drawn: a return in tick 1 and a tick of flight after it."""
    m = _fly(_model(game="duel", action_repeat=2, ball_speed=1, opponent_speed=0), 10, 76, -1, 1)
    m.px = 2
    m.frame = m.render()
    before = m.frame.copy()
    _, r, t, pc = m.process(AM.NOOP)    # tick 1: bx 9, the return (by stays 76, vy -1, vx by the segment); tick 2: up
    assert m.vy == -1 and m.by == 75 and "paddle_2" in m.events
    np.testing.assert_array_equal(pc, AM.pixel_change(m.render(), before))
    np.testing.assert_array_equal(m.frame, RM.frame_of(m.c, m.record()))
    for game in GAMES:
        m = _model(game=game, action_repeat=8, serve_wait=0)
        _, _, _, pc = m.process(AM.NOOP)
        assert pc.sum() == 0 and m.wait == 8


# ---- the traces of the GPU test ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(RM.TRACE_EVENTS)))
def test_each_trace_holds_its_events(k):
    conf, tr = RM.trace_config(k), RM.run_trace(k)
    assert RM.TRACE_EVENTS[k] <= tr["events"], RM.TRACE_EVENTS[k] - tr["events"]
    scripted = k >= len(RM.TRACE_SETTINGS)
    assert tr["acts"].shape == ((RM.SCRIPTED_STEPS, RM.SCRIPTED_B) if scripted else (RM.TRACE_STEPS, RM.TRACE_B))
    assert conf.action_repeat == (4 if scripted else (2, 4, 8)[k % 3])
    if not scripted:
        assert 0.88 < tr["active"].mean() < 0.92
    live = tr["active"] != 0
    assert (tr["terminal"][live] == 1).any() and tr["episode"].max() > 0 and (tr["records"][:, :, 13:] == 0).all()
    if conf.return_reward:
        assert "returned" in tr["events"]


def test_the_traces_together_hold_every_event_and_the_settings_the_gpu_test_needs():
    seen = set()
    for k in range(len(RM.TRACE_EVENTS)):
        seen |= RM.TRACE_EVENTS[k]
    assert RM.NEW_EVENTS <= seen and RM.EVERY_EVENT <= seen, (RM.NEW_EVENTS | RM.EVERY_EVENT) - seen
    confs = [RM.trace_config(k) for k in range(len(RM.TRACE_SETTINGS))]
    for game in GAMES:
        assert sorted(c.action_repeat for c in confs if c.game == game) == [2, 4, 8]
        assert any(c.return_reward > 0 and c.ball_speed == 4 for c in confs if c.game == game)
    assert [c.game for c in (RM.trace_config(6), RM.trace_config(7))] == ["breakout", "duel"]
