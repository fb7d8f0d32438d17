"""CPU tests of the device arcade: config validation, the block, the header's constants, the entries' host
checks, and the rules on the host model of tests/arcade_model.py, worked by hand."""
import os
import re

import numpy as np
import pytest

try:
    import arcade_model as AM
    from maze_model import philox4x32_10
except ImportError:            # imported as tests.<module>
    from tests import arcade_model as AM
    from tests.maze_model import philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = (1 << 60) - 1


def _conf(**kw):
    from unreal_amd.environment.arcade_environment import ArcadeConfig
    return ArcadeConfig(**kw)


def _model(seed=0, g=0, **kw):
    return AM.HostBreakout(_conf(**kw), g, seed)


def _fly(m, bx, by, vx, vy, bricks=None):
    m.bx, m.by, m.vx, m.vy, m.wait = bx, by, vx, vy, -1
    if bricks is not None:
        m.bricks = bricks
    m.frame = m.render()
    return m


# ---- config ---------------------------------------------------------------------------------------------------------------
BAD = [dict(game="pong"), dict(rows=0), dict(rows=7), dict(rows=True), dict(rows=2.0), dict(rows="3"),
       dict(rows=2, row_rewards=(1,)), dict(rows=2, row_rewards=(1, 2, 3)), dict(rows=2, row_rewards=(1, -1)),
       dict(rows=2, row_rewards=(1, 101)), dict(rows=2, row_rewards=(1, 1.5)), dict(rows=2, row_rewards=(True, 1)),
       dict(rows=1, row_rewards=5), dict(rows=2, row_rewards="11"),
       dict(paddle_width=2), dict(paddle_width=26), dict(paddle_width=11), dict(paddle_width=12.0), dict(paddle_width=True),
       dict(paddle_speed=0), dict(paddle_speed=9), dict(paddle_speed=False), dict(paddle_speed=1.0),
       dict(ball_speed=0), dict(ball_speed=5), dict(ball_speed=True), dict(ball_speed=2.5),
       dict(lives=0), dict(lives=6), dict(lives=True), dict(lives=3.0),
       dict(serve_wait=-1), dict(serve_wait=256), dict(serve_wait=False), dict(serve_wait=8.0),
       dict(life_reward=1), dict(life_reward=-101), dict(life_reward=False), dict(life_reward=-1.0),
       dict(max_episode_steps=0), dict(max_episode_steps=2 ** 31), dict(max_episode_steps=True),
       dict(max_episode_steps=100.0), dict(max_episode_steps=None)]


@pytest.mark.parametrize("kw", BAD, ids=[repr(sorted(k.items())) for k in BAD])
def test_a_setting_outside_its_range_is_a_value_error(kw):
    from unreal_amd.environment.environment import Environment
    with pytest.raises(ValueError):
        Environment.register_arcade_config("arcade_bad", **kw)
    assert "arcade_bad" not in Environment.ARCADE_CONFIG


def test_the_edges_of_every_range_are_accepted_and_registered():
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.arcade_environment import ArcadeConfig
    for kw in (dict(rows=1, paddle_width=4, paddle_speed=1, ball_speed=1, lives=1, serve_wait=0, life_reward=-100,
                    max_episode_steps=1, row_rewards=[0]),
               dict(rows=6, paddle_width=24, paddle_speed=8, ball_speed=4, lives=5, serve_wait=255, life_reward=0,
                    max_episode_steps=2 ** 31 - 1, row_rewards=np.array([100, 0, 1, 2, 3, 4]))):
        ArcadeConfig(**kw)
    try:
        Environment.register_arcade_config("arcade_ok")
        conf = Environment.ARCADE_CONFIG["arcade_ok"]
        assert isinstance(conf, ArcadeConfig) and conf.row_rewards == (1,) * 6 and conf.max_episode_steps == 5000
        assert (conf.rows, conf.paddle_width, conf.paddle_speed, conf.ball_speed, conf.lives, conf.serve_wait,
                conf.life_reward) == (6, 12, 3, 2, 3, 8, 0)
        Environment.action_size = 18                       # another environment's cached count is not the arcade's
        assert Environment.get_action_size("arcade", "arcade_ok") == 4
        assert Environment.action_size == 18
        assert Environment.get_objective_size("arcade", "arcade_ok") == 0
        assert Environment.get_image_shape("arcade", "arcade_ok") == [84, 84]
        with pytest.raises(KeyError):
            Environment.get_action_size("arcade", "arcade_unknown")
    finally:
        Environment.ARCADE_CONFIG.pop("arcade_ok", None)
        Environment.action_size = -1


def test_block_words_by_value():
    c = _conf(rows=3, row_rewards=(7, 4, 1), paddle_width=16, paddle_speed=5, ball_speed=3, lives=4, serve_wait=20,
              life_reward=-9, max_episode_steps=123456)
    b = c.block(0xFEDCBA9876543210)
    assert b.dtype == np.int32 and b.shape == (24,)
    want = [1, 0, 3, 123456, 0x76543210, np.int32(-0x01234568), 16, 5, 3, 4, 20, -9, 7, 4, 1] + [0] * 9
    assert b.tolist() == [int(w) for w in want]
    assert _conf().block(5).tolist() == [1, 0, 6, 5000, 5, 0, 12, 3, 2, 3, 8, 0, 1, 1, 1, 1, 1, 1] + [0] * 6
    assert _conf(max_episode_steps=2 ** 31 - 1).block(0)[3] == 2 ** 31 - 1


def test_header_constants_are_the_python_ones():
    from unreal_amd import ops
    src = open(os.path.join(ROOT, "include", "unreal_hip.h")).read()
    defs = dict(re.findall(r"#define (UNREAL_ARCADE_\w+) (\w+)", src))
    assert int(defs["UNREAL_ARCADE_BREAKOUT"]) == ops.ARCADE_BREAKOUT == 1
    assert int(defs["UNREAL_ARCADE_CFG_WORDS"]) == ops.ARCADE_CFG_WORDS == 24 == len(_conf().block(0))
    assert int(defs["UNREAL_ARCADE_RECORD"]) == ops.ARCADE_RECORD == 16 == len(_model().record())
    assert int(defs["UNREAL_ARCADE_SERVE_STREAM"], 16) == ops.ARCADE_SERVE_STREAM == AM.SERVE_STREAM
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("unreal_arcade_reset", "unreal_arcade_step", "unreal_arcade_rollout_step", "unreal_arcade_policy_rollout_step"):
        assert name in text and name in src


def test_entries_refuse_bad_arguments_without_a_launch():
    """Fake device pointers: every call below is refused by the host check, so none reaches a kernel."""
    from unreal_amd.build import build_library
    from unreal_amd import _lib
    build_library(verbose=False)
    L = _lib.lib()
    dev = 1 << 20
    tail = [dev, 0, dev, dev, dev]                       # cfg, actor_base, ep_steps, episode, records
    reset = [4, 3, None, None, dev, dev, dev, dev]       # B, H1, mask, pos, last_action, last_reward, count, frames
    ring = [None] + [dev] * 10 + [None, None] + [dev] * 3    # pos .. score_valid
    step = [4, 3, dev, None] + ring + [1, 1]
    roll = [4, 3, dev] + ring + [dev] * 4 + [None, None, 0, 0, 4, 0]
    pol = [4, 3, dev, 256] + [dev] * 8 + ring + [dev] * 4 + [None, None, 0, 0, 4, 0]
    f = L._fn

    def bad_tails():
        yield [None, 0, dev, dev, dev]                   # a null block
        yield [dev + 2, 0, dev, dev, dev]                # a misaligned one
        yield [dev, -1, dev, dev, dev]
        for k in (2, 3, 4):                              # no ep_steps / episode / records
            yield [None if i == k else w for i, w in enumerate(tail)]

    for t in bad_tails():
        assert f["unreal_arcade_reset"](*reset, *t, None) == -22, t
        assert f["unreal_arcade_step"](*step, *t, None) == -22, t
        assert f["unreal_arcade_rollout_step"](*roll, *t, None) == -22, t
        assert f["unreal_arcade_policy_rollout_step"](*pol, *t, None) == -22, t
    # B, H1, frames alignment
    assert f["unreal_arcade_reset"](0, 3, *reset[2:], *tail, None) == -22
    assert f["unreal_arcade_reset"](4, 1, *reset[2:], *tail, None) == -22
    assert f["unreal_arcade_reset"](*reset[:7], dev + 8, *tail, None) == -22
    assert f["unreal_arcade_step"](*step[:2], None, *step[3:], *tail, None) == -22          # no actions
    # A != 4 in both rollout entries; a next_lar row too short for A + 1 columns
    for A in (0, 3, 6, 18):
        assert f["unreal_arcade_rollout_step"](*roll[:-2], A, 0, *tail, None) == -22, A
        assert f["unreal_arcade_policy_rollout_step"](*pol[:-2], A, 0, *tail, None) == -22, A
    assert f["unreal_arcade_rollout_step"](*roll[:-5], dev, 260, 256, 4, 0, *tail, None) == -22
    assert f["unreal_arcade_policy_rollout_step"](*pol[:3], 255, *pol[4:], *tail, None) == -22       # ldx < 256
    assert f["unreal_arcade_policy_rollout_step"](*pol[:4], None, *pol[5:], *tail, None) == -22      # no Wp
    with pytest.raises(_lib.UnrealLibError):
        L.call("unreal_arcade_step", *step, None, 0, dev, dev, dev, None)


# ---- the rules, by hand ------------------------------------------------------------------------------------------------------
def test_serve_by_fire_and_at_serve_wait():
    seed, g = 0x1234567890, 5
    m = _model(seed=seed, g=g)
    assert (m.px, m.wait, m.lives, m.bricks, m.episode) == (36, 0, 3, FULL, 0)
    _, r, t, _ = m.process(AM.FIRE)
    u = philox4x32_10((g, 0, AM.SERVE_STREAM, 0), (seed & 0xFFFFFFFF, seed >> 32))
    assert (m.bx, m.by, m.vy, m.wait, m.serve_index) == (2 + 2 * (int(u[0]) % 39), 40, 1, -1, 1)
    assert m.vx == (1 if int(u[1]) & 1 else -1) and (r, t) == (0, False) and m.events == {"serve_fire"}
    assert m.bx % 2 == 0 and 2 <= m.bx <= 78
    # the ball did not move in the serving step; in the next it makes ball_speed = 2 micro-steps
    bx = m.bx
    m.process(AM.NOOP)
    assert m.by == 42 and abs(m.bx - bx) <= 2
    # serve_wait = 3: three steps count, the fourth serves; the second serve of an episode uses serve index 1
    m = _model(seed=seed, g=g, serve_wait=3)
    for k in range(3):
        m.process(AM.NOOP)
        assert m.wait == k + 1 and not m.events
    m.serve_index = 1
    m.process(AM.LEFT)
    u = philox4x32_10((g, 0, AM.SERVE_STREAM, 1), (seed & 0xFFFFFFFF, seed >> 32))
    assert m.events == {"serve_auto"} and (m.wait, m.bx, m.px, m.serve_index) == (-1, 2 + 2 * (int(u[0]) % 39), 33, 2)
    # serve_wait = 0: only fire serves
    m = _model(serve_wait=0)
    for _ in range(300):
        m.process(AM.NOOP)
    assert m.wait == 300 and m.serve_index == 0


def test_side_walls_and_top_wall():
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
    m = _fly(_model(ball_speed=1, rows=1), 40, 6, 1, -1)
    m.process(AM.NOOP)
    assert (m.bx, m.by, m.vx, m.vy) == (41, 6, 1, 1) and m.events == {"wall_top"}


REWARDS = (1, 2, 3, 4, 5, 6)


def test_brick_hits_in_x_and_in_y_clear_the_lowest_bit_and_turn_that_axis():
    # the ball sits in the hole of brick (2, 0) (bit 20: x 2..9, y 24..26); to its right brick (2, 1), bit 21
    m = _fly(_model(ball_speed=1, row_rewards=REWARDS), 8, 25, 1, -1, FULL & ~(1 << 20))
    _, r, t, _ = m.process(AM.NOOP)
    assert m.bricks == FULL & ~(3 << 20) and r == 3 and not t and m.events == {"brick_x"}
    assert (m.bx, m.by, m.vx, m.vy) == (8, 24, -1, -1) and m.totals == [1, 0, 0]
    # the box at (9, 26) overlaps bricks 21 (row 2) and 31 (row 3): the lower bit goes
    m = _fly(_model(ball_speed=1, row_rewards=REWARDS), 8, 26, 1, -1, FULL & ~(1 << 20) & ~(1 << 30))
    _, r, _, _ = m.process(AM.NOOP)
    assert m.bricks == FULL & ~(3 << 20) & ~(1 << 30) and r == 3 and (m.bx, m.by, m.vx, m.vy) == (8, 25, -1, -1)
    # from below: y 35 is the last line of row 5; x 21, 22 lie in column 2: bit 52
    m = _fly(_model(ball_speed=1, row_rewards=REWARDS), 20, 36, 1, -1)
    _, r, t, _ = m.process(AM.NOOP)
    assert m.bricks == FULL & ~(1 << 52) and r == 6 and not t and m.events == {"brick_y"}
    assert (m.bx, m.by, m.vx, m.vy) == (21, 36, 1, 1)
    # straddling columns 2 and 3 from below: bits 52 and 53, the lower one goes
    m = _fly(_model(ball_speed=1, row_rewards=REWARDS), 24, 36, 1, -1)
    m.process(AM.NOOP)
    assert m.bricks == FULL & ~(1 << 52) and m.bx == 25


def test_two_bricks_in_one_step():
    m = _fly(_model(ball_speed=1, row_rewards=REWARDS), 8, 25, 1, 1, FULL & ~(1 << 20))
    _, r, _, _ = m.process(AM.NOOP)
    assert m.bricks == FULL & ~(3 << 20) & ~(1 << 30) and r == 3 + 4
    assert m.events == {"brick_x", "brick_y", "two_bricks"} and (m.bx, m.by, m.vx, m.vy) == (8, 25, -1, -1)
    assert m.totals == [2, 0, 0]


@pytest.mark.parametrize("bx,vx", [(35, -2), (37, -2), (38, -1), (40, -1), (41, 1), (43, 1), (44, 2), (47, 2)])
def test_the_four_paddle_segments(bx, vx):
    # paddle x 36..47, middle 42: d = bx + 1 - 42
    m = _fly(_model(ball_speed=1), bx - 1, 76, 1, 1)
    _, r, t, _ = m.process(AM.NOOP)
    assert (m.bx, m.by, m.vx, m.vy) == (bx, 76, vx, -1) and (r, t) == (0, False)
    assert m.events == {"paddle_%d" % ((-2, -1, 1, 2).index(vx))}


def test_the_paddle_collides_only_at_its_top():
    for bx in (34, 48):                                   # beside the paddle: on it goes
        m = _fly(_model(ball_speed=1), bx - 1, 76, 1, 1)
        m.process(AM.NOOP)
        assert (m.bx, m.by, m.vy) == (bx, 77, 1) and not m.events
    m = _fly(_model(ball_speed=1), 40, 77, 1, 1)          # already below the top line: it passes through
    m.process(AM.NOOP)
    assert (m.by, m.vy) == (78, 1) and not m.events


def test_a_miss_costs_a_life_and_the_last_life_ends_the_episode():
    m = _fly(_model(life_reward=-5), 10, 82, 1, 1)
    _, r, t, _ = m.process(AM.NOOP)
    assert (m.lives, m.wait, r, t) == (2, 0, -5, False) and m.events == {"life_lost"} and m.totals == [0, 1, 0]
    assert (m.bx, m.by) == (11, 82)                       # the second micro-step did not run
    assert (m.frame == AM.WHITE).all(2).sum() == 4 * 2    # two lives, no ball
    m.process(AM.NOOP)
    assert m.wait == 1
    m = _fly(_model(life_reward=-5), 10, 82, 1, 1)
    m.lives = 1
    _, r, t, _ = m.process(AM.NOOP)
    assert (m.lives, r, t) == (0, -5, True) and m.events == {"life_lost", "end_lives"} and not m.success


def test_the_last_brick_is_a_success_terminal():
    m = _fly(_model(rows=1, row_rewards=(9,)), 28, 21, 1, -1, 1 << 3)      # brick (0, 3): x 26..33, y 18..20
    _, r, t, _ = m.process(AM.NOOP)
    assert m.bricks == 0 and (r, t, m.success) == (9, True, True) and m.events == {"brick_y", "end_clear"}
    assert (m.bx, m.by, m.vy) == (29, 21, 1) and m.totals == [1, 0, 1]    # the second micro-step did not run
    m.reset()
    assert m.bricks == (1 << 10) - 1 and m.episode == 1 and m.totals == [1, 0, 1] and (m.bx, m.by, m.vx, m.vy) == (0, 0, 0, 0)


def test_time_out():
    m = _model(max_episode_steps=3)
    out = [m.process(AM.NOOP)[1:3] for _ in range(3)]
    assert out == [(0, False), (0, False), (0, True)] and m.events == {"end_timeout"} and not m.success
    m.reset()
    assert m.ep_steps == 0 and not m.process(AM.NOOP)[2]


@pytest.mark.parametrize("kw", [dict(), dict(rows=2, lives=5, paddle_width=24), dict(rows=1, lives=1, paddle_width=4)])
def test_reset_frame_pixel_counts(kw):
    m = _model(**kw)
    c = m.c
    count = lambda colour: int((m.frame == colour).all(2).sum())
    assert count(AM.BORDER) == 816 - 4 * c.lives
    assert count(AM.WHITE) == 4 * c.lives                                  # the lives; no ball
    assert count(AM.PADDLE) == 2 * c.paddle_width + 240                    # the top row of bricks has the paddle's colour
    for r in range(1, c.rows):
        assert count(AM.ROW_COLOURS[r]) == 240
    assert count((0, 0, 0)) == 84 * 84 - 816 - 240 * c.rows - 2 * c.paddle_width
    assert (m.frame[78:80, 42 - c.paddle_width // 2:42 + c.paddle_width // 2] == AM.PADDLE).all()


def test_pixel_change_of_a_paddle_move_by_hand():
    m = _model()
    _, _, _, pc = m.process(AM.RIGHT)                   # x 36..38 go black, x 48..50 appear: 344 per pixel, rows 78, 79
    want = np.zeros((20, 20), np.float32)
    # crop coordinates x - 2 = 34, 35 | 36 and 46, 47 | 48; y - 2 = 76, 77: block row 19
    want[19, 8] = want[19, 11] = np.float32(4 * 344 / 12240.0)
    want[19, 9] = want[19, 12] = np.float32(2 * 344 / 12240.0)
    np.testing.assert_array_equal(pc, want)
    assert m.px == 39 and pc.dtype == np.float32


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


@pytest.mark.parametrize("k", range(len(AM.TRACE_SETTINGS)))
def test_the_random_traces_hold_the_events_the_gpu_test_asserts(k):
    acts, active = AM.trace_inputs(k)
    models = AM.host_batch(_conf(**AM.TRACE_SETTINGS[k]), AM.TRACE_B, AM.TRACE_SEED, frames=False)
    seen = _events_of(models, AM.TRACE_STEPS, lambda s, b, m: acts[s, b] if active[s, b] else None)
    assert AM.TRACE_EVENTS[k] <= seen, AM.TRACE_EVENTS[k] - seen
    assert not active.all() and active.mean() > 0.8


def test_the_traces_together_hold_every_event():
    models = AM.host_batch(_conf(**AM.SCRIPTED_SETTING), AM.SCRIPTED_B, AM.TRACE_SEED, frames=False)
    seen = _events_of(models, AM.SCRIPTED_STEPS, lambda s, b, m: AM.follow_ball(m))
    assert AM.SCRIPTED_EVENTS <= seen, AM.SCRIPTED_EVENTS - seen
    every = {"wall_left", "wall_right", "wall_top", "brick_x", "brick_y", "two_bricks", "paddle_0", "paddle_1", "paddle_2",
             "paddle_3", "life_lost", "end_lives", "end_clear", "end_timeout", "serve_fire", "serve_auto"}
    assert set().union(AM.SCRIPTED_EVENTS, *AM.TRACE_EVENTS) == every
