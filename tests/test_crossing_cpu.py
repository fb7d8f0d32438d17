"""CPU tests of the device arcade's crossing game: config validation with the cross-game keywords in both
directions between the four games, the block by value next to the unchanged blocks of the other three, the header's
constants, the reset draw's key layout, and the rules on the host model of tests/crossing_model.py, worked by hand; then the
events of the traces tests/test_crossing_gpu.py compares."""
import os
import re

import numpy as np
import pytest

try:
    import arcade_model as AM
    import crossing_model as CM
    from philox_model import philox4x32_10_raw as philox_ref
except ImportError:            # imported as tests.<module>
    from tests import arcade_model as AM
    from tests import crossing_model as CM
    from tests.philox_model import philox4x32_10_raw as philox_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOOP, FORWARD, RIGHT, LEFT = AM.NOOP, CM.FORWARD, AM.RIGHT, AM.LEFT
ONE_PARKED = [(1, 0, 1, 1)]


def _conf(**kw):
    from unreal_amd.environment.arcade_environment import ArcadeConfig
    kw.setdefault("game", "crossing")
    return ArcadeConfig(**kw)


def _model(seed=0, g=0, **kw):
    return CM.HostCrossing(_conf(**kw), g, seed)


def _count(frame, colour):
    return int((frame == colour).all(2).sum())


def _place(m, lane, x):
    """Move the cars of `lane` so that one starts at screen column x."""
    m.offsets[lane] = (x + CM.SHIFT) % CM.TRACK


# ---- config ---------------------------------------------------------------------------------------------------------------
LANE = (2, 1, 1, 1)
CROSS_BAD = [dict(lanes=[]), dict(lanes=[LANE] * 9), dict(lanes=LANE), dict(lanes="2111"), dict(lanes=3), dict(lanes=[(2, 1, 1)]),
             dict(lanes=[(3, 1, 1, 1)]), dict(lanes=[(0, 1, 1, 1)]), dict(lanes=[(8, 1, 1, 1)]), dict(lanes=[(True, 1, 1, 1)]),
             dict(lanes=[(2, 5, 1, 1)]), dict(lanes=[(2, -1, 1, 1)]), dict(lanes=[(2, 1.0, 1, 1)]), dict(lanes=[(2, 1, 0, 1)]),
             dict(lanes=[(2, 1, 5, 1)]), dict(lanes=[(2, 1, True, 1)]), dict(lanes=[(2, 1, 1, 0)]), dict(lanes=[(2, 1, 1, 2)]),
             dict(lanes=[(2, 1, 1, -2)]), dict(lanes=[(2, 1, 1, 1.0)]), dict(lanes=[LANE, "2111"]),
             dict(car_length=3), dict(car_length=17), dict(car_length=True), dict(car_length=8.0),
             dict(knock_back=0), dict(knock_back=71), dict(knock_back=True), dict(knock_back=8.0), dict(knock_back="8"),
             dict(crossings=-1), dict(crossings=100), dict(crossings=False), dict(crossings=2.0),
             dict(cross_reward=-1), dict(cross_reward=101), dict(cross_reward=True), dict(cross_reward=1.0),
             dict(hit_reward=1), dict(hit_reward=-101), dict(hit_reward=False), dict(hit_reward=-1.0),
             # the shared settings keep Breakout's ranges
             dict(paddle_width=2), dict(paddle_width=26), dict(paddle_width=11), dict(paddle_width=True),
             dict(paddle_speed=0), dict(paddle_speed=9), dict(paddle_speed=1.0),
             dict(ball_speed=0), dict(ball_speed=5), dict(ball_speed=True),
             dict(serve_wait=-1), dict(serve_wait=256), dict(serve_wait=8.0),
             dict(max_episode_steps=0), dict(max_episode_steps=2 ** 31), dict(max_episode_steps=None),
             dict(action_repeat=0), dict(action_repeat=9), dict(action_repeat=True),
             # no paddle returns a ball here
             dict(return_reward=1), dict(return_reward=100), dict(return_reward=-1), dict(return_reward=False),
             # the other games' own settings, even at their defaults
             dict(rows=6), dict(row_rewards=(1,) * 6), dict(lives=3), dict(life_reward=0), dict(points=5),
             dict(opponent_width=12), dict(opponent_speed=2), dict(win_reward=1), dict(lose_reward=-1), dict(alien_rows=3),
             dict(alien_rewards=(1, 1, 1)), dict(march_period=4), dict(descend=4), dict(bomb_period=12), dict(bomb_speed=1)]
OWN = [dict(lanes=[LANE]), dict(car_length=8), dict(knock_back=8), dict(crossings=0), dict(cross_reward=1), dict(hit_reward=0)]
BAD = [dict(game="crossing", **kw) for kw in CROSS_BAD] + \
      [dict(game="frogger"), dict(game="Crossing"), dict(game=7)] + \
      [dict(game=g, **kw) for g in ("breakout", "duel", "invaders") for kw in OWN] + OWN


@pytest.mark.parametrize("kw", BAD, ids=[repr(sorted(k.items())) for k in BAD])
def test_a_setting_outside_its_range_or_of_another_game_is_a_value_error(kw):
    from unreal_amd.environment.environment import Environment
    with pytest.raises(ValueError):
        Environment.register_arcade_config("crossing_bad", **kw)
    assert "crossing_bad" not in Environment.ARCADE_CONFIG


def test_the_edges_of_every_range_are_accepted_and_registered():
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment import arcade_environment as AE
    from unreal_amd import ops
    # the three pinned dictionaries stay what they are; crossing comes in through tables of its own
    assert AE.GAMES == {"breakout": 1, "duel": 3} and AE.GAME_IDS == {"breakout": 1, "duel": 3, "invaders": 5}
    assert sorted(AE.GAME_SETTINGS) == ["breakout", "duel", "invaders"]
    assert AE.ALL_GAME_IDS == dict(AE.GAME_IDS, crossing=7) and ops.ARCADE_CROSSING == 7
    assert AE.CROSSING_SETTINGS == dict(lanes=None, car_length=8, knock_back=8, crossings=0, cross_reward=1, hit_reward=0)
    for kw in (dict(lanes=[(1, 0, 1, -1)], car_length=4, knock_back=1, crossings=0, cross_reward=0, hit_reward=-100,
                    paddle_width=4, paddle_speed=1, ball_speed=1, serve_wait=0, max_episode_steps=1, action_repeat=1,
                    return_reward=0),
               dict(lanes=[(4, 4, 4, 1)] * 8, car_length=16, knock_back=70, crossings=99, cross_reward=100, hit_reward=0,
                    paddle_width=24, paddle_speed=8, ball_speed=4, serve_wait=255, max_episode_steps=2 ** 31 - 1,
                    action_repeat=8),
               dict(lanes=([np.int64(2), np.int32(3), 2, np.int64(-1)],), knock_back=np.int32(16), crossings=np.int64(5))):
        AE.ArcadeConfig(game="crossing", **kw)
    try:
        Environment.register_arcade_config("crossing_ok", game="crossing")
        conf = Environment.ARCADE_CONFIG["crossing_ok"]
        assert isinstance(conf, AE.ArcadeConfig) and conf.game == "crossing" and conf.action_size == 4
        assert (conf.lanes, conf.car_length, conf.knock_back, conf.crossings, conf.cross_reward, conf.hit_reward,
                conf.paddle_width, conf.paddle_speed, conf.ball_speed, conf.serve_wait, conf.max_episode_steps,
                conf.action_repeat, conf.return_reward) == (AE.DEFAULT_LANES, 8, 8, 0, 1, 0, 12, 3, 2, 8, 5000, 1, 0)
        # the documented default: eight lanes, alternating directions, mixed speeds
        assert len(conf.lanes) == 8 and [l[3] for l in conf.lanes] == [1, -1] * 4 and len({l[1] for l in conf.lanes}) > 2
        assert not hasattr(conf, "rows") and not hasattr(conf, "points") and not hasattr(conf, "lives")
        assert Environment.get_action_size("arcade", "crossing_ok") == 4
        assert Environment.get_objective_size("arcade", "crossing_ok") == 0
        # the other games' defaults are untouched
        conf = AE.ArcadeConfig()
        assert (conf.game, conf.rows, conf.lives, conf.paddle_width) == ("breakout", 6, 3, 12) and not hasattr(conf, "lanes")
        assert AE.ArcadeConfig(game="invaders").lives == 3 and not hasattr(AE.ArcadeConfig(game="duel"), "knock_back")
        mix = AE.ArcadeMix([AE.ArcadeConfig(), conf, AE.ArcadeConfig(game="crossing", paddle_width=4)])
        assert mix.task_names == ("0:breakout", "1:breakout", "2:crossing") and mix.block(3)[48] == 7
    finally:
        Environment.ARCADE_CONFIG.pop("crossing_ok", None)


def test_the_block_by_value():
    c = _conf(lanes=[(4, 3, 2, 1), (1, 0, 1, -1), (2, 4, 4, 1)], car_length=13, knock_back=70, crossings=9, cross_reward=55,
              hit_reward=-7, max_episode_steps=123456, paddle_width=16, paddle_speed=5, ball_speed=3, serve_wait=20,
              action_repeat=4)
    b = c.block(0xFEDCBA9876543210)
    assert b.dtype == np.int32 and b.shape == (24,)
    cars, speed, period, right = 2 | 0 << 2 | 1 << 4, 3 | 0 << 3 | 4 << 6, 1 | 0 << 2 | 3 << 4, 1 | 0 << 1 | 1 << 2
    want = [7, 3, 3, 123456, 0x76543210, np.int32(-0x01234568), 16, 5, 3, 9, 20, -7, 55, 70, 13, cars, speed, period, 0, right,
            0, 0, 0, 0]
    assert b.tolist() == [int(w) for w in want]
    # the default: eight lanes (cars 2 1 4 2 2 1 4 2, speeds 1 2 1 3 1 4 1 2, periods 1 1 2 1 1 1 3 1, right left ...)
    d = _conf().block(5).tolist()
    assert d[:15] == [7, 0, 8, 5000, 5, 0, 12, 3, 2, 0, 8, 0, 1, 8, 8] and d[18] == 0 and d[20:] == [0] * 4
    assert d[15] == sum(v << (2 * l) for l, v in enumerate((1, 0, 2, 1, 1, 0, 2, 1)))
    assert d[16] == sum(v << (3 * l) for l, v in enumerate((1, 2, 1, 3, 1, 4, 1, 2)))
    assert d[17] == sum(v << (2 * l) for l, v in enumerate((0, 0, 1, 0, 0, 0, 2, 0))) and d[19] == 0b01010101
    # the other games' blocks are what they were
    assert _conf(game="breakout").block(5).tolist() == [1, 0, 6, 5000, 5, 0, 12, 3, 2, 3, 8, 0, 1, 1, 1, 1, 1, 1] + [0] * 6
    assert _conf(game="duel").block(5).tolist() == [3, 0, 5, 5000, 5, 0, 12, 3, 2, 12, 8, -1, 1, 2] + [0] * 10
    assert _conf(game="invaders").block(5).tolist() == [5, 0, 3, 5000, 5, 0, 12, 3, 2, 3, 8, 0, 1, 1, 1, 0, 4, 4, 0, 12, 1, 0, 0, 0]


def test_header_constants_and_documents():
    from unreal_amd import ops
    src = open(os.path.join(ROOT, "include", "unreal_hip.h")).read()
    defs = dict(re.findall(r"#define (UNREAL_ARCADE_\w+) (\w+)", src))
    assert int(defs["UNREAL_ARCADE_CROSSING"]) == ops.ARCADE_CROSSING == 7
    assert [int(defs["UNREAL_ARCADE_" + g]) for g in ("BREAKOUT", "DUEL", "INVADERS")] == [1, 3, 5]
    assert int(defs["UNREAL_ARCADE_CFG_WORDS"]) == ops.ARCADE_CFG_WORDS == 24 == len(_conf().block(0))
    assert int(defs["UNREAL_ARCADE_RECORD"]) == ops.ARCADE_RECORD == 16 == len(_model().record())
    assert int(defs["UNREAL_ARCADE_LANE_STREAM"], 16) == ops.ARCADE_LANE_STREAM == CM.LANE_STREAM == 0x43524F53
    assert len({CM.LANE_STREAM, AM.SERVE_STREAM, ops.ARCADE_BOMB_STREAM}) == 3
    assert src.count("[1] action_repeat - 1") == 2           # (tests/test_arcade_repeat_cpu.py counts the literal)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ("UNREAL_ARCADE_CROSSING", "UNREAL_ARCADE_LANE_STREAM", "knock_back", "car_length"):
        assert word in text and word in src, word
    kernel = open(os.path.join(ROOT, "unreal_amd", "csrc", "arcade.hip")).read()
    assert "kArcadeCrossing = 7" in kernel and "0x%08Xu" % CM.LANE_STREAM in kernel
    for name in ("arcade_step_kernel", "arcade_step_tl_kernel", "arcade_reset_kernel", "arcade_mix_step_kernel",
                 "arcade_mix_step_tl_kernel", "arcade_mix_reset_kernel"):
        body = kernel[kernel.index("void %s(" % name):]
        assert "kArcadeCrossing" in body[:body.index("\n}\n")], name
    for name in ("arcade_selfplay_step_kernel", "arcade_versus_step_kernel"):      # no branch there
        body = kernel[kernel.index("void %s(" % name):]
        assert "kArcadeCrossing" not in body[:body.index("\n}\n")], name
    assert "\n## 7x. " in open(os.path.join(ROOT, "DESIGN.md")).read() and "crossing" in open(os.path.join(ROOT, "README.md")).read()


# ---- the rules, by hand ------------------------------------------------------------------------------------------------------
def test_the_reset_draws_key_layout_against_the_philox_model():
    """key = seed (lo, hi), counter = (actor, episode, stream constant, 0): the model's offsets are the bytes of the
    reference Philox of tests/philox_model.py on those words, seven bits each, and differ per actor, episode and seed."""
    seed = 0xFEDCBA9876543210
    key = (seed & 0xFFFFFFFF, seed >> 32)
    seen = set()
    for g, episodes in ((0, 1), (199, 3), (2 ** 31 - 1, 2)):
        m = CM.HostCrossing(_conf(), g, seed, frames=False)
        for ep in range(episodes):
            u = philox_ref((g, ep, CM.LANE_STREAM, 0), key)
            assert m.episode == ep and m.offsets == [(int(u[l // 4]) >> (8 * (l % 4))) & 127 for l in range(8)]
            rec = m.record()
            assert (int(rec[5]) & 0xFFFFFFFF, int(rec[6]) & 0xFFFFFFFF) == (int(u[0]) & 0x7F7F7F7F, int(u[1]) & 0x7F7F7F7F)
            assert [int(x) for x in u] != [int(x) for x in philox_ref((g, ep, AM.SERVE_STREAM, 0), key)]
            seen.add(tuple(m.offsets))
            m.reset()
    assert len(seen) == 6
    assert CM.HostCrossing(_conf(), 0, seed + 1, frames=False).offsets != CM.HostCrossing(_conf(), 0, seed, frames=False).offsets
    # a one-lane game draws all eight offsets all the same: the game stays a function of the block's seed alone
    assert CM.HostCrossing(_conf(lanes=ONE_PARKED), 5, seed, frames=False).offsets == \
        CM.HostCrossing(_conf(), 5, seed, frames=False).offsets


def test_the_reset_state_and_record():
    m = _model(paddle_width=4, seed=3, g=2)
    assert (m.px, m.py, m.stun, m.count, m.tick_counter, m.ep_steps, m.episode) == (40, 76, 0, 0, 0, 0, 0)
    rec = m.record()
    assert rec.dtype == np.int32 and rec.shape == (16,)
    assert rec[:5].tolist() == [40, 76, 0, 0, 0] and not rec[7:].any()
    m.totals = [5, 6, 7]
    m.reset()
    assert m.episode == 1 and m.record()[10:13].tolist() == [5, 6, 7]          # the totals run on
    assert _model(paddle_width=24).px == 30 and _model().px == 36


def test_the_walker_moves_and_is_clamped():
    m = _model(paddle_width=4, paddle_speed=3, ball_speed=2, lanes=ONE_PARKED)
    _place(m, 0, -20)
    m.tick(NOOP); assert (m.px, m.py) == (40, 76)
    m.tick(FORWARD); assert (m.px, m.py) == (40, 74)
    m.tick(RIGHT); m.tick(RIGHT); assert (m.px, m.py) == (46, 74)
    for _ in range(12):
        m.tick(RIGHT)
    assert m.px == 78 and "clamp_right" in m.events                           # 82 - w
    m.px = 4
    m.tick(LEFT); assert m.px == 2
    m.tick(LEFT); assert m.px == 2 and "clamp_left" in m.events
    assert m.count == 0 and m.totals == [0, 0, 0]


def test_lanes_move_by_their_period_direction_and_speed_and_wrap_at_the_seam():
    lanes = [(1, 4, 1, 1), (1, 3, 1, -1), (1, 2, 4, 1), (1, 0, 1, 1), (1, 1, 3, -1), (1, 1, 2, 1)]
    m = _model(lanes=lanes, paddle_width=4)
    m.offsets = [126, 1, 10, 77, 0, 127, 99, 98]
    want = list(m.offsets)
    for t in range(26):
        assert m.tick_counter == t % 12
        m.tick(NOOP)
        for l, (_, speed, period, direction) in enumerate(lanes):
            if (t % 12) % period == 0:
                want[l] = (want[l] + direction * speed) % 128
        assert m.offsets == want, t
    # the first tick moved every lane: 126 -> 2 and 1 -> 126 wrapped; the parked lane and the lanes without traffic stand
    assert m.offsets[3] == 77 and m.offsets[6:] == [99, 98]
    assert _model(lanes=lanes).tick_counter == 0


@pytest.mark.parametrize("w", [4, 24])
@pytest.mark.parametrize("dx,hit", [(-1, False), (0, True), (3, True), (7, True), (8, False)])
def test_a_hit_on_the_walkers_first_and_last_column_and_a_miss_by_one(w, dx, hit):
    """A parked car of 8 px at columns 30..37 of lane 7 (rows 68..71).  dx places the walker: dx <= 0 from the left (its last
    column at 30 + dx), dx >= 7 from the right (its first column at 30 + dx), dx = 3 inside."""
    m = _model(paddle_width=w, lanes=[(1, 0, 1, 1)] * 8, ball_speed=4, knock_back=8, hit_reward=-3, serve_wait=2, paddle_speed=1)
    for l in range(8):
        _place(m, l, -20)
    _place(m, 7, 30)
    m.px = 30 + dx - (w - 1) if dx <= 3 else 30 + dx
    m.py = 76
    assert m.tick(FORWARD) == 0 and m.py == 72                               # rows 72..75: below the lane
    r = m.tick(FORWARD)                                                      # rows 68..71
    if hit:
        assert r == -3 and m.py == 76 and m.stun == 2 and m.totals == [0, 1, 0] and "hit" in m.events
    else:
        assert r == 0 and m.py == 68 and m.stun == 0 and m.totals == [0, 0, 0]
        assert ("miss_right" if dx < 0 else "miss_left") in m.events         # (named by the side of the walker the car is on)


@pytest.mark.parametrize("py,met", [(8, False), (9, True), (12, True), (15, True), (16, False), (61, True), (64, False)])
def test_the_rows_in_which_a_lane_is_met(py, met):
    m = _model(paddle_width=4, lanes=[(1, 0, 1, 1)] * 8, hit_reward=-1)
    for l in range(8):
        _place(m, l, 39)                                                       # over the walker's columns 40..43
    m.py = py
    assert (m.tick(NOOP) == -1) == met


def test_a_car_over_the_seam_and_cars_clipped_at_the_border_hit_and_are_drawn():
    m = _model(paddle_width=4, lanes=[(1, 0, 1, 1), (2, 0, 1, 1)], car_length=16, hit_reward=-1)
    m.offsets[0] = 120                                  # track 120..127 and 0..7: screen 98..105 and -22..-15, out of the field
    m.offsets[1] = 10                                   # track 10..25 and 74..89: screen -12..3 (clipped at 2) and 52..67
    f = m.render()
    assert _count(f[12:16], AM.ROW_COLOURS[1]) == 0
    row = (f[20] == AM.ROW_COLOURS[2]).all(1)
    assert np.flatnonzero(row).tolist() == [2, 3] + list(range(52, 68)) and (f[20, :2] == AM.BORDER).all()
    m.offsets[1] = 98                                   # track 98..113 and 34..49: screen 76..91 (clipped at 81) and 12..27
    f = m.render()
    row = (f[20] == AM.ROW_COLOURS[2]).all(1)
    assert np.flatnonzero(row).tolist() == list(range(12, 28)) + list(range(76, 82)) and (f[20, 82:] == AM.BORDER).all()
    m.px, m.py = 78, 20                                 # under the drawn part of the clipped car
    assert m.tick(NOOP) == -1
    # a car over the seam inside the field: no setting puts the seam on the screen (track 0 is screen -22), so a seam car is
    # seen only where it enters at the left: track 124..11 -> screen 102..105 and -22..-11; it moves and hits like any other
    m = _model(paddle_width=4, lanes=[(1, 4, 1, 1)], car_length=16)
    m.offsets[0] = 124
    m.tick(NOOP)
    assert m.offsets[0] == 0 and "wrap_up" in m.events and sorted(m.car_columns(0)) == list(range(-22, -6))
    m = _model(paddle_width=4, lanes=[(1, 4, 1, -1)], car_length=16, hit_reward=-1)
    m.offsets[0] = 2
    m.tick(NOOP)
    assert m.offsets[0] == 126 and "wrap_down" in m.events
    assert sorted(m.car_columns(0)) == list(range(-22, -8)) + [104, 105]


def test_the_knock_back_its_clamp_and_the_stun():
    m = _model(paddle_width=4, lanes=[(1, 0, 1, 1)] * 8, knock_back=16, serve_wait=3, hit_reward=-2, ball_speed=4)
    for l in range(8):
        _place(m, l, 39)
    m.py = 47                                           # lane 4 (rows 44..47) is met
    assert m.tick(NOOP) == -2 and (m.py, m.stun) == (63, 3) and "knock_clamped" not in m.events
    # stunned inside lane 6's car (rows 60..63): no second hit, no move, the lanes go on
    for k in range(3):
        assert m.tick(FORWARD) == 0 and (m.px, m.py, m.stun) == (40, 63, 2 - k) and "stunned_in_car" in m.events
    assert m.totals == [0, 1, 0]
    assert m.tick(NOOP) == -2 and (m.py, m.stun) == (76, 3) and "knock_clamped" in m.events      # 63 + 16 = 79 -> 76
    assert m.totals == [0, 2, 0]
    # serve_wait = 0: hit again in the next tick
    m = _model(paddle_width=4, lanes=[(1, 0, 1, 1)] * 8, knock_back=1, serve_wait=0, hit_reward=-2)
    for l in range(8):
        _place(m, l, 39)
    m.py = 12
    assert [m.tick(NOOP) for _ in range(4)] == [-2, -2, -2, -2] and m.py == 16
    assert m.tick(NOOP) == 0 and m.py == 16             # rows 16..19: between the lanes


def test_a_crossing_the_target_and_the_time_out():
    m = _model(paddle_width=4, lanes=ONE_PARKED, ball_speed=4, crossings=2, cross_reward=9, max_episode_steps=50)
    _place(m, 0, -20)
    m.px = 17
    for k in range(17):
        _, r, t, _ = m.process(FORWARD)
        assert (r, t) == (0, False) and m.py == 72 - 4 * k
    assert m.py == 8                                    # not yet: py <= 6
    _, r, t, _ = m.process(FORWARD)
    assert (r, t) == (9, False) and (m.px, m.py, m.count) == (40, 76, 1) and m.totals == [1, 0, 0]
    assert _count(m.frame, AM.WHITE) == 4
    for k in range(18):
        _, r, t, _ = m.process(FORWARD)
    assert (r, t) == (9, True) and m.success and m.totals == [2, 0, 1] and "end_target" in m.events
    # a hit and a crossing cannot fall in one tick: py <= 6 covers rows <= 9, the top lane starts at row 12
    assert max(range(7)) + CM.WALKER_H - 1 < 12
    m = _model(paddle_width=4, lanes=ONE_PARKED, crossings=0, max_episode_steps=3)
    assert [m.process(NOOP)[2] for _ in range(3)] == [False, False, True] and not m.success and "end_timeout" in m.events
    # the target AT the limit is the target
    m = _model(paddle_width=4, lanes=ONE_PARKED, ball_speed=4, crossings=1, max_episode_steps=18)
    _place(m, 0, -20)
    out = [m.process(FORWARD) for _ in range(18)]
    assert out[-1][2] and m.success and "end_target" in m.events


def test_steps_past_each_kind_of_terminal():
    m = _model(paddle_width=4, lanes=ONE_PARKED, ball_speed=4, crossings=1, action_repeat=4, max_episode_steps=100)
    _place(m, 0, -20)
    for _ in range(4):
        assert not m.process(FORWARD)[2]
    assert m.process(FORWARD)[2] and m.ticks == 2 and "cut_short" in m.events and m.totals == [1, 0, 1]
    # past the target: one tick a step, the count runs on, the target is counted once
    for k in range(18):
        _, r, t, _ = m.process(FORWARD)
        assert t and m.ticks == 1
    assert m.count == 2 and m.totals == [2, 0, 1] and m.success
    m = _model(paddle_width=4, lanes=ONE_PARKED, crossings=5, max_episode_steps=2, action_repeat=4)
    m.process(NOOP)
    assert m.process(NOOP)[2] and not m.success
    assert m.process(FORWARD)[2] and m.ticks == 4 and m.ep_steps == 3 and not m.success     # past the limit: whole steps


# ---- frames -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(paddle_width=4), dict(lanes=ONE_PARKED, car_length=4),
                                dict(paddle_width=24, lanes=[(4, 4, 1, 1)] * 8, car_length=16)])
def test_reset_frame_pixel_counts(kw):
    m = _model(seed=11, g=3, **kw)
    f = m.frame
    assert f.shape == (84, 84, 3) and f.dtype == np.uint8
    assert (_count(f, AM.WHITE), _count(f, AM.BORDER), _count(f, AM.PADDLE)) == (0, 816, 4 * m.c.paddle_width)
    drawn = 0
    for l, (cars, _, _, _) in enumerate(m.c.lanes):
        cols = [x for x in m.car_columns(l) if 2 <= x <= 81]
        assert len(m.car_columns(l)) == cars * m.c.car_length
        assert _count(f[12 + 8 * l:16 + 8 * l], AM.ROW_COLOURS[1 + l % 5]) == 4 * len(cols)
        assert AM.ROW_COLOURS[1 + l % 5] != AM.PADDLE
        drawn += 4 * len(cols)
    assert int((f != 0).any(2).sum()) == 816 + 4 * m.c.paddle_width + drawn
    assert not f[16:20, 2:82].any() and not f[6:12, 2:82].any()


def test_draw_order():
    m = _model(paddle_width=4, lanes=[(1, 0, 1, 1)] * 8, car_length=16)
    for l in range(8):
        _place(m, l, 36)
    m.px, m.py, m.count = 40, 66, 25                     # rows 66..69 over lane 7's rows 68..71
    f = m.render()
    assert (f[66:70, 40:44] == AM.PADDLE).all()          # the walker in front of the car
    assert (f[68:72, 36:40] == AM.ROW_COLOURS[1 + 7 % 5]).all() and (f[70:72, 40:44] == AM.ROW_COLOURS[3]).all()
    assert _count(f[2:4], AM.WHITE) == 4 * 19 and (f[2, 80] == AM.BORDER).all()           # 19 blocks, on the border
    m.py = 3
    assert (m.render()[3:7, 40:44] == AM.PADDLE).all()   # in front of the border and of nothing else


def test_pixel_change_of_one_lane_move_and_of_one_walker_move():
    m = _model(paddle_width=4, lanes=[(1, 4, 1, 1)], car_length=8, ball_speed=4)
    _place(m, 0, 20)
    m.frame = m.render()
    _, _, _, pc = m.process(NOOP)                        # the car moves from 20..27 to 24..31: 4 columns leave, 4 enter
    colour = sum(AM.ROW_COLOURS[1])
    assert pc.shape == (20, 20) and abs(pc.sum() - 2 * 4 * 4 * colour / float(AM.PC_DENOM)) < 1e-6
    assert not pc[4:].any()
    m = _model(paddle_width=4, lanes=ONE_PARKED, ball_speed=4)
    _, _, _, pc = m.process(FORWARD)                     # the walker leaves rows 76..79 for 72..75
    assert abs(pc.sum() - 2 * 4 * 4 * sum(AM.PADDLE) / float(AM.PC_DENOM)) < 1e-6 and not pc[:16].any()


def test_an_agent_step_at_action_repeat_4_is_four_model_ticks_with_the_rewards_summed():
    kw = dict(CM.SHORT_SETTING)
    one, four = CM.HostCrossing(_conf(**kw), 3, 5), CM.HostCrossing(_conf(**dict(kw, action_repeat=4)), 3, 5)
    rs = np.random.RandomState(4)
    n_cut = 0
    for step in range(200):
        a = int(rs.randint(0, 4))
        _, r4, t4, _ = four.process(a)
        total = 0
        for k in range(four.ticks):
            _, r, t, _ = one.process(a)
            total += r
        assert four.ticks == 4 or one.ended()
        n_cut += four.ticks < 4
        assert total == r4 and (one.record() == four.record()).all()
        assert (four.frame == one.frame).all()
        if t4:
            assert four.ended() or four.ep_steps >= 150
            one.reset(); four.reset()
            one.ep_steps = four.ep_steps = 0
    assert n_cut > 0


def test_host_batch_shard_is_the_same_actors_as_the_whole_batch():
    """host_batch(conf, B, actor_base=B) against models B .. 2B-1 of host_batch(conf, 2B): the same actions for 60 steps, a
    reset after every terminal; rewards, terminals, pixel change, records and frames.  (tests/test_distributed_cpu.py makes this
    comparison for the model modules it lists; this one is not on its list, so it is made here.)"""
    conf = _conf(**dict(CM.SHORT_SETTING, action_repeat=4, max_episode_steps=20))
    B, seed = 4, 0xA3C
    whole, shard = CM.host_batch(conf, 2 * B, seed), CM.host_batch(conf, B, seed, actor_base=B)
    rs = np.random.RandomState(1)
    ends = 0
    for step in range(60):
        acts = rs.randint(0, 4, B)
        for a, m, n in zip(acts, whole[B:], shard):
            (_, r0, t0, pc0), (_, r1, t1, pc1) = m.process(a), n.process(a)
            assert (r0, t0) == (r1, t1) and (pc0 == pc1).all() and (m.record() == n.record()).all() and (m.frame == n.frame).all()
            if t0:
                ends += 1
                m.reset(); n.reset()
    assert ends > 0 and [m.g for m in shard] == [4, 5, 6, 7]
    assert any((a.record() != b.record()).any() for a, b in zip(whole[:B], shard))       # (the draws are the actors' own)


# ---- the traces --------------------------------------------------------------------------------------------------------------
def test_the_traces_hold_the_events_the_gpu_tests_rely_on():
    random = set().union(*[CM.run_trace(k)["events"] for k in range(4)])
    assert CM.TRACE_EVENTS <= random, CM.TRACE_EVENTS - random
    short = CM.run_trace(1)
    assert CM.SHORT_EVENTS <= short["events"]                                 # random play reaches all of it
    assert {-1.0, 0.0, 5.0} <= set(short["reward"].reshape(-1).tolist())
    assert (short["records"][-1, :, 10] > 0).any() and (short["records"][-1, :, 11] > 0).sum() > 100
    assert (short["records"][-1, :, 12] > 0).sum() > 20
    assert CM.REPEAT_EVENTS <= CM.run_trace(4)["events"]
    assert CM.SCRIPTED_EVENTS <= CM.run_trace(5)["events"], CM.SCRIPTED_EVENTS - CM.run_trace(5)["events"]
    runner = CM.run_trace(6)
    assert CM.RUNNER_EVENTS <= runner["events"] and runner["records"][:, :, 3].max() == 20
    widest = CM.trace_config(3)
    assert widest.paddle_width == 24 and widest.car_length == 16 and len(widest.lanes) == 8 and len(CM.trace_config(2).lanes) == 1
    for k in range(CM.N_TRACES):
        tr = CM.run_trace(k)
        assert tr["records"].shape[2] == 16 and not tr["records"][:, :, 7:10].any() and not tr["records"][:, :, 13:].any()
        assert (tr["records"][:, :, 5:7] & ~0x7F7F7F7F == 0).all() and (tr["records"][:, :, 4] < 12).all()
