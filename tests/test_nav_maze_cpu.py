"""First-person navigation mazes (register_maze_config with apples, rewards, goal_respawn, action_set): configuration
checks, the block's words, Environment.get_action_size and known answers of the host model in tests/nav_maze_model.py
(no GPU)."""
import numpy as np
import pytest

try:
    import fp_maze_model as FP
    import maze_model as MM
    import nav_maze_model as NM
except ImportError:            # imported as tests.<module>
    from tests import fp_maze_model as FP
    from tests import maze_model as MM
    from tests import nav_maze_model as NM

OPEN7 = ["-------",
         "-------",
         "-------",
         "---S---",
         "-------",
         "-------",
         "------G"]
# apples at (4, 3) and (3, 1); the goal at (6, 6), the start at (3, 3)
APPLE7 = ["-------",
          "---A---",
          "-------",
          "---SA--",
          "-------",
          "-------",
          "------G"]
# a corridor row y = 3 between walls: x = 1..5 free, the rest walls
CORRIDOR = ["+++++++",
            "+++++++",
            "+++++++",
            "+S-A-G+",
            "+++++++",
            "+++++++",
            "+++++++"]


def _cfg(layouts, **kw):
    from unreal_amd.environment.maze_environment import MazeConfig
    return MazeConfig(layouts, **kw)


def _fp(layouts, **kw):
    return _cfg(layouts, view="first_person", **kw)


@pytest.mark.parametrize("kw", [dict(goal_reward=2), dict(apple_reward=0), dict(hit_reward=0), dict(goal_respawn=True,
                                max_episode_steps=9), dict(action_set="lab")])
def test_navigation_options_with_the_top_down_view_raise(kw):
    with pytest.raises(ValueError):
        _cfg([OPEN7], **kw)
    with pytest.raises(ValueError):
        _cfg([OPEN7], view="top_down", **kw)
    _fp([OPEN7], **kw)                       # the same options in first person are fine


def test_apples_in_a_top_down_layout_raise():
    with pytest.raises(ValueError):
        _cfg([APPLE7])
    assert _fp([APPLE7]).nav


def test_more_than_64_apples_raise():
    lay = "S" + "A" * 65 + "-" * (144 - 67) + "G"
    with pytest.raises(ValueError):
        _fp([lay])
    ok = "S" + "A" * 64 + "-" * (144 - 66) + "G"
    assert len(_fp([ok]).apples[0]) == 64


@pytest.mark.parametrize("name", ["goal_reward", "apple_reward", "hit_reward"])
@pytest.mark.parametrize("value", [101, -101, 1.5, 2.0, True, False, "1", None])
def test_bad_rewards_raise(name, value):
    with pytest.raises(ValueError):
        _fp([OPEN7], **{name: value})


@pytest.mark.parametrize("name", ["goal_reward", "apple_reward", "hit_reward"])
@pytest.mark.parametrize("value", [100, -100, 0, np.int32(7)])
def test_rewards_in_range_are_taken(name, value):
    c = _fp([OPEN7], **{name: value})
    assert getattr(c, name) == int(value) and c.nav


def test_goal_respawn_needs_a_step_limit_and_a_drawn_start_with_a_drawn_goal():
    with pytest.raises(ValueError):
        _fp([OPEN7], goal_respawn=True)
    with pytest.raises(ValueError):
        _fp([OPEN7], goal_respawn=True, max_episode_steps=10, random_goal=True)
    _fp([OPEN7], goal_respawn=True, max_episode_steps=10, random_goal=True, random_start=True)


@pytest.mark.parametrize("action_set", ["Lab", "strafe", "", None, 6])
def test_unknown_action_set_raises(action_set):
    with pytest.raises(ValueError):
        _fp([OPEN7], action_set=action_set)


def test_register_maze_config_takes_the_navigation_options():
    from unreal_amd.environment.environment import Environment
    Environment.register_maze_config("nav_cpu_register", [APPLE7], view="first_person", goal_reward=10, apple_reward=1,
                                     hit_reward=0, goal_respawn=True, max_episode_steps=50, action_set="lab")
    try:
        c = Environment.MAZE_CONFIG["nav_cpu_register"]
        assert (c.goal_reward, c.apple_reward, c.hit_reward, c.goal_respawn, c.action_set) == (10, 1, 0, True, "lab")
        assert c.nav and c.action_size == 6 and c.reward_bound == 10
    finally:
        Environment.MAZE_CONFIG.pop("nav_cpu_register", None)
    with pytest.raises(ValueError):
        Environment.register_maze_config("nav_cpu_bad", [APPLE7], view="first_person", goal_reward=1000)
    assert "nav_cpu_bad" not in Environment.MAZE_CONFIG


def test_configs_without_navigation_options_build_todays_block():
    """Explicit defaults change nothing: no NAV flag, no extension, the same words."""
    rs = np.random.RandomState(5)
    lays = [MM.random_layout(12, rs) for _ in range(3)]
    for view in ("top_down", "first_person"):
        kw = dict(view=view, random_start=True, random_goal=True, show_goal=True, max_episode_steps=9)
        base = _cfg(lays, **kw)
        same = _cfg(lays, goal_reward=1, apple_reward=1, hit_reward=-1, goal_respawn=False, action_set="turn", **kw)
        assert not base.nav and not same.nav and base.action_size == 4 and base.reward_bound == 1
        np.testing.assert_array_equal(same.block(77), base.block(77))
        assert len(base.block(77)) == 8 + 3 * (18 + 144) and base.block(77)[2] == 7


def test_block_words_of_a_navigation_config():
    lays = [APPLE7, OPEN7, CORRIDOR]
    c = _fp(lays, random_start=True, random_goal=True, max_episode_steps=40, goal_reward=10, apple_reward=2,
            hit_reward=-3, goal_respawn=True, action_set="lab", start_heading=1)
    plain = _fp(lays, random_start=True, random_goal=True, max_episode_steps=40, start_heading=1)
    blk, pb = c.block(0xABCDEF), plain.block(0xABCDEF)
    rec = 18 + 49
    n = 8 + 3 * rec
    assert blk[2] == pb[2] == 1 | 2 | 8            # the apples alone make `plain` a navigation block
    today = _fp([[r.replace("A", "-") for r in l] for l in lays], random_start=True, random_goal=True, max_episode_steps=40,
                start_heading=1).block(0xABCDEF)
    assert len(today) == n and today[2] == 1 | 2
    np.testing.assert_array_equal(np.delete(blk[:n], 2), np.delete(today, 2))   # the layout records are today's
    np.testing.assert_array_equal(pb[:n], blk[:n])
    assert list(pb[n:n + 8]) == [1, 1, -1, 0, 0, 0, 0, 0]
    ext = blk[n:]
    assert len(ext) == 8 + 3 * 65
    assert list(ext[:8]) == [10, 2, -3, 1 | 2, 0, 0, 0, 0]
    assert list(ext[8:8 + 3]) == [2, 1 * 7 + 3, 3 * 7 + 4] and not ext[11:8 + 65].any()
    assert ext[8 + 65] == 0 and not ext[8 + 66:8 + 130].any()
    assert list(ext[8 + 130:8 + 132]) == [1, 3 * 7 + 3] and not ext[8 + 132:].any()
    # the apple cells are free cells (BFS, start / goal draws)
    assert 3 * 7 + 4 in c.free[0] and 3 * 7 + 3 in c.free[2]
    # only apples: a navigation block with today's rewards and the turn set
    only = _fp([APPLE7]).block(0)
    assert only[2] & 8 and list(only[8 + rec:8 + rec + 4]) == [1, 1, -1, 0]


def test_get_action_size_of_navigation_and_other_configs():
    """6 for a registered config with action_set='lab', without reading or writing the class cache; every other case as
    before, the first-query-wins cache included."""
    from unreal_amd.environment.environment import Environment
    saved = Environment.action_size
    Environment.register_maze_config("nav_cpu_lab", [APPLE7], view="first_person", action_set="lab")
    Environment.register_maze_config("nav_cpu_turn", [APPLE7], view="first_person", goal_reward=5)
    Environment.register_gym_config("nav_cpu_gym", 9)
    try:
        Environment.action_size = -1
        assert Environment.get_action_size("maze", "nav_cpu_lab") == 6
        assert Environment.action_size == -1                          # not written
        assert Environment.get_action_size("maze", "nav_cpu_turn") == 4
        assert Environment.action_size == 4                           # the reference's cache
        assert Environment.get_action_size("maze", "nav_cpu_lab") == 6    # not read
        assert Environment.get_action_size("lab", "x") == 4           # first query wins, as before
        assert Environment.get_action_size("maze", "unregistered") == 4
        Environment.action_size = 17
        assert Environment.get_action_size("maze", "nav_cpu_lab") == 6
        assert Environment.get_action_size("maze", "nav_cpu_turn") == 17
        assert Environment.get_action_size("lab", "nav_cpu_lab") == 17      # another env type: the name is not a maze
        for env_type, name, want in (("lab", "x", 6), ("indoor", "x", 3), ("gym", "nav_cpu_gym", 9),
                                     ("maze", "", 4)):
            Environment.action_size = -1
            assert Environment.get_action_size(env_type, name) == want
            assert Environment.action_size == want
    finally:
        Environment.action_size = saved
        for n in ("nav_cpu_lab", "nav_cpu_turn"):
            Environment.MAZE_CONFIG.pop(n, None)
        Environment.GYM_CONFIG.pop("nav_cpu_gym", None)


# ---- host model known answers -----------------------------------------------------------------------------------------
def _actor(layout, h=0, **kw):
    kw.setdefault("start_heading", h)
    c = _fp([layout], **kw)
    return c, NM.HostNavMaze(c, 0, 1, seed=0)


@pytest.mark.parametrize("h", range(4))
def test_each_strafe_and_look_of_the_lab_set(h):
    """From (3, 3) of an open maze: look left / right turn in place; strafe left / right move by -r / +r; forward / back
    by +d / -d; none of them is rewarded."""
    c, m = _actor(OPEN7, h, action_set="lab")
    d, r = NM.DIRS[h], NM.DIRS[(h + 1) % 4]
    want = {0: (3, 3, (h + 3) % 4), 1: (3, 3, (h + 1) % 4), 2: (3 - r[0], 3 - r[1], h), 3: (3 + r[0], 3 + r[1], h),
            4: (3 + d[0], 3 + d[1], h), 5: (3 - d[0], 3 - d[1], h)}
    for a, (x, y, hh) in want.items():
        m.reset()
        _, rew, term, _ = m.process(a)
        assert (m.x, m.y, m.h, rew, term) == (x, y, hh, 0, False), a


def test_turn_set_keeps_todays_moves():
    c, m = _actor(OPEN7, 1, goal_reward=3)
    for a, want in ((0, (3, 3, 0)), (1, (3, 3, 2)), (2, (3, 4, 1)), (3, (3, 2, 1))):
        m.reset()
        m.process(a)
        assert (m.x, m.y, m.h) == want, a
    m.reset()
    _, r, _, _ = m.process(4)                 # not an action of the turn set: nothing happens
    assert (m.x, m.y, m.h, r) == (3, 3, 1, 0)


def test_a_hit_during_a_strafe():
    """In the corridor facing +x, strafing either way runs into a wall: the agent stays, reward hit_reward."""
    c, m = _actor(CORRIDOR, 0, action_set="lab", hit_reward=-7)
    for a in (2, 3):
        _, r, t, _ = m.process(a)
        assert (m.x, m.y, r, t) == (1, 3, -7, False)
    _, r, _, _ = m.process(5)                 # back: into the wall at (0, 3)
    assert (m.x, m.y, r) == (1, 3, -7)


def test_an_apple_is_collected_once_and_restored_at_reset():
    c, m = _actor(CORRIDOR, 0, apple_reward=4, goal_reward=10)
    _, r, _, _ = m.process(2)                 # (2, 3)
    assert r == 0
    _, r, _, _ = m.process(2)                 # (3, 3): the apple
    assert r == 4 and m.collected == 1 and m.apples_total == 1 and m.record()[1:5] == [1, 0, 0, 1]
    m.process(3)                              # back to (2, 3)
    _, r, _, _ = m.process(2)                 # into (3, 3) again: collected already
    assert r == 0 and m.apples_total == 1
    m.reset()
    assert m.collected == 0 and m.apples_total == 1
    m.process(2)
    _, r, _, _ = m.process(2)
    assert r == 4 and m.apples_total == 2


def test_an_apple_is_drawn_until_collected():
    """Looking down the corridor the apple's floor is APPLE_FLOOR; once collected (and the agent stepped off) it is gone."""
    c, m = _actor(CORRIDOR, 0, apple_reward=1)
    green = lambda f: int((f == NM.APPLE_FLOOR).all(2).sum())
    assert green(m.frame) > 0
    m.process(2); m.process(2); m.process(3)
    assert m.collected == 1 and green(m.frame) == 0
    plain = FP.render(c, 0, m.x, m.y, m.h, m.gx, m.gy)
    np.testing.assert_array_equal(m.frame, plain)


def test_an_apple_under_a_start_is_not_collected():
    """A reset onto an apple cell collects nothing; stepping off and back onto it does."""
    lay = ["-------", "-------", "-------", "---A---", "-------", "-------", "------G"]
    c = _fp([lay], random_start=True, start_heading=0, apple_reward=5)
    apple = 3 * 7 + 3
    for g in range(200):
        m = NM.HostNavMaze(c, g, 200, seed=1)
        if (m.y * 7 + m.x) == apple:
            break
    else:
        raise AssertionError("no start on the apple")
    assert m.collected == 0 and m.apples_total == 0
    _, r, _, _ = m.process(2)
    assert r == 0
    _, r, _, _ = m.process(3)
    assert r == 5 and m.collected == 1


def test_an_apple_under_a_drawn_goal_is_inactive():
    """With random_goal, an episode whose goal is drawn on the apple cell neither draws nor counts that apple."""
    lay = ["S------", "-------", "-------", "---A---", "-------", "-------", "-------"]
    c = _fp([lay], random_goal=True, random_start=True, start_heading=0, show_goal=True)
    apple = 3 * 7 + 3
    for g in range(400):
        m = NM.HostNavMaze(c, g, 400, seed=2)
        if m.goal_cell == apple:
            break
    else:
        raise AssertionError("no goal on the apple")
    assert m.active_apples() == frozenset()
    np.testing.assert_array_equal(m.frame, FP.render(c, 0, m.x, m.y, m.h, m.gx, m.gy))
    other = next(NM.HostNavMaze(c, g, 400, seed=2) for g in range(400)
                 if NM.HostNavMaze(c, g, 400, seed=2).goal_cell != apple)
    assert other.active_apples() == frozenset([apple])


def test_philox_known_answer_and_the_respawn_draw():
    """Philox4x32-10 at counter = key = 0 is Random123's known answer; a respawn draws word 1 over the free cells other
    than the goal and word 2 mod 4 for the heading, at counter (g, episode, RESPAWN_STREAM, goals_total)."""
    u = MM.philox4x32_10((0, 0, 0, 0), (0, 0))
    assert [int(w) for w in u] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert NM.RESPAWN_STREAM == 0x4D415A52 and NM.RESPAWN_STREAM != MM.MAZE_STREAM
    c = _fp([OPEN7], random_start=True, random_goal=True, goal_respawn=True, max_episode_steps=9)
    seed = 0x1234_5678_9ABC
    w = MM.philox4x32_10((5, 3, NM.RESPAWN_STREAM, 2), (seed & 0xFFFFFFFF, seed >> 32))
    others = [int(x) for x in c.free[0] if x != 17]
    assert NM.respawn_cell(c, 0, 5, 3, 2, 17, seed) == (others[int(w[1]) % 48], int(w[2]) % 4)
    fixed = _fp([OPEN7], goal_respawn=True, max_episode_steps=9, start_heading=2)
    assert NM.respawn_cell(fixed, 0, 5, 3, 2, 48, seed) == (3 * 7 + 3, 2)
    draws = set(NM.respawn_cell(c, 0, 5, 3, k, 17, seed) for k in range(1, 200))
    assert len(draws) > 100 and all(s != 17 for s, _ in draws)


def test_a_respawn_at_the_goal_and_a_goal_on_the_time_out_step():
    """goal_respawn: the goal gives goal_reward and moves the agent to the respawn draw, the episode running on; the goal
    on the time-out step is terminal with the goal reward."""
    lay = ["-------", "-------", "-------", "---SG--", "-------", "-------", "-------"]
    c = _fp([lay], goal_respawn=True, max_episode_steps=3, start_heading=0, goal_reward=10, apple_reward=1, hit_reward=0)
    m = NM.HostNavMaze(c, 0, 1, seed=0)
    _, r, t, pc = m.process(2)
    assert (r, t, m.respawned, m.goals_total, (m.x, m.y), m.h) == (10, False, True, 1, (3, 3), 0)
    assert pc.sum() == 0                      # the same view as before the step
    m.process(0)                              # step 2: look left
    m.process(1)
    assert m.ep_steps == 3 and m.timed_out
    m.reset()
    m.process(0); m.process(1)
    _, r, t, _ = m.process(2)                 # the goal on the time-out step
    assert (r, t, m.at_goal, m.respawned, m.goals_total) == (10, True, True, False, 2)
    # without goal_respawn the goal ends the episode, as today
    c2 = _fp([lay], max_episode_steps=3, start_heading=0, goal_reward=10)
    m2 = NM.HostNavMaze(c2, 0, 1, seed=0)
    _, r, t, _ = m2.process(2)
    assert (r, t, m2.timed_out, m2.respawned) == (10, True, False, False)


def test_default_rewards_match_the_first_person_model():
    """A navigation config with today's rewards and no apples or respawn steps like fp_maze_model (frames included)."""
    rs = np.random.RandomState(8)
    lays = [MM.random_layout(12, rs) for _ in range(2)]
    kw = dict(random_start=True, random_goal=True, show_goal=True, max_episode_steps=15)
    nav, plain = _fp(lays, action_set="turn", goal_reward=1, **kw), _fp(lays, **kw)
    for g in range(6):
        a, b = NM.HostNavMaze(nav, g, 6, seed=3), FP.HostFirstPersonMaze(plain, g, 6, seed=3)
        for k in range(60):
            act = rs.randint(0, 4)
            ra, rb = a.process(act), b.process(act)
            assert ra[1:3] == rb[1:3]
            np.testing.assert_array_equal(a.frame, b.frame)
            if ra[2]:
                a.reset(); b.reset()


def test_draws_do_not_depend_on_views_groups_or_ranks():
    """The reset and respawn draws are functions of (seed, global actor, episode, goals_total): a batch cut into
    ranks or groups yields the same models as one batch."""
    c = _fp([APPLE7, OPEN7], random_start=True, random_goal=True, goal_respawn=True, max_episode_steps=30,
            action_set="lab", goal_reward=10)
    whole = NM.host_batch(c, 16, seed=9)
    parts = NM.host_batch(c, 8, 0, 16, seed=9) + NM.host_batch(c, 8, 8, 16, seed=9)
    rs = np.random.RandomState(0)
    for k in range(200):
        acts = rs.randint(0, 6, 16)
        for m1, m2, a in zip(whole, parts, acts):
            r1, r2 = m1.process(a), m2.process(a)
            assert r1[1:3] == r2[1:3]
            assert (m1.x, m1.y, m1.h, m1.layout) == (m2.x, m2.y, m2.h, m2.layout)
            if r1[2]:
                m1.reset(); m2.reset()
    assert sum(m.goals_total for m in whole) > 0
