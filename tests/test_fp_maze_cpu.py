"""First-person maze views (register_maze_config(..., view="first_person")): configuration checks and known answers of the
host model in tests/fp_maze_model.py (no GPU)."""
import numpy as np
import pytest

try:
    import fp_maze_model as FP
    import maze_model as MM
except ImportError:            # imported as tests.<module>
    from tests import fp_maze_model as FP
    from tests import maze_model as MM

OPEN7 = ["-------",
         "-------",
         "-------",
         "---S---",
         "-------",
         "-------",
         "------G"]


def _cfg(layouts, **kw):
    from unreal_amd.environment.maze_environment import MazeConfig
    return MazeConfig(layouts, **kw)


@pytest.mark.parametrize("kw", [dict(view="side"), dict(view=None), dict(view="first_person", start_heading=4),
                                dict(view="first_person", start_heading=-1), dict(view="first_person", start_heading=1.5),
                                dict(view="first_person", start_heading=True), dict(start_heading=0)])
def test_bad_view_and_start_heading_raise(kw):
    with pytest.raises(ValueError):
        _cfg([OPEN7], **kw)


def test_register_maze_config_takes_view_and_start_heading():
    from unreal_amd.environment.environment import Environment
    Environment.register_maze_config("fp_cpu_register", [OPEN7], view="first_person", start_heading=3)
    try:
        c = Environment.MAZE_CONFIG["fp_cpu_register"]
        assert (c.view, c.start_heading) == ("first_person", 3)
    finally:
        Environment.MAZE_CONFIG.pop("fp_cpu_register", None)
    with pytest.raises(ValueError):
        Environment.register_maze_config("fp_cpu_bad", [OPEN7], view="isometric")
    assert "fp_cpu_bad" not in Environment.MAZE_CONFIG


def test_default_block_words_are_unchanged():
    """The defaults are the top-down config: header word 7 stays 0, and a first-person config with a drawn heading has the
    same block; a fixed heading only sets word 7 to heading + 1."""
    rs = np.random.RandomState(3)
    lays = [MM.random_layout(12, rs) for _ in range(3)]
    kw = dict(random_start=True, random_goal=True, show_goal=True, max_episode_steps=9)
    base = _cfg(lays, **kw)
    assert (base.view, base.start_heading) == ("top_down", None)
    blk = base.block(0x1234_5678_9ABC)
    assert blk[7] == 0 and list(blk[:7]) == [12, 3, 7, 9, 0x5678_9ABC, 0x1234, 18 + 144]
    np.testing.assert_array_equal(_cfg(lays, view="top_down", **kw).block(0x1234_5678_9ABC), blk)
    np.testing.assert_array_equal(_cfg(lays, view="first_person", **kw).block(0x1234_5678_9ABC), blk)
    fixed = _cfg(lays, view="first_person", start_heading=2, **kw).block(0x1234_5678_9ABC)
    assert fixed[7] == 3
    np.testing.assert_array_equal(np.delete(fixed, 7), np.delete(blk, 7))


def test_wall_at_one_and_a_half_cells_fills_rows_14_to_69():
    """The eye at (1, 3) looks along +x; (2, 3) is free and (3, 3) a wall: its x-face lies at t = 3/2.  Columns whose ray
    stays in row 3 up to t = 3/2 (|q| < 28) show it on rows 14..69 exactly, in the interior-wall x-face colour."""
    lay = ["-------", "-------", "-------", "-S-+---", "-------", "-------", "------G"]
    cfg = _cfg([lay], view="first_person", start_heading=0)
    img = FP.render(cfg, 0, 1, 3, 0, 6, 6)
    cols = [i for i in range(84) if abs(2 * i + 1 - 84) < 28]
    assert cols == list(range(28, 56))
    for i in cols:
        tn, td, border, xface, _ = FP.cast(cfg.walls[0], 7, 1, 3, 0, i)
        assert (tn, td, border, xface) == (3, 2, False, True)
        wall = (img[:, i] == (255, 0, 0)).all(1)
        assert list(np.flatnonzero(wall)) == list(range(14, 70)), i
    assert (img[:14, 40] == 0).all() and (img[70:, 40] == FP.FLOOR).all()


def test_symmetric_corridor_gives_a_mirrored_view():
    """An open map seen from its middle row along +x, the goal on the view axis: every column mirrors its partner."""
    cfg = _cfg([OPEN7], view="first_person", start_heading=0, show_goal=True)
    img = FP.render(cfg, 0, 0, 3, 0, 5, 3)
    np.testing.assert_array_equal(img, img[:, ::-1])
    assert (img == FP.GOAL_FLOOR).all(2).any()
    assert (img[:, :, 1] > 0).any() and not (img[:, :, 0] == 255).all(axis=None)     # the border (channel 1) is seen


def test_four_right_turns_return_the_first_frame():
    rs = np.random.RandomState(5)
    cfg = _cfg([MM.random_layout(14, rs) for _ in range(2)], view="first_person", random_start=True,
               random_goal=True, show_goal=True)
    for g in range(6):
        m = FP.HostFirstPersonMaze(cfg, g, 6, seed=11)
        first = m.frame.copy()
        frames = []
        for _ in range(4):
            _, r, t, pc = m.process(1)
            assert (r, t) == (0, False)
            frames.append(m.frame)
        np.testing.assert_array_equal(frames[-1], first)
        assert len({f.tobytes() for f in frames}) == 4        # the four headings look different
        assert pc.shape == (20, 20) and pc.dtype == np.float32 and pc.max() > 0


@pytest.mark.parametrize("N", [7, 12, 14, 21])
def test_the_camera_has_no_ties(N):
    """No column of any heading meets a forward and a side boundary at the same t (odd vs even), from any cell of an
    open map (its rays cross the most boundaries)."""
    walls = np.zeros(N * N, dtype=bool)
    for ex, ey in ((0, 0), (N // 2, N // 2), (N - 1, 1)):
        for h in range(4):
            for i in range(84):
                assert FP.cast(walls, N, ex, ey, h, i)[4] == 0


def test_goal_tile_follows_show_goal():
    """The goal two cells ahead: drawn in (40, 40, 255) on the floor with show_goal, plain floor without."""
    for show in (True, False):
        cfg = _cfg([OPEN7], view="first_person", start_heading=0, show_goal=show)
        img = FP.render(cfg, 0, 1, 3, 0, 3, 3)
        goal = (img == FP.GOAL_FLOOR).all(2)
        assert goal.any() == show
        if show:
            rows, cols = np.nonzero(goal)
            assert rows.min() > 42 and set(cols) == set(83 - cols)
            # two cells ahead: floor((2H + p) / 2p) == 2, i.e. 3p <= 168 < 5p (p = 2y + 1 - 84): rows 59..69
            assert sorted(set(rows)) == list(range(59, 70))


def test_heading_draw_known_answers():
    """With start_heading None the heading is Philox word 2 of the reset draw, mod 4 (key = seed, counter = (global actor,
    episode, 0x4D415A45, 0)); a fixed heading is used as given."""
    cfg = _cfg([OPEN7], view="first_person")
    got = [FP.reset_heading(cfg, g, ep, 0xBEEF) for g in range(4) for ep in range(3)]
    want = [int(MM.philox4x32_10((g, ep, 0x4D415A45, 0), (0xBEEF, 0))[2]) % 4 for g in range(4) for ep in range(3)]
    assert got == want
    assert got == KNOWN_HEADINGS
    fixed = _cfg([OPEN7], view="first_person", start_heading=2)
    assert {FP.reset_heading(fixed, g, ep, 0xBEEF) for g in range(4) for ep in range(3)} == {2}


KNOWN_HEADINGS = [1, 1, 1, 0, 2, 2, 1, 0, 1, 0, 1, 0]          # actors 0..3, episodes 0..2, seed 0xBEEF


def test_pixel_change_is_the_reference_formula():
    """The host model's exact pixel change equals oracle.maze.calc_pixel_change on bytes / 255 to float rounding."""
    from oracle.maze import calc_pixel_change
    rs = np.random.RandomState(7)
    cfg = _cfg([MM.random_layout(21, rs)], view="first_person", random_start=True, random_goal=True, show_goal=True)
    m = FP.HostFirstPersonMaze(cfg, 0, 1, seed=3)
    n_moved = 0
    for a in rs.randint(0, 4, 60):
        old = m.frame
        _, _, t, pc = m.process(a)
        ref = calc_pixel_change(m.frame / 255.0, old / 255.0)
        assert np.abs(pc - ref).max() <= 1e-7
        n_moved += pc.max() > 0
        if t:
            m.reset()
    assert n_moved > 10
