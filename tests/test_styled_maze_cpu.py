"""Styled first-person walls and landmarks without a GPU: MazeConfig's validation and block words, the texel
formula against exact rational arithmetic, one known frame, and generated landmarks against tests/styled_maze_model.py."""
from fractions import Fraction

import numpy as np
import pytest

try:
    import fp_maze_model as FP
    import gen_maze_model as GM
    import maze_model as MM
    import styled_maze_model as SM
except ImportError:            # imported as tests.<module>
    from tests import fp_maze_model as FP
    from tests import gen_maze_model as GM
    from tests import maze_model as MM
    from tests import styled_maze_model as SM

from unreal_amd.environment.maze_environment import MazeConfig

SIZES = (7, 12, 14, 21)
STYLES = [(200, 100, 50, 0xAA), (0, 255, 0, 0x00), (255, 255, 255, 0xFF), (10, 20, 250, 0x0F), (90, 90, 90, 0x81),
          (255, 0, 255, 0x3C), (1, 2, 3, 0x55)]
W = H = 84


def styled_layout(N, rs, n_styles, marks=""):
    """A random layout whose wall cells carry random digits 0..n_styles ('+' for 0)."""
    cells = list(MM.random_layout(N, rs, marks=marks))
    for c, ch in enumerate(cells):
        k = rs.randint(0, n_styles + 1)
        if ch == "+" and k:
            cells[c] = str(k)
    return "".join(cells)


def plain(layout):
    return "".join("+" if ch.isdigit() else ch for ch in layout)


def gen_config(N, **kw):
    return MazeConfig(None, random_start=True, random_goal=True, view="first_person", generate=N, **kw)


# ---- validation ------------------------------------------------------------------------------------------------------
def test_validation_errors():
    rs = np.random.RandomState(0)
    lay = MM.random_layout(7, rs)
    fp = dict(random_start=True, random_goal=True, view="first_person")
    ok = MazeConfig([lay], wall_styles=[(1, 2, 3, 4)], **fp)
    assert ok.styled and ok.flags & MazeConfig.STYLED and not MazeConfig([lay], **fp).styled
    bad_styles = [[], [(1, 2, 3, 4)] * 8, [(1, 2, 3)], [(1, 2, 3, 4, 5)], [(1, 2, 3, 256)], [(-1, 2, 3, 4)],
                  [(True, 2, 3, 4)], [(1.0, 2, 3, 4)], [(1, 2, 3, "4")], "1234", [7], 5]
    for ws in bad_styles:
        with pytest.raises(ValueError):
            MazeConfig([lay], wall_styles=ws, **fp)
    with pytest.raises(ValueError):                      # first person only
        MazeConfig([lay], random_start=True, random_goal=True, wall_styles=[(1, 2, 3, 4)])
    wall = lay.index("+")
    digit = lambda d: lay[:wall] + d + lay[wall + 1:]
    with pytest.raises(ValueError):                      # a digit without wall_styles
        MazeConfig([digit("1")], **fp)
    with pytest.raises(ValueError):                      # ... also top-down
        MazeConfig([digit("1")], random_start=True, random_goal=True)
    with pytest.raises(ValueError):                      # a digit beyond the styles
        MazeConfig([digit("3")], wall_styles=STYLES[:2], **fp)
    for d in ("8", "9", "0"):
        with pytest.raises(ValueError):
            MazeConfig([digit(d)], wall_styles=STYLES, **fp)
    MazeConfig([digit("2")], wall_styles=STYLES[:2], **fp)
    for dens in (-1, 257, True, 1.0, "3", None):
        with pytest.raises(ValueError):
            gen_config(7, wall_styles=STYLES, gen_landmark_density=dens)
    with pytest.raises(ValueError):                      # needs wall_styles
        gen_config(7, gen_landmark_density=5)
    with pytest.raises(ValueError):                      # needs generate
        MazeConfig([lay], wall_styles=STYLES, gen_landmark_density=5, **fp)
    assert gen_config(7, wall_styles=STYLES, gen_landmark_density=256).gen_landmark_density == 256
    from unreal_amd.environment.environment import Environment
    try:
        Environment.register_maze_config("styled_reg", [digit("1")], wall_styles=[(9, 8, 7, 6)], **fp)
        assert Environment.MAZE_CONFIG["styled_reg"].wall_styles == [(9, 8, 7, 6)]
        with pytest.raises(ValueError):
            Environment.register_maze_config("styled_reg2", [digit("2")], wall_styles=[(9, 8, 7, 6)], **fp)
    finally:
        Environment.MAZE_CONFIG.pop("styled_reg", None)


def test_digits_are_walls():
    """Digits count as walls for connectivity, the free list, the wall bits and the apples' surroundings."""
    rs = np.random.RandomState(3)
    for N in SIZES:
        lay = styled_layout(N, rs, 7, marks="AA")
        a = MazeConfig([lay], True, True, view="first_person", wall_styles=STYLES)
        b = MazeConfig([plain(lay)], True, True, view="first_person")
        np.testing.assert_array_equal(a.walls[0], b.walls[0])
        np.testing.assert_array_equal(a.free[0], b.free[0])
        np.testing.assert_array_equal(a.apples[0], b.apples[0])
        np.testing.assert_array_equal(a.styles[0], [int(ch) if ch.isdigit() else 0 for ch in lay])
        assert a.styles[0].max() > 0 and (a.styles[0][~a.walls[0]] == 0).all()
    closed = list("-" * 49)
    for c in range(7):
        closed[7 * c + 3] = "1"                          # a styled wall that cuts the map in two
    with pytest.raises(ValueError):
        MazeConfig(["".join(closed)], True, True, view="first_person", wall_styles=STYLES)


# ---- block words -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("nav", [False, True])
def test_static_block_is_the_unstyled_block_plus_the_style_section(N, nav):
    rs = np.random.RandomState(N + nav)
    n_styles = 7 if N != 12 else 3
    lays = [styled_layout(N, rs, n_styles, marks="AAA" if nav else "") for _ in range(3)]
    kw = dict(random_start=True, random_goal=True, show_goal=True, max_episode_steps=9, view="first_person")
    if nav:
        kw.update(goal_reward=10, hit_reward=0, goal_respawn=True, action_set="lab")
    cfg = MazeConfig(lays, wall_styles=STYLES[:n_styles], **kw)
    base = MazeConfig([plain(l) for l in lays], **kw).block(0x1234567890)
    got = cfg.block(0x1234567890)
    want = base.copy()
    want[2] |= 32
    ids = [np.array([int(ch) if ch.isdigit() else 0 for ch in l]) for l in lays]
    want = np.concatenate([want, SM.style_section(STYLES[:n_styles], 0, N, ids)])
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, want)
    off = len(base)                                      # the section's offset: after the records / navigation extension
    assert off == 8 + 3 * (18 + N * N) + (8 + 3 * 65 if nav else 0)
    assert got[off] == n_styles and got[off + 1] == 0 and not got[off + 2:off + 8].any()
    r, g, b, pat = STYLES[0]
    assert got[off + 8] == np.array([r | g << 8 | b << 16 | pat << 24], np.uint32).view(np.int32)[0]
    assert not got[off + 8 + n_styles:off + 16].any()
    sw = (N * N + 7) // 8
    assert len(got) == off + 16 + 3 * sw
    for c in (0, 7, 8, N * N - 1):                       # nibble c & 7 of word c >> 3
        assert (int(got[off + 16 + sw + (c >> 3)]) >> (4 * (c & 7))) & 15 == ids[1][c]


@pytest.mark.parametrize("N", SIZES)
def test_generated_block_is_the_unstyled_block_plus_the_style_section(N):
    kw = dict(gen_loops=2, gen_apples=3, show_goal=True, max_episode_steps=30)
    cfg = gen_config(N, wall_styles=STYLES[:5], gen_landmark_density=64, **kw)
    want = gen_config(N, **kw).block(77).copy()
    assert len(want) == 16
    want[2] |= 32
    want = np.concatenate([want, SM.style_section(STYLES[:5], 64, N, [])])
    np.testing.assert_array_equal(cfg.block(77), want)
    assert len(want) == 32 and want[2] & 16 and want[16] == 5 and want[17] == 64


def test_an_unstyled_config_has_no_flag_and_no_section():
    rs = np.random.RandomState(5)
    lay = MM.random_layout(7, rs)
    blk = MazeConfig([lay], True, True, view="first_person").block(1)
    assert not blk[2] & 32 and len(blk) == 8 + 18 + 49
    assert len(gen_config(7).block(1)) == 16


# ---- texels ---------------------------------------------------------------------------------------------------------
def world_hit(ex, ey, h, i, forward, index):
    """The hit point (x, y) of column i's ray from the centre of cell (ex, ey), in world coordinates (cell (x, y) covers
    [x, x + 1) x [y, y + 1)), exactly."""
    dx, dy = FP.DIRS[h]
    rx, ry = FP.DIRS[(h + 1) % 4]
    q = 2 * i + 1 - W
    t = Fraction(2 * index + 1, 2) if forward else Fraction((2 * index + 1) * W, 2 * abs(q))
    x = Fraction(2 * ex + 1, 2) + t * dx + t * Fraction(q, W) * rx
    y = Fraction(2 * ey + 1, 2) + t * dy + t * Fraction(q, W) * ry
    return x, y


def frac8(c):
    return int((c - (c.numerator // c.denominator)) * 8)


@pytest.mark.parametrize("N", SIZES)
def test_texel_is_the_eighth_of_the_world_coordinate_along_the_face(N):
    """Every heading, column and crossing index a ray can reach in an N x N map (a ray crosses at most N boundaries of
    either kind), from two eye cells: u == floor(8 frac(c)), c the coordinate along the face, in exact fractions."""
    for h in range(4):
        dx, dy = FP.DIRS[h]
        rx, ry = FP.DIRS[(h + 1) % 4]
        for i in range(W):
            for index in range(N + 1):
                for forward in (True, False):
                    u = SM.texel(h, i, forward, index)
                    for ex, ey in ((0, 0), (N - 1, N // 2)):
                        x, y = world_hit(ex, ey, h, i, forward, index)
                        # a forward crossing meets a face perpendicular to d: the coordinate along it is r's axis
                        along = (y if rx == 0 else x) if forward else (y if dx == 0 else x)
                        across = (x if rx == 0 else y) if forward else (x if dx == 0 else y)
                        assert across.denominator == 1                  # the hit lies on a cell boundary
                        assert u == frac8(along), (h, i, forward, index)
                        assert 0 <= u <= 7


def test_one_face_shows_the_same_stripes_from_two_cells_and_headings():
    """The west face of the wall cell (4, 3), seen from (1, 3) looking along +x (forward crossings) and from (3, 1)
    looking along +y (side crossings): every hit's texel is the eighth of its world y, whichever view it came from."""
    N = 7
    walls = np.zeros(N * N, dtype=bool)
    walls[3 * N + 4] = True
    seen = {}
    for (ex, ey, h, want_forward) in ((1, 3, 0, True), (3, 1, 1, False)):
        eighths = set()
        for i in range(W):
            tn, td, cell, xface, forward, index = SM.cast(walls, N, ex, ey, h, i)
            if cell != 3 * N + 4 or not xface:
                continue
            x, y = world_hit(ex, ey, h, i, forward, index)
            if x != 4:
                continue
            assert forward == want_forward and 3 <= y < 4
            u = SM.texel(h, i, forward, index)
            assert u == frac8(y)
            assert seen.setdefault(frac8(y), u) == u
            eighths.add(u)
        assert len(eighths) >= 4, (h, eighths)
    assert set(seen) == set(range(8))


# ---- frames ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [7, 21])
def test_a_styled_config_without_digits_renders_the_plain_bytes(N):
    rs = np.random.RandomState(N)
    lay = MM.random_layout(N, rs)
    kw = dict(random_start=True, random_goal=True, show_goal=True, view="first_person")
    styled, base = MazeConfig([lay], wall_styles=STYLES, **kw), MazeConfig([lay], **kw)
    assert not styled.styles[0].any()
    m = SM.host_batch(styled, 1)[0]
    for cell in base.free[0]:
        for h in range(4):
            m.x, m.y, m.h = int(cell) % N, int(cell) // N, h
            np.testing.assert_array_equal(m._render(), FP.render(base, 0, m.x, m.y, h, m.gx, m.gy))


@pytest.mark.parametrize("yface", [False, True])
def test_known_frame_of_a_striped_wall_straight_ahead(yface):
    """N = 7, a wall of style (200, 100, 50, 0b10101010) across the view, two cells ahead: every column hits it at t = 3/2
    (rows 14..69); odd eighths of a cell are halved, and a face crossed along y is scaled by 5 / 8 after that."""
    N, style = 7, (200, 100, 50, 0b10101010)
    cells = [["-"] * N for _ in range(N)]
    for j in range(1, 6):
        if yface:
            cells[3][j] = "1"                            # row y = 3, seen from (3, 1) looking along +y
        else:
            cells[j][3] = "1"                            # column x = 3, seen from (1, 3) looking along +x
    cfg = MazeConfig(["".join("".join(r) for r in cells)], True, True, view="first_person", wall_styles=[style])
    m = SM.host_batch(cfg, 1)[0]
    m.x, m.y, m.h = (3, 1, 1) if yface else (1, 3, 0)
    m.gx, m.gy = 6, 6
    img = m._render()
    full = np.array([125, 62, 31] if yface else [200, 100, 50])
    half = np.array([62, 31, 15] if yface else [100, 50, 25])
    assert (img[:14] == 0).all() and (img[70:] == 40).all()
    for i in range(W):
        q = 2 * i + 1 - W
        # the hit's coordinate along the wall: 3 1/2 +- (3/2) q / W (+ looking along +x, whose right is +y)
        c = Fraction(7, 2) + (Fraction(-3 * q, 2 * W) if yface else Fraction(3 * q, 2 * W))
        want = half if frac8(c) & 1 else full
        assert (img[14:70, i] == want).all(), i
    # a few columns by hand.  Looking along +x: q = 1, 3, 5 hit 3 1/2 + q / 56, eighth 4; q = 7 exactly 5/8, eighth 5;
    # q = -1 eighth 3.  Looking along +y the coordinate runs the other way: 3 1/2 - q / 56 is in eighth 3 for q = 1 .. 7
    # (3/8 exactly at q = 7) and in eighth 4 for q = -1
    for i, dark in ((42, yface), (43, yface), (44, yface), (45, True), (41, not yface)):
        assert (img[40, i] == (half if dark else full)).all(), i


# ---- generated landmarks -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_generated_layout_writes_the_models_landmarks(N):
    R = (N + 1) // 2
    kw = dict(gen_loops=min(3, 2 * R * (R - 1) - (R * R - 1)), gen_apples=4)
    for seed, density, S in ((1, 64, 7), (0xFFFF0000FFFF, 200, 3), (5, 256, 1), (6, 0, 2)):
        cfg = gen_config(N, wall_styles=STYLES[:S], gen_landmark_density=density, **kw)
        for g, ep in ((0, 0), (3, 1), (1000, 7)):
            walls, apples = GM.generate(N, kw["gen_loops"], 4, seed, g, ep)
            ids = SM.landmark_ids(N, walls, S, density, seed, g, ep)
            lay = cfg.generated_layout(seed, g, ep)
            assert lay == SM.layout_string(walls, apples, ids)
            assert (ids[~walls] == 0).all() and ids.max() <= S
            if density == 0:
                assert not any(ch.isdigit() for ch in lay)
            if density == 256:
                assert (ids[walls] > 0).all() and "+" not in lay
            if density == 64 and N > 7:
                assert 0 < (ids > 0).sum() < walls.sum()
            back = cfg.layout_config(lay)                # the styles survive the round trip
            assert back.wall_styles == cfg.wall_styles and back.generate is None
            np.testing.assert_array_equal(back.styles[0], ids)
            np.testing.assert_array_equal(back.walls[0], walls)
    # the unstyled layout of the same key is the same maze
    assert gen_config(N, **kw).generated_layout(1, 3, 1) == GM.layout_string(*GM.generate(N, kw["gen_loops"], 4, 1, 3, 1))


def test_landmarks_do_not_depend_on_actor_base():
    N, seed = 12, 9
    cfg = gen_config(N, gen_loops=1, wall_styles=STYLES, gen_landmark_density=100)
    a = SM.host_batch(cfg, 6, actor_base=0, actors_total=16, seed=seed)
    b = SM.host_batch(cfg, 2, actor_base=4, actors_total=16, seed=seed)
    for m in a + b:
        m.reset()
    for k in range(2):
        np.testing.assert_array_equal(a[4 + k].style_ids(), b[k].style_ids())
        np.testing.assert_array_equal(a[4 + k].actor_record(), b[k].actor_record())
        np.testing.assert_array_equal(a[4 + k].frame, b[k].frame)
        lay = cfg.generated_layout(seed, 4 + k, b[k].episode)
        assert lay == SM.layout_string(b[k].config.walls[0], b[k].config.apples[0], b[k].style_ids())
    assert len(a[0].actor_record()) == 8 + 18 + N * N + 65 + (N * N + 7) // 8
