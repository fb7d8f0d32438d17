"""Generated first-person mazes (MazeConfig(generate=N)): configuration checks, the block's words,
MazeConfig.generated_layout against the Kruskal restatement of tests/gen_maze_model.py, and the properties of the
layouts (no GPU)."""
import hashlib
from collections import deque

import numpy as np
import pytest

try:
    import gen_maze_model as GM
    import maze_model as MM
except ImportError:            # imported as tests.<module>
    from tests import gen_maze_model as GM
    from tests import maze_model as MM

SIZES = (7, 12, 14, 21)
ROOMS = {7: 4, 12: 6, 14: 7, 21: 11}


def _gen(N, **kw):
    from unreal_amd.environment.maze_environment import MazeConfig
    kw.setdefault("view", "first_person")
    kw.setdefault("random_start", True)
    kw.setdefault("random_goal", True)
    return MazeConfig(None, generate=N, **kw)


def _max_loops(N):
    R = ROOMS[N]
    return 2 * R * (R - 1) - (R * R - 1)


@pytest.mark.parametrize("kw", [
    dict(layouts=["-" * 49]),                                  # layouts with generate
    dict(view="top_down"), dict(random_start=False), dict(random_goal=False),
    dict(generate=8), dict(generate=0), dict(generate=7.0), dict(generate=True), dict(generate="7"),
    dict(gen_loops=-1), dict(gen_loops=_max_loops(7) + 1), dict(gen_loops=1.0), dict(gen_loops=True),
    dict(generate=21, gen_loops=_max_loops(21) + 1),
    dict(gen_apples=-1), dict(gen_apples=17), dict(gen_apples=2.0), dict(gen_apples=False),
    dict(generate=21, gen_apples=65), dict(generate=12, gen_apples=37),
    dict(goal_respawn=True),                                   # (needs max_episode_steps, as for any config)
    dict(action_set="jump"), dict(start_heading=4), dict(max_episode_steps=-1)])
def test_bad_generated_configs_raise(kw):
    from unreal_amd.environment.maze_environment import MazeConfig
    args = dict(layouts=None, generate=7, view="first_person", random_start=True, random_goal=True)
    args.update(kw)
    with pytest.raises(ValueError):
        MazeConfig(**args)


def test_generator_settings_without_generate_raise():
    from unreal_amd.environment.maze_environment import MazeConfig
    for kw in (dict(gen_loops=1), dict(gen_apples=1), dict(gen_loops=True)):
        with pytest.raises(ValueError):
            MazeConfig(["-" * 48 + "G"], random_start=True, **kw)
    with pytest.raises(ValueError):
        MazeConfig(None)
    with pytest.raises(ValueError):
        MazeConfig()
    with pytest.raises(ValueError):
        MazeConfig.reference().generated_layout(0, 0, 0)


def test_the_limits_of_loops_and_apples_are_accepted():
    for N in SIZES:
        R = ROOMS[N]
        cfg = _gen(N, gen_loops=_max_loops(N), gen_apples=min(64, R * R))
        assert cfg.nav and cfg.N == N and cfg.L == 0
        m = cfg.generated_layout(1, 2, 3)
        assert m.count("A") == min(64, R * R)
        assert len(m) - m.count("+") == R * R + 2 * R * (R - 1)       # every room and every edge open


def test_static_blocks_are_unchanged_word_for_word():
    """Blocks of configs without `generate`, against the hashes of the blocks these configs had before generated mazes
    existed."""
    from unreal_amd.environment.maze_environment import MazeConfig
    rs = np.random.RandomState(1234)
    want = {"ref": (75, "2b98dc91e8ea55ee8d2eebd4376665579af8d7ad549bd32d16b982d233030802"),
            "td12": (494, "042fe67afc4959a320563c02bfe7b2a5f7175431254281e0a3b7aed2ed6f54ae"),
            "fp21": (926, "07001083a566e1f64cf512bd4414291bf087ec5761b3cc32719818b338599c5d"),
            "nav14": (1132, "6d5a42d8f7f1ee06bf4ba8c021ba6721ad87af2fb3ee203a2bb28601380cad60")}
    got = {}
    got["ref"] = MazeConfig.reference().block(0)
    got["td12"] = MazeConfig([MM.random_layout(12, rs, marks="SG") for _ in range(3)], show_goal=True,
                             max_episode_steps=50).block(7)
    got["fp21"] = MazeConfig([MM.random_layout(21, rs) for _ in range(2)], True, True, view="first_person",
                             start_heading=2).block(2 ** 40 + 5)
    got["nav14"] = MazeConfig([MM.random_layout(14, rs, marks="AAAAA") for _ in range(4)], True, True, True, 30,
                              "first_person", None, 10, 2, 0, True, "lab").block(99)
    for name, (n, digest) in want.items():
        assert len(got[name]) == n, name
        assert hashlib.sha256(got[name].tobytes()).hexdigest() == digest, name
    for cfg in (MazeConfig.reference(),):
        assert cfg.generate is None and not cfg.flags & MazeConfig.GENERATED


def test_generated_block_words():
    from unreal_amd.environment.maze_environment import MazeConfig
    cfg = _gen(14, gen_loops=3, show_goal=True, max_episode_steps=40, start_heading=1)
    assert not cfg.nav and cfg.action_size == 4
    blk = cfg.block(0x1234567890)
    assert list(blk) == [14, 0, 1 | 2 | 4 | 16, 40, 0x34567890, 0x12, 18 + 196, 2, 1, 1, -1, 0, 3, 0, 0, 0]
    cfg = _gen(21, gen_loops=2, gen_apples=9, goal_reward=10, apple_reward=2, hit_reward=0, goal_respawn=True,
               max_episode_steps=99, action_set="lab")
    assert cfg.nav and cfg.action_size == 6 and cfg.reward_bound == 10
    blk = cfg.block(5)
    assert list(blk) == [21, 0, 1 | 2 | 8 | 16, 99, 5, 0, 18 + 441, 0, 10, 2, 0, 3, 2, 9, 0, 0]
    assert MazeConfig.GENERATED == 16
    assert list(cfg.layout_ids(5, 4, 100)) == [0, 0, 0, 0]


def test_register_maze_config_takes_the_generator_keywords():
    from unreal_amd.environment.environment import Environment
    try:
        Environment.register_maze_config("gen_reg", None, random_start=True, random_goal=True, view="first_person",
                                         generate=12, gen_loops=4, gen_apples=5, action_set="lab")
        cfg = Environment.MAZE_CONFIG["gen_reg"]
        assert (cfg.generate, cfg.gen_loops, cfg.gen_apples) == (12, 4, 5)
        assert Environment.get_action_size("maze", "gen_reg") == 6
        Environment.register_maze_config("gen_reg4", generate=7, random_start=True, random_goal=True,
                                         view="first_person")
        Environment.action_size = -1
        assert Environment.get_action_size("maze", "gen_reg4") == 4
        with pytest.raises(ValueError):
            Environment.register_maze_config("gen_bad", generate=7, view="first_person")
        assert "gen_bad" not in Environment.MAZE_CONFIG
    finally:
        Environment.action_size = -1
        for n in ("gen_reg", "gen_reg4"):
            Environment.MAZE_CONFIG.pop(n, None)


def _connected(walls, N):
    free = np.flatnonzero(~walls)
    seen, todo = {int(free[0])}, deque([int(free[0])])
    while todo:
        c = todo.popleft()
        x, y = c % N, c // N
        for nx, ny in ((x + 1, y), (x - 1, y), (x, y + 1), (x, y - 1)):
            d = ny * N + nx
            if 0 <= nx < N and 0 <= ny < N and not walls[d] and d not in seen:
                seen.add(d)
                todo.append(d)
    return len(seen) == len(free)


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("loops,apples", [(0, 0), (5, 0), (0, 7), (5, 16)])
def test_generated_layout_is_the_models(N, loops, apples):
    """MazeConfig.generated_layout (Prim) == the model (Kruskal) for several (seed, g, episode); the free cells are
    4-connected and 2 R^2 - 1 + loops in number; the apples lie on rooms, ascending, in the asked number; for even N the
    last row and column are walls."""
    cfg = _gen(N, gen_loops=loops, gen_apples=apples)
    R = ROOMS[N]
    cases = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2 ** 63 + 11, 4095, 7), (0xDEADBEEF, 123456, 2 ** 20)]
    cases += [(5, g, ep) for g in range(7) for ep in range(2)]
    seen = set()
    for seed, g, ep in cases:
        got = cfg.generated_layout(seed, g, ep)
        walls, cells = GM.generate(N, loops, apples, seed, g, ep)
        assert got == GM.layout_string(walls, cells), (seed, g, ep)
        assert set(got) <= set("+-A")
        assert int((~walls).sum()) == 2 * R * R - 1 + loops
        assert _connected(walls, N)
        assert len(cells) == apples and cells == sorted(set(cells))
        for c in cells:
            assert (c % N) % 2 == 0 and (c // N) % 2 == 0 and not walls[c]
        if N % 2 == 0:
            w2 = walls.reshape(N, N)
            assert w2[N - 1].all() and w2[:, N - 1].all()
        static = cfg.layout_config(got)                      # the layout is a valid static layout of the same options
        assert static.N == N and len(static.free[0]) == 2 * R * R - 1 + loops and list(static.apples[0]) == cells
        seen.add(got)
    assert len(seen) > len(cases) // 2                       # seed, actor and episode all enter the draw


@pytest.mark.parametrize("N", SIZES)
def test_the_31_71_97_241_free_cells_of_a_perfect_maze(N):
    cfg = _gen(N)
    m = cfg.generated_layout(3, 1, 4)
    assert len(m) - m.count("+") == {7: 31, 12: 71, 14: 97, 21: 241}[N]


def test_layouts_do_not_depend_on_how_actors_are_split():
    """The host models of global actors [0, 12) built whole, and as [0, 5) + [5, 12) with actor_base: the same layouts,
    goals, starts and headings through three episodes."""
    cfg = _gen(12, gen_loops=2, gen_apples=4)
    whole = GM.host_batch(cfg, 12, 0, 12, seed=77)
    parts = GM.host_batch(cfg, 5, 0, 12, seed=77) + GM.host_batch(cfg, 7, 5, 12, seed=77)
    for ep in range(3):
        for a, b in zip(whole, parts):
            assert a.g == b.g and a.episode == b.episode == ep
            np.testing.assert_array_equal(a.actor_record(), b.actor_record())
            assert (a.x, a.y, a.h, a.gx, a.gy) == (b.x, b.y, b.h, b.gx, b.gy)
            assert GM.layout_string(a.config.walls[0], a.config.apples[0]) == cfg.generated_layout(77, a.g, ep)
            np.testing.assert_array_equal(a.frame, b.frame)
        for m in whole + parts:
            m.reset()


def test_every_layout_of_512_actors_and_3_episodes_is_new_at_21():
    cfg = _gen(21)
    layouts = set(cfg.generated_layout(9, g, ep) for g in range(512) for ep in range(3))
    assert len(layouts) == 1536


def test_distinct_layouts_at_7_are_the_models_count():
    """A 4 x 4 room grid has about 10^5 spanning trees: collisions among 1536 are expected; the count is the model's."""
    cfg = _gen(7)
    got = set(cfg.generated_layout(9, g, ep) for g in range(512) for ep in range(3))
    want = set(GM.layout_string(*GM.generate(7, 0, 0, 9, g, ep)) for g in range(512) for ep in range(3))
    assert got == want and 1400 < len(got) <= 1536


def test_host_model_regenerates_at_every_reset_and_not_at_a_respawn():
    cfg = _gen(7, gen_apples=3, goal_respawn=True, max_episode_steps=40, show_goal=True)
    m = GM.host_batch(cfg, 1, seed=4)[0]
    rs = np.random.RandomState(0)
    layouts, respawns = [m.config.walls[0].copy()], 0
    for step in range(4000):
        before = m.config.walls[0]
        _, r, t, _ = m.process(int(rs.randint(0, 4)))
        assert m.config.walls[0] is before                   # a step, a respawn included, keeps the layout
        respawns += m.respawned
        if t:
            m.reset()
            layouts.append(m.config.walls[0].copy())
            rec = m.actor_record()
            assert len(rec) == 8 + 18 + 49 + 65 and rec[8 + 16] == 31 and rec[8 + 18 + 49] == 3
    assert respawns > 0 and len(layouts) == 101
    assert len(set(w.tobytes() for w in layouts)) > 90


def test_malformed_generated_maze_tails_are_refused_without_launch():
    """View 2 needs a block and per-actor records and, having no layout records, takes no layout array: every other
    tail is EINVAL on the host, so these fake device pointers never reach a kernel."""
    from unreal_amd.build import build_library
    from unreal_amd import _lib
    build_library(verbose=False)
    L = _lib.lib()
    dev = 1 << 20
    step = [4, 3, dev, None] + [dev] * 11 + [None, None] + [dev] * 3 + [1, 1]
    # (view, N, cfg, actor_base, goal, layout, ep_steps, episode, heading)
    for tail in ([2, 7, None, 0, dev, None, dev, dev, dev],          # no block
                 [2, 7, dev, 0, dev, None, dev, dev, None],          # no per-actor records
                 [2, 7, dev, 0, dev, dev, dev, dev, dev],            # a layout array: a tail built for another view
                 [2, 8, dev, 0, dev, None, dev, dev, dev],           # no such grid size
                 [2, 7, dev, 0, None, None, dev, dev, dev],          # no goal array
                 [1, 7, dev, 0, dev, None, dev, dev, dev],           # static first person needs its layout ids
                 [3, 7, dev, 0, dev, None, dev, dev, dev]):          # no such view
        assert L._fn["unreal_maze_step"](*step, *tail, None) == -22, tail
        assert L._fn["unreal_maze_reset"](4, 3, None, dev, dev, dev, dev, dev, *tail, None) == -22, tail
