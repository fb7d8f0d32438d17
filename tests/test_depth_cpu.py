"""Depth prediction for first-person mazes, the parts that need no GPU: the host model of the labels on
hand-derivable views, the class census of empty rooms, the parameter layout, the refusals and the entries' argument
checks."""
import os
import re

import numpy as np
import pytest

try:
    import depth_model as DM
    import fp_maze_model as FP
except ImportError:            # imported as tests.<module>
    from tests import depth_model as DM
    from tests import fp_maze_model as FP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _walls(N, cells=()):
    w = np.zeros(N * N, dtype=bool)
    for x, y in cells:
        w[y * N + x] = True
    return w


# ---- labels one can derive by hand ----------------------------------------------------------------------------------------
def test_positions_are_band_centres_with_odd_q():
    cols = [DM.column(j) for j in range(DM.POSITIONS)]
    assert cols == list(range(3, 84, 7)) and len(cols) == 12 and cols[-1] + 3 == 83
    assert all((2 * i + 1 - 84) % 2 == 1 for i in cols)
    assert 2 * DM.column(7) + 1 - 84 == 21
    assert DM.EDGES == (1, 2, 3, 4, 6, 8, 12) and DM.CLASSES == len(DM.EDGES) + 1


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 6])
def test_corridor_seen_end_on(d):
    """A camera at (0, 3) of a 7 x 7 map looking along +x at a wall d cells ahead: the two centre columns (|q| = 7 cross
    their first side boundary at t = 6) run straight into it at t = (d - 1) + 1/2."""
    N = 7
    side = [(x, y) for x in range(N) for y in (2, 4)]          # the corridor's walls
    w = _walls(N, side + [(d, 3)])
    rays = DM.rays(w, N, 0, 3, 0)
    k = d - 1
    assert rays[5] == (2 * k + 1, 2) and rays[6] == (2 * k + 1, 2)
    want = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 4}[k]              # t = 0.5, 1.5, 2.5, 3.5, 4.5, 5.5 against the edges
    lab = DM.labels(w, N, 0, 3, 0)
    assert lab[5] == lab[6] == want and lab.dtype == np.uint8 and lab.shape == (12,)
    assert (lab <= want).all()                                   # the corridor's side walls are never farther than its end


@pytest.mark.parametrize("h", [0, 1, 2, 3])
def test_adjacent_wall_is_class_zero_everywhere(h):
    """A wall cell right ahead: every column crosses the forward boundary at t = 1/2 before its first side boundary
    (84 / 2|q| >= 84 / 154 > 1/2), so all twelve positions are class 0.  The map border ahead does the same."""
    N = 12
    dx, dy = FP.DIRS[h]
    w = _walls(N, [(5 + dx, 5 + dy)])
    assert DM.rays(w, N, 5, 5, h) == [(1, 2)] * 12
    assert (DM.labels(w, N, 5, 5, h) == 0).all()
    ex, ey = (N - 1 if dx > 0 else 0 if dx < 0 else 5), (N - 1 if dy > 0 else 0 if dy < 0 else 5)
    assert (DM.labels(_walls(N), N, ex, ey, h) == 0).all()


def test_a_ray_exactly_on_an_edge_lands_in_the_upper_class():
    """q = 21 (position 7) crosses side boundary m at t = (2m + 1) 84 / 42 = 2 (2m + 1).  From the bottom row looking
    along +x (right is +y) its first side step leaves the map at t = 2 exactly: class 2 (edges 1 and 2), not 1."""
    N = 7
    w = _walls(N)
    tn, td = DM.rays(w, N, 0, N - 1, 0)[7]
    assert (tn, td) == (84, 42) and tn == 2 * td and DM.on_edge(tn, td)
    assert DM.depth_class(tn, td) == 2 == DM.labels(w, N, 0, N - 1, 0)[7]
    # one row up the same column leaves at m = 1, t = 6: class 5 (edges 1, 2, 3, 4, 6)
    tn, td = DM.rays(w, N, 0, N - 2, 0)[7]
    assert tn == 6 * td and DM.depth_class(tn, td) == 5
    # just below an edge stays in the lower class
    assert DM.depth_class(2 * 42 - 1, 42) == 1 and DM.depth_class(12 * 5, 5) == 7 and DM.depth_class(12 * 5 - 1, 5) == 6


@pytest.mark.parametrize("N,used,edge_rays", [(7, 6, 128), (12, 7, 448), (14, 8, 576), (21, 8, 1024)])
def test_class_census_of_an_empty_room(N, used, edge_rays):
    """Over every cell and heading of an empty room: which classes occur, none of them rare, how many rays end exactly
    on an edge, and the size of the integers the kernel compares."""
    counts, edge, big = DM.room_census(N)
    assert counts.sum() == N * N * 4 * 12
    assert list(np.flatnonzero(counts)) == list(range(used))
    assert (counts[:used] / float(counts.sum())).min() >= 0.05
    assert edge == edge_rays
    assert big <= 3108 and 2 * 12 * big < 2 ** 31


def test_pickups_goal_and_styles_do_not_change_depth():
    """The model reads walls alone: a styled wall is a wall, an apple or goal cell is free."""
    from unreal_amd.environment.maze_environment import MazeConfig
    rows = ["S--A---", "-+-2---", "---1--G", "-------", "--+----", "---B---", "-------"]
    styled = MazeConfig([rows], view="first_person", wall_styles=[(200, 10, 10, 0x0F), (10, 200, 10, 0xAA)],
                        pickups=[(5, (1, 2, 3), False)])
    plain = MazeConfig([[r.replace("A", "-").replace("B", "-").replace("1", "+").replace("2", "+") for r in rows]],
                       view="first_person")
    np.testing.assert_array_equal(styled.walls[0], plain.walls[0])
    for (x, y, h) in ((0, 0, 0), (3, 3, 3), (6, 6, 2), (2, 5, 1)):
        np.testing.assert_array_equal(DM.labels(styled.walls[0], 7, x, y, h), DM.labels(plain.walls[0], 7, x, y, h))


# ---- parameters ---------------------------------------------------------------------------------------------------------------
def test_param_spec_appends_exactly_the_four_variables():
    from unreal_amd.model.model import param_spec, FlatParams
    for kw in (dict(), dict(use_lstm=False), dict(use_pixel_change=False, use_reward_prediction=False),
               dict(objective_size=3), dict(use_lstm=False, use_pixel_change=False, use_value_replay=False,
                                            use_reward_prediction=False)):
        for A in (4, 6):
            base = param_spec(A, **kw)
            assert param_spec(A, use_depth_prediction=False, **kw) == base
            with_head = param_spec(A, use_depth_prediction=True, **kw)
            assert with_head[:len(base)] == base
            assert with_head[len(base):] == [("W_dp_fc1", (256, 128), 256), ("b_dp_fc1", (128,), 256),
                                             ("W_dp_fc2", (128, 96), 128), ("b_dp_fc2", (96,), 128)]
    assert len(param_spec(4)) == 20 and len(param_spec(4, use_depth_prediction=True)) == 24
    # the flat layout of every other variable is what it is without the head
    a, b = FlatParams(param_spec(4), "cpu"), FlatParams(param_spec(4, use_depth_prediction=True), "cpu")
    assert all(b.offsets[k] == v for k, v in a.offsets.items())
    assert b.n_params == a.n_params + 256 * 128 + 128 + 128 * 96 + 96


def test_options_have_the_flags():
    from unreal_amd.options import get_options
    f = get_options("training", preset="lab", argv=[])
    assert f.use_depth_prediction is False and f.depth_lambda == 1.0
    f = get_options("training", preset="lab", argv=["--use_depth_prediction", "true", "--depth_lambda", "0.33"])
    assert f.use_depth_prediction is True and f.depth_lambda == 0.33


def test_header_constants_and_doc():
    from unreal_amd import ops
    src = open(os.path.join(ROOT, "include", "unreal_hip.h")).read()
    assert int(re.search(r"#define UNREAL_DEPTH_POSITIONS (\d+)", src).group(1)) == ops.DEPTH_POSITIONS == DM.POSITIONS
    assert int(re.search(r"#define UNREAL_DEPTH_CLASSES (\d+)", src).group(1)) == ops.DEPTH_CLASSES == DM.CLASSES
    assert ops.DEPTH_EDGES == DM.EDGES
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "unreal_maze_depth_labels" in text and "unreal_depth_loss_grad" in text


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_option_is_refused_outside_first_person_mazes():
    from unreal_amd import ops
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.maze_environment import (MazeConfig, BatchedMazeEnvironment, batched_maze_environment,
                                                         check_depth_labels, REFERENCE_MAP)
    from unreal_amd.environment.arcade_environment import BatchedArcadeEnvironment, ArcadeConfig
    from unreal_amd.environment.hostfed_environment import HostFedEnvironment
    from unreal_amd.train.trainer import Trainer
    top = MazeConfig([REFERENCE_MAP])
    fp = MazeConfig([REFERENCE_MAP], view="first_person")
    # the environment
    check_depth_labels(fp)
    for conf in (None, top):
        with pytest.raises(ValueError, match="first_person"):
            check_depth_labels(conf)
        with pytest.raises(ValueError, match="first_person"):
            BatchedMazeEnvironment(2, 2, "cpu", config=conf, depth_labels=True)
        with pytest.raises(ValueError, match="first_person"):
            batched_maze_environment(2, 2, "cpu", config=conf, depth_labels=True)
    with pytest.raises(ValueError, match="arcade"):
        BatchedArcadeEnvironment(2, 2, "cpu", config=ArcadeConfig(), depth_labels=True)
    with pytest.raises(ValueError, match="host-fed"):
        HostFedEnvironment(None, 2, 2, "cpu", depth_labels=True)
    # ops
    with pytest.raises(ValueError):
        ops.Ring(2, 2, "cpu", depth=True)                        # no maze state: not a device maze's ring
    for maze in (None, (ops.MAZE_TOP_DOWN, 7, None, 0)):
        with pytest.raises(ValueError, match="first-person"):
            ops.check_depth_maze(maze)
        with pytest.raises(ValueError, match="first-person"):
            ops.maze_depth_labels(None, maze)
    ops.check_depth_maze((ops.MAZE_FIRST_PERSON_GENERATED_FORAGE, 7, None, 0))
    # the trainer
    Environment.register_maze_config("depth_cpu_top", [REFERENCE_MAP])
    Environment.register_maze_config("depth_cpu_fp", [REFERENCE_MAP], view="first_person")
    try:
        assert Trainer.check_depth_prediction("maze", "depth_cpu_fp", True, 0.5) == (True, 0.5)
        assert Trainer.check_depth_prediction("arcade", "x", False) == (False, 1.0)       # off: nothing is checked
        for env_type, name in (("maze", ""), ("maze", "depth_cpu_top"), ("arcade", "breakout"), ("lab", "nav_maze_static_01"),
                               ("indoor", "rooms"), ("gym", "Pong")):
            with pytest.raises(ValueError, match="first-person|first_person"):
                Trainer.check_depth_prediction(env_type, name, True)
        for lam in (-1.0, float("inf"), float("nan"), True, "1"):
            with pytest.raises(ValueError, match="depth_lambda"):
                Trainer.check_depth_prediction("maze", "depth_cpu_fp", True, lam)
    finally:
        Environment.MAZE_CONFIG.pop("depth_cpu_top", None)
        Environment.MAZE_CONFIG.pop("depth_cpu_fp", None)


# ---- the entries ----------------------------------------------------------------------------------------------------------------
def test_entries_are_exported_and_refuse_bad_arguments_without_launch():
    """-EINVAL on the host, so these fake device pointers never reach a kernel."""
    from unreal_amd.build import build_library
    from unreal_amd import _lib
    build_library(verbose=False)
    L = _lib.lib()
    assert "unreal_maze_depth_labels" in L.protos and "unreal_depth_loss_grad" in L.protos
    dev = 1 << 20
    fn = L._fn["unreal_maze_depth_labels"]
    # (B, H1, N, count, pos, heading, record_words, cfg, layout, r_depth)
    for args in ([0, 3, 7, dev, dev, dev, 0, dev, dev, dev],             # B <= 0
                 [-2, 3, 7, dev, dev, dev, 0, dev, dev, dev],
                 [4, 0, 7, dev, dev, dev, 0, dev, dev, dev],             # H1 <= 0
                 [4, 3, 8, dev, dev, dev, 0, dev, dev, dev],             # a grid size the frame does not tile into
                 [4, 3, 0, dev, dev, dev, 0, dev, dev, dev],
                 [4, 3, 7, None, dev, dev, 0, dev, dev, dev],            # no count
                 [4, 3, 7, dev, None, dev, 0, dev, dev, dev],            # no pos
                 [4, 3, 7, dev, dev, None, 0, dev, dev, dev],            # no heading
                 [4, 3, 7, dev, dev, dev, 0, None, dev, dev],            # no block
                 [4, 3, 7, dev, dev, dev, 0, dev, dev, None],            # no labels
                 [4, 3, 7, dev, dev, dev, -1, dev, dev, dev],            # record widths: negative, shorter than the 8 words
                 [4, 3, 7, dev, dev, dev, 7, dev, dev, dev],
                 [4, 3, 7, dev, dev, dev, 0, dev, None, dev],            # generated (no layout array) without records
                 [4, 3, 7, dev, dev, dev, 8 + 18 + 49 + 64, dev, None, dev],        # ... or records one word short
                 [4, 3, 21, dev, dev, dev, 8 + 18 + 49 + 65, dev, None, dev]):      # ... or those of a smaller maze
        assert fn(*args, None) == -22, args
    fn = L._fn["unreal_depth_loss_grad"]
    # (rows, logits, ld, r_depth, frame_idx, active, scale, dlogits, loss, hits)
    for args in ([0, dev, 96, dev, dev, dev, 1.0, dev, dev, dev],        # rows <= 0
                 [-1, dev, 96, dev, dev, dev, 1.0, dev, dev, dev],
                 [5, dev, 95, dev, dev, dev, 1.0, dev, dev, dev],        # a row shorter than the 96 logits
                 [5, dev, 0, dev, dev, dev, 1.0, dev, dev, dev],
                 [5, None, 96, dev, dev, dev, 1.0, dev, dev, dev],       # no logits
                 [5, dev, 96, None, dev, dev, 1.0, dev, dev, dev],       # no labels
                 [5, dev, 96, dev, None, dev, 1.0, dev, dev, dev],       # no frame indices
                 [5, dev, 96, dev, dev, None, 1.0, dev, dev, dev],       # no row mask
                 [5, dev, 96, dev, dev, dev, 1.0, dev, None, dev],       # no loss
                 [5, dev, 96, dev, dev, dev, 1.0, dev, dev, None],       # no hits
                 [2 ** 31 // 12, dev, 96, dev, dev, dev, 1.0, dev, dev, dev]):      # rows * 12 beyond int32
        assert fn(*args, None) == -22, args
    with pytest.raises(_lib.UnrealLibError):
        L.call("unreal_depth_loss_grad", 0, dev, 96, dev, dev, dev, 1.0, None, dev, dev, None)
