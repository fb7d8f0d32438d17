"""Exploration bonus without a GPU: option checks, flags, the entries' argument checks, hand-derivable
answers of the integer host model (tests/explore_model.py) that the GPU tests hold the kernels against, and the condition
the hash was chosen for: distinct views of a maze get distinct codes."""
import numpy as np
import pytest
import torch

try:
    import explore_model as EM
    import fp_maze_model as FM
    import maze_model as MM
    import philox_model as PH
except ImportError:            # imported as tests.<module>
    from tests import explore_model as EM
    from tests import fp_maze_model as FM
    from tests import maze_model as MM
    from tests import philox_model as PH


@pytest.fixture(scope="module")
def built():
    from unreal_amd.build import build_library
    return build_library(verbose=False)


def test_check_explore_options():
    from unreal_amd.train.trainer import Trainer
    chk = Trainer.check_explore_options
    assert chk("maze", 0.0) == (0.0, 7, 8, 22) and chk("arcade", 0.05, 4, 64, 10) == (0.05, 4, 64, 10)
    assert chk("maze", 1, 21, 2, 26) == (1.0, 21, 2, 26)
    for cell in (4, 6, 7, 12, 14, 21):
        assert chk("maze", 0.1, cell)[1] == cell
    for env_type in ("lab", "indoor", "gym"):
        assert chk(env_type, 0.0) == (0.0, 7, 8, 22)                # off: every environment
        with pytest.raises(ValueError, match="host-fed"):
            chk(env_type, 0.01)
    for bad in (-0.1, float("nan"), float("inf"), True, "0.1", None):
        with pytest.raises(ValueError, match="explore_beta"):
            chk("maze", bad)
    for bad in (0, 1, 2, 3, 5, 28, 42, 84, 7.0, True, "7", None):
        with pytest.raises(ValueError, match="explore_cell"):
            chk("maze", 0.1, bad)
    for bad in (1, 65, 0, -8, 8.0, True, None):
        with pytest.raises(ValueError, match="explore_levels"):
            chk("maze", 0.1, 7, bad)
    for bad in (9, 27, 0, 22.0, True, None):
        with pytest.raises(ValueError, match="explore_bits"):
            chk("maze", 0.1, 7, 8, bad)
    with pytest.raises(ValueError, match="explore_bits"):
        chk("maze", 0.0, 7, 8, 9)                                   # checked even when the option is off


def test_trainer_refuses_before_touching_the_device():
    from unreal_amd.train.trainer import Trainer
    args = (0, None, 7e-4, None, None, "lab", "nav_maze_static_01", True, True, True, True, 0.05, 0.001, 20, 20, 0.99, 0.9,
            2000, 10 ** 6, "cuda:0")
    with pytest.raises(ValueError, match="host-fed"):
        Trainer(*args, explore_beta=0.01)
    with pytest.raises(ValueError, match="explore_cell"):
        Trainer(*args, explore_cell=5)


def test_flag_names_and_defaults():
    from unreal_amd.options import get_options
    f = get_options("training")
    assert (f.explore_beta, f.explore_cell, f.explore_levels, f.explore_bits) == (0.0, 7, 8, 22)
    g = get_options("training", argv=["--explore_beta", "0.05", "--explore_cell", "4", "--explore_levels", "16",
                                      "--explore_bits", "20"])
    assert (g.explore_beta, g.explore_cell, g.explore_levels, g.explore_bits) == (0.05, 4, 16, 20)
    assert isinstance(g.explore_cell, int) and isinstance(g.explore_bits, int)


def test_stream_constant_is_new():
    """The multipliers' Philox stream collides with none of the streams the kernels and the host already draw from."""
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "unreal_amd", "csrc")
    seen = {}
    for name in sorted(os.listdir(root)):
        for m in re.finditer(r"(k\w+Stream)\s*=\s*(0x[0-9A-Fa-f]+)u", open(os.path.join(root, name)).read()):
            seen[m.group(1)] = int(m.group(2), 16)
    assert seen.pop("kExploreStream") == EM.STREAM == 0x4558504C
    assert len(seen) >= 7 and EM.STREAM not in seen.values(), seen
    from unreal_amd import ops
    assert ops.EXPLORE_STREAM == EM.STREAM


def _with(good, **kw):
    a = list(good)
    for k, v in kw.items():
        a[int(k[1:])] = v
    return a


def test_entries_refuse_bad_arguments_without_launch(built):
    """Fake device pointers: every call below is refused on the host, so none of them reaches a kernel."""
    from unreal_amd import _lib
    L = _lib.lib()
    dev = 1 << 20
    # unreal_explore_multipliers(F, seed, mult)
    fn = L._fn["unreal_explore_multipliers"]
    for a in ([0, 1, dev], [-1, 1, dev], [1324, 1, dev], [432, 1, None]):
        assert fn(*a, None) == -22, a
    # unreal_frame_codes
    fn = L._fn["unreal_frame_codes"]
    #       rows frames stride n  H   W   idx  B  act  ns   te  cell lev vmax bits mult codes
    good = [8, dev, 21168, 16, 84, 84, dev, 4, dev, dev, dev, 7, 8, 255, 22, dev, dev]
    assert len(good) == len(L.protos["unreal_frame_codes"]) - 1
    bad = [_with(good, _0=0), _with(good, _0=-1), _with(good, _3=0), _with(good, _4=0), _with(good, _5=-84),
           _with(good, _2=21167), _with(good, _2=21160), _with(good, _2=21176),         # stride: short, not a multiple of 16
           _with(good, _1=dev + 8),                                                    # frames not 16-byte aligned
           _with(good, _11=5), _with(good, _11=1), _with(good, _11=0), _with(good, _11=8),      # cell: 84 = 2 2 3 7
           _with(good, _11=2), _with(good, _11=3),                                     # F = 5292, 2352 > 1323
           _with(good, _12=1), _with(good, _12=65), _with(good, _13=0), _with(good, _13=256),
           _with(good, _14=9), _with(good, _14=27),
           _with(good, _8=None), _with(good, _9=None), _with(good, _10=None), _with(good, _7=0),   # half a gate
           _with(good, _4=24, _5=36, _2=24 * 36 * 3, _11=8), _with(good, _4=24, _5=36, _2=24 * 36 * 3, _11=9)]   # cell divides H only / W only
    bad += [_with(good, **{"_%d" % k: None}) for k in (1, 6, 15, 16)]
    for a in bad:
        assert fn(*a, None) == -22, a
    with pytest.raises(_lib.UnrealLibError):
        L.call("unreal_frame_codes", *_with(good, _11=5), None)
    # unreal_count_add(rows, codes, table, bits)
    fn = L._fn["unreal_count_add"]
    for a in ([0, dev, dev, 22], [8, None, dev, 22], [8, dev, None, 22], [8, dev, dev, 9], [8, dev, dev, 27]):
        assert fn(*a, None) == -22, a
    # unreal_count_bonus
    fn = L._fn["unreal_count_bonus"]
    #       rows codes table bits beta rewards act idx n_slots bonus total r_bonus stats_i stats_f
    good = [8, dev, dev, 22, 0.05, dev, dev, dev, 64, dev, dev, dev, dev, dev]
    assert len(good) == len(L.protos["unreal_count_bonus"]) - 1
    bad = [_with(good, _0=0), _with(good, _3=9), _with(good, _3=27), _with(good, _4=-0.5), _with(good, _4=float("nan")),
           _with(good, _4=float("inf")), _with(good, _6=None), _with(good, _7=None), _with(good, _8=0)]
    bad += [_with(good, **{"_%d" % k: None}) for k in (1, 2, 5, 9, 10, 12, 13)]
    for a in bad:
        assert fn(*a, None) == -22, a
    # unreal_vr_returns_bonus
    fn = L._fn["unreal_vr_returns_bonus"]
    good = [5, 4, dev, dev, dev, dev, dev, dev, 0.99, dev]
    assert len(good) == len(L.protos["unreal_vr_returns_bonus"]) - 1
    bad = [_with(good, _0=0), _with(good, _1=1)] + [_with(good, **{"_%d" % k: None}) for k in (2, 3, 4, 5, 6, 7, 9)]
    for a in bad:
        assert fn(*a, None) == -22, a


def test_wrappers_have_no_cpu_fallback(built):
    from unreal_amd import ops
    x, xi, xb = torch.zeros(4096), torch.zeros(4096, dtype=torch.int32), torch.zeros(16 * 21168, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.frame_codes(8, xb, 21168, 16, 84, 84, xi, 7, 8, 255, 22, xi, xi)
    with pytest.raises(ValueError, match="cell"):
        ops.frame_codes(8, xb, 21168, 16, 84, 84, xi, 5, 8, 255, 22, xi, xi)
    with pytest.raises(ValueError, match="features"):
        ops.frame_codes(8, xb, 21168, 16, 84, 84, xi, 2, 8, 255, 22, xi, xi)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.count_add(8, xi, xi, 10)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.count_bonus(8, xi, xi, 10, 0.1, x, xi, xi, x, x, x, xi, x)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.explore_multipliers(432, 7, xi)
    with pytest.raises(ValueError, match="beta"):
        ops.count_bonus(8, xi, xi, 10, -1.0, x, xi, xi, x, x, x, xi, x)


# ---- hand answers of the model ---------------------------------------------------------------------------------------------
CELL, LEVELS, BITS = 7, 8, 22
MULT = EM.multipliers(EM.n_features(84, 84, CELL), 0xA3C)


def test_multipliers_are_odd_words_of_the_stream():
    assert MULT.shape == (432,) and (MULT & np.uint64(1)).all() and int(MULT.max()) < 1 << 32
    w = PH.philox4x32_10(0xA3C, np.arange(432, dtype=np.uint64), 0x4558504C)[0]
    np.testing.assert_array_equal(MULT, w | np.uint64(1))
    assert len(np.unique(MULT)) == 432


def test_blank_and_saturated_frames():
    for vmax in (1, 100, 255):
        z = np.zeros((1, 84, 84, 3), np.uint8)
        assert (EM.levels_of(z, CELL, LEVELS, vmax) == 0).all() and EM.hash_of(EM.levels_of(z, CELL, LEVELS, vmax), MULT)[0] == 0
        assert EM.codes_of(z, CELL, LEVELS, vmax, BITS, MULT)[0] == 0
        full = np.full((1, 84, 84, 3), vmax, np.uint8)
        for levels in (2, 8, 64):
            # S = M = vmax cell^2 gives M levels // (M + 1): the top level whenever levels <= M + 1.  (vmax 1 at cell 7
            # has M + 1 = 50 < 64: the 64 levels are then more than the 50 sums there are, and the top one is 62.)
            top = levels - 1 if levels <= vmax * CELL * CELL + 1 else 62
            assert (EM.levels_of(full, CELL, levels, vmax) == top).all()
        assert (EM.levels_of(np.full((1, 84, 84, 3), 255, np.uint8), CELL, LEVELS, vmax) == LEVELS - 1).all()   # clamped


def test_one_pixel_across_a_level_edge_changes_exactly_that_feature():
    # vmax 255, cell 7, 8 levels: level = 8 S // 12496, so level 1 starts at S = 1562 = 6 * 255 + 32
    base = np.zeros((84, 84, 3), np.uint8)
    y0, x0, c = 14, 35, 1                                           # cell (2, 5), channel 1: feature (2 * 12 + 5) * 3 + 1
    f = (2 * 12 + 5) * 3 + 1
    base[y0:y0 + 6, x0 + 3, c] = 255
    frames = np.stack([base.copy() for _ in range(3)])
    frames[0, y0 + 6, x0 + 6, c] = 30
    frames[1, y0 + 6, x0 + 6, c] = 31                               # S = 1561: stops just below the edge
    frames[2, y0 + 6, x0 + 6, c] = 32                               # S = 1562: crosses it
    lv = EM.levels_of(frames, CELL, LEVELS, 255)
    np.testing.assert_array_equal(lv[0], lv[1])
    assert (lv[0] == 0).all()
    want = np.zeros(432, np.int64)
    want[f] = 1
    np.testing.assert_array_equal(lv[2], want)
    codes = EM.codes_of(frames, CELL, LEVELS, 255, BITS, MULT)
    assert codes[0] == codes[1] == 0 and codes[2] == ((int(MULT[f]) * EM.GOLDEN) & EM.M32) >> (32 - BITS)
    # the pixel next door belongs to the neighbouring cell, the next byte to the neighbouring channel
    other = base.copy()
    other[y0 + 6, x0 + 7, c] = 255
    assert EM.levels_of(other[None], CELL, LEVELS, 255)[0, f] == 0


def test_bytes_above_vmax_are_clamped():
    rs = np.random.RandomState(3)
    fr = rs.randint(0, 256, (4, 84, 84, 3)).astype(np.uint8)
    for vmax in (1, 100):
        np.testing.assert_array_equal(EM.cell_sums(fr, CELL, vmax), EM.cell_sums(np.minimum(fr, vmax), CELL, 255))
        np.testing.assert_array_equal(EM.codes_of(fr, CELL, LEVELS, vmax, BITS, MULT),
                                      EM.codes_of(np.minimum(fr, vmax), CELL, LEVELS, vmax, BITS, MULT))
    assert (EM.cell_sums(fr, CELL, 255) == fr.astype(np.int64).reshape(4, 12, 7, 12, 7, 3).sum((2, 4)).reshape(4, -1)).all()


def test_feature_order_on_a_frame_that_is_not_square():
    fr = np.zeros((1, 24, 36, 3), np.uint8)
    fr[0, 13, 30, 2] = 255                                          # cell 4: row 3, column 7 of 6 x 9 cells
    s = EM.cell_sums(fr, 4, 255)[0]
    assert s.shape == (6 * 9 * 3,) and s[(3 * 9 + 7) * 3 + 2] == 255 and s.sum() == 255


def test_earning_rows_counts_and_bonus():
    act = np.array([[1, 1, 1, 1], [1, 0, 1, 1], [1, 0, 1, 0]])
    n, te = np.array([3, 1, 3, 2]), np.array([0, 1, 2, 1])
    np.testing.assert_array_equal(EM.earning(act, n, te), [[1, 0, 1, 1], [1, 0, 1, 0], [1, 0, 0, 0]])
    table = np.zeros(1024, np.int64)
    table[5] = 3
    codes = np.array([5, 5, 7, -1, 1024])
    EM.count_add(table, codes)
    assert table[5] == 5 and table[7] == 1 and table.sum() == 6
    b, earn, first = EM.bonus_of(table, codes, 0.5)
    np.testing.assert_allclose(b, [0.5 / np.sqrt(5), 0.5 / np.sqrt(5), 0.5, 0, 0], rtol=1e-15)
    assert (earn, first) == (3, 1)


# ---- the condition on the hash: distinct views get distinct codes -------------------------------------------------------------
def _layout(N, seed):
    return MM.random_layout(N, np.random.RandomState(seed))


def _distinct(frames):
    return len({f.tobytes() for f in frames})


def test_first_person_views_of_a_maze_get_distinct_codes():
    from unreal_amd.environment.maze_environment import MazeConfig
    conf = MazeConfig([_layout(7, 11)], view="first_person", show_goal=True)
    N = conf.N
    gx, gy = conf.goal[0] % N, conf.goal[0] // N
    free = [c for c in range(N * N) if not conf.walls[0][c]]
    frames = [FM.render(conf, 0, c % N, c // N, h, gx, gy) for c in free for h in range(4)]
    n_frames = _distinct(frames)
    codes = EM.codes_of(np.stack(frames), 7, 8, 255, 22, MULT)
    assert len(frames) == 4 * len(free) and n_frames > len(free)
    assert len(np.unique(codes)) == n_frames, (len(np.unique(codes)), n_frames)


def test_top_down_views_of_a_maze_get_distinct_codes():
    from unreal_amd.environment.maze_environment import MazeConfig
    conf = MazeConfig([_layout(7, 11)], show_goal=True)
    N = conf.N
    free = [c for c in range(N * N) if not conf.walls[0][c]]
    gx, gy = conf.goal[0] % N, conf.goal[0] // N
    frames = [MM.render(conf, 0, c % N, c // N, gx, gy).astype(np.uint8) for c in free]
    assert max(int(f.max()) for f in frames) == 1                    # bytes 0 / 1: vmax = 1
    n_frames = _distinct(frames)
    assert n_frames == len(free)
    codes = EM.codes_of(np.stack(frames), 7, 8, 1, 22, MULT)
    assert len(np.unique(codes)) == n_frames, (len(np.unique(codes)), n_frames)
    # with the first-person byte range the same frames all quantise to level 0: the range must be the environment's
    assert len(np.unique(EM.codes_of(np.stack(frames), 7, 8, 255, 22, MULT))) == 1
