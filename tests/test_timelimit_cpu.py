"""Time-limit bootstrapping and GAE(lambda), host side: argument validation, the options, the C ABI's refusals
and, on the host models alone, that the scripted traces of tests/timelimit_cases.py hold every case the GPU tests rely on
(so a drift of a config shows here)."""
import os

import numpy as np
import pytest

try:
    import timelimit_cases as TC
except ImportError:            # imported as tests.<module>
    from tests import timelimit_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def _trainer(env_type, env_name, **kw):
    """The constructor refuses a bad option before it touches the network or a device."""
    from unreal_amd.train.trainer import Trainer
    return Trainer(0, None, 1e-3, None, None, env_type, env_name, True, False, False, False, 0.05, 0.001, 5, 5, 0.99, 0.9, 40,
                   10 ** 6, "cuda:0", **kw)


def test_bootstrap_timeouts_is_refused_where_it_is_out_of_scope():
    from unreal_amd.environment.environment import Environment
    from unreal_amd.train.trainer import Trainer
    lay = TC.NAV_LAYOUTS[0]
    Environment.register_maze_config("tl_top_down", [lay.replace("A", "-")], max_episode_steps=5)
    Environment.register_maze_config("tl_sense", [lay], goal_sense=True, **TC.NAV_KW)
    Environment.register_maze_config("tl_no_limit", [lay], view="first_person")
    Environment.register_maze_config("tl_ok", [lay], goal_respawn=True, **TC.NAV_KW)
    for env_type, env_name, word in (("maze", "tl_top_down", "top-down"), ("maze", "no_such_config", "top-down"),
                                     ("maze", "tl_sense", "goal_sense"), ("maze", "tl_no_limit", "step limit"),
                                     ("lab", "nav_maze_static_01", "host-fed"), ("indoor", "x", "host-fed"),
                                     ("gym", "Breakout-v0", "host-fed")):
        with pytest.raises(ValueError, match=word):
            Trainer.check_rollout_options(env_type, env_name, True, None)
        with pytest.raises(ValueError, match=word):
            _trainer(env_type, env_name, bootstrap_timeouts=True)
        assert Trainer.check_rollout_options(env_type, env_name, False, 0.5) == (False, 0.5)     # GAE: every environment
    assert Trainer.check_rollout_options("maze", "tl_ok", True, None) == (True, None)
    assert Trainer.check_rollout_options("arcade", "anything", True, 1) == (True, 1.0)


@pytest.mark.parametrize("bad", [-0.01, 1.01, float("nan"), float("inf"), "0.9", True, [0.9]])
def test_gae_lambda_outside_the_unit_interval_is_refused(bad):
    from unreal_amd.train.trainer import Trainer
    with pytest.raises(ValueError, match="gae_lambda"):
        Trainer.check_rollout_options("maze", "", False, bad)
    with pytest.raises(ValueError, match="gae_lambda"):
        _trainer("arcade", "x", gae_lambda=bad)
    for good in (0, 0.0, 0.95, 1, 1.0):
        assert Trainer.check_rollout_options("maze", "", False, good) == (False, float(good))


def test_environments_refuse_a_store_out_of_scope():
    from unreal_amd.environment.maze_environment import MazeConfig, check_final_obs, batched_maze_environment
    lay = TC.NAV_LAYOUTS[0]
    check_final_obs(MazeConfig([lay], goal_respawn=True, **TC.NAV_KW))
    check_final_obs(TC.maze_config(TC.MAZE_CASES[2][1]))
    for conf in (None, MazeConfig([lay.replace("A", "-")], max_episode_steps=5), MazeConfig([lay], goal_sense=True, **TC.NAV_KW)):
        with pytest.raises(ValueError, match="out of scope"):
            check_final_obs(conf)
        with pytest.raises(ValueError, match="out of scope"):      # refused before any device memory is asked for
            batched_maze_environment(2, 3, "cuda:0", config=conf, final_obs=True)


def test_options_parse():
    from unreal_amd.options import get_options
    f = get_options("training", argv=[])
    assert f.bootstrap_timeouts is False and f.gae_lambda is None
    f = get_options("training", argv=["--bootstrap_timeouts", "True", "--gae_lambda", "0.95"])
    assert f.bootstrap_timeouts is True and f.gae_lambda == 0.95
    src = open(os.path.join(ROOT, "tools", "train_maze.py")).read()
    assert '"--bootstrap-timeouts"' in src and '"--gae-lambda"' in src


def test_entries_are_declared_named_and_refuse_bad_arguments_without_a_launch():
    """Fake device pointers: every call below is refused by the host check, so none reaches a kernel."""
    from unreal_amd.build import build_library
    from unreal_amd import _lib
    build_library(verbose=False)
    L = _lib.lib()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    names = ("unreal_arcade_rollout_step_tl", "unreal_arcade_policy_rollout_step_tl", "unreal_maze_rollout_step_tl",
             "unreal_maze_policy_rollout_step_tl", "unreal_boot_gather", "unreal_base_returns_tl")
    for name in names:
        assert name in L.protos and name in text, name
    dev = 1 << 20
    ring = [dev] * 16                          # pos .. score_valid
    roll = [dev] * 6 + [264, 256, 4, 0]        # active .. next_lar, lar_ld, lar_col0, A, idx_base_actor
    pol = [dev, 256] + [dev] * 8               # X, ldx, Wp, bp, Wv, bv, u, pi, v, actions_out
    arcade = [dev, 0, dev, dev, dev]           # cfg, actor_base, ep_steps, episode, records
    maze = lambda view: [view, 7, dev, 0] + [dev] * 5
    EINVAL = -22
    for store in (None, dev + 8):              # a null store, a misaligned one
        assert L._fn["unreal_arcade_rollout_step_tl"](4, 3, dev, *ring, *roll, *arcade, store, None) == EINVAL
        assert L._fn["unreal_arcade_policy_rollout_step_tl"](4, 3, *pol, *ring, *roll, *arcade, store, None) == EINVAL
        assert L._fn["unreal_maze_rollout_step_tl"](4, 3, dev, *ring, *roll, *maze(1), store, None) == EINVAL
        assert L._fn["unreal_maze_policy_rollout_step_tl"](4, 3, *pol, *ring, *roll, *maze(1), store, None) == EINVAL
    # views without a final-observation store: top-down, goal sense
    for view, tail in ((0, [0, 7, None, 0] + [None] * 5), (3, maze(3)), (4, [4, 7, dev, 0, dev, None, dev, dev, dev])):
        assert L._fn["unreal_maze_rollout_step_tl"](4, 3, dev, *ring, *roll, *tail, dev, None) == EINVAL, view
    # the scan: lambda outside [0, 1], a null pointer
    scan = lambda lam, r=dev: L._fn["unreal_base_returns_tl"](4, 5, r, dev, dev, dev, dev, 0.99, lam, dev, dev, None)
    assert scan(-0.1) == EINVAL and scan(1.5) == EINVAL and scan(float("nan")) == EINVAL and scan(0.9, None) == EINVAL
    # the gather: state without its sources, columns too narrow
    g = lambda **kw: L._fn["unreal_boot_gather"](*[kw.get(k, v) for k, v in (
        ("B", 4), ("T", 5), ("H1", 3), ("base", 0), ("final_base", 12), ("A", 4), ("count", dev), ("te", dev), ("n", dev),
        ("la", dev), ("lr", dev), ("actions", dev), ("rewards", dev), ("cc", dev), ("ch", dev), ("wc", dev), ("wh", dev),
        ("idx", dev), ("c0", dev), ("h0", dev), ("xcat", dev), ("ld", 264), ("col0", 256))], None)
    for bad in (dict(B=0), dict(T=0), dict(H1=1), dict(base=-1), dict(final_base=-1), dict(idx=None), dict(te=None),
                dict(wc=None), dict(h0=None), dict(ld=260), dict(A=256), dict(actions=None)):
        assert g(**bad) == EINVAL, bad


# ---- the traces ----------------------------------------------------------------------------------------------------------------
def test_the_breakout_anchor():
    """One row, one life, a 4-px paddle, ball speed 4, no self-serve, seed 1: fire then RIGHT loses the life at step 12
    whatever the actor; never firing ends only at the limit."""
    conf = TC.arcade_config(dict(TC.BREAKOUT, max_episode_steps=1000))
    for g, m in enumerate(TC.arcade_models(conf, TC.B)):
        for s in range(1, 13):
            _, _, t, _ = m.process(TC.fire_right(m))
            assert t == (s == 12), (g, s)
        assert "end_lives" in m.events
    m = TC.arcade_models(conf, 1)[0]
    for s in range(1, 1001):
        _, _, t, _ = m.process(TC.NOOP)
        assert t == (s == 1000)
    assert "end_timeout" in m.events


@pytest.mark.parametrize("k", range(len(TC.ARCADE_CASES)), ids=TC.ARCADE_NAMES)
def test_arcade_traces_hold_their_cases(k):
    name, settings, scripts, want = TC.ARCADE_CASES[k]
    conf, tr = TC.arcade_trace(k)
    assert want <= tr["kinds"], (name, want - tr["kinds"])
    assert set(np.unique(tr["flags"])) >= {0, 2} and len(tr["final"]) == int((tr["flags"] == 2).sum())
    assert not ((tr["flags"][1:] != 0) & (tr["flags"][:-1] != 0)).any()        # no two ends in a row: the ring discards none
    if name == "breakout-20":
        ends = {(s + 1, f) for s, f in zip(*np.nonzero(tr["flags"])) for f in [int(tr["flags"][s, f])]}
        assert {s for s, _ in ends} == {12, 20, 24, 36, 40}        # (true ends at 12, 24, 36; cuts at 20, 40)
    if name == "breakout-12":                                   # the step that loses the life and reaches the limit is a true end
        assert (tr["flags"][11] == [1, 2, 1, 2, 1, 2]).all()
    if name == "breakout-9":
        assert (tr["flags"][8] == 2).all() and not (tr["flags"] == 1).any()
    # the view test's batch of four: a truncated actor among the last two
    conf, tr4 = TC.arcade_trace(k, 4)
    assert (tr4["flags"][:, 2:] == 2).any(), name


@pytest.mark.parametrize("k", range(len(TC.MAZE_CASES)), ids=TC.MAZE_NAMES)
def test_maze_traces_hold_their_cases(k):
    name, args, kind, scripts, want = TC.MAZE_CASES[k]
    conf, tr = TC.maze_trace(k)
    assert conf.N == 7 and conf.max_episode_steps == 5 and conf.nav and conf.forage == (kind == "forage")
    assert want <= tr["kinds"], (name, want - tr["kinds"])
    assert len(tr["final"]) == int((tr["flags"] == 2).sum()) > 0
    assert not ((tr["flags"][1:] != 0) & (tr["flags"][:-1] != 0)).any()        # no two ends in a row: the ring discards none


def test_a_goal_in_the_timeout_step_is_a_cut_only_where_goals_respawn():
    """Actor 0 walks five cells to its goal with a limit of five steps."""
    _, respawn = TC.maze_trace(0)
    _, plain = TC.maze_trace(1)
    assert (respawn["actions"][:5] == plain["actions"][:5]).all()
    assert respawn["flags"][4, 0] == 2 and plain["flags"][4, 0] == 1
    assert respawn["rewards"][4, 0] == plain["rewards"][4, 0] == 1
    # actor 3 reaches its goal at step 3: no end with respawn (cut at 5), a true end without
    assert respawn["flags"][2, 3] == 0 and respawn["flags"][4, 3] == 2 and plain["flags"][2, 3] == 1
    conf, tr4 = TC.maze_trace(0, 4)
    assert (tr4["flags"][:, 2:] == 2).any()


def test_the_scan_in_numpy():
    """lambda = 1 is the n-step return, lambda = 0 the one-step TD error; flag 1 drops the bootstrap, 0 and 2 keep it."""
    r = np.array([[1.0], [0.0], [2.0]])
    v = np.array([[0.5], [0.25], [0.125]])
    for te, boot in ((0, 3.0), (2, 3.0), (1, 0.0)):
        R, adv = TC.gae_scan(r, v, [3], [3.0], [te], 0.5, 1.0)
        want = [1 + 0.5 * (0 + 0.5 * (2 + 0.5 * boot)), 0 + 0.5 * (2 + 0.5 * boot), 2 + 0.5 * boot]
        np.testing.assert_allclose(R[:, 0], want, rtol=1e-15)
        np.testing.assert_allclose(adv[:, 0], np.array(want) - v[:, 0], rtol=1e-15)
        R, adv = TC.gae_scan(r, v, [3], [3.0], [te], 0.5, 0.0)
        np.testing.assert_allclose(adv[:, 0], [1 + 0.5 * 0.25 - 0.5, 0.5 * 0.125 - 0.25, 2 + 0.5 * boot - 0.125], rtol=1e-15)
    R, adv = TC.gae_scan(r, v, [1], [3.0], [2], 0.5, 0.95)
    assert R[0, 0] == 1 + 0.5 * 3.0 and (R[1:] == 0).all() and (adv[1:] == 0).all()
