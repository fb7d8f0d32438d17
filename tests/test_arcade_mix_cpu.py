"""CPU tests of game mixtures: ArcadeMix and its registration, the block, the assignment of tasks to actors, the
batch-1 `task=`, the tool's flag, the _mix entries' host checks, and, on the host models alone, that the traces of
tests/test_arcade_mix_gpu.py end episodes of every task both ways."""
import os
import subprocess
import sys

import numpy as np
import pytest

try:
    import mix_model as MM
except ImportError:            # imported as tests.<module>
    from tests import mix_model as MM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("unreal_arcade_mix_reset", "unreal_arcade_mix_step", "unreal_arcade_mix_rollout_step",
           "unreal_arcade_mix_policy_rollout_step", "unreal_arcade_mix_rollout_step_tl",
           "unreal_arcade_mix_policy_rollout_step_tl")


def _conf(**kw):
    from unreal_amd.environment.arcade_environment import ArcadeConfig
    return ArcadeConfig(**kw)


# ---- ArcadeMix ------------------------------------------------------------------------------------------------------------------
def test_a_mixture_holds_one_to_sixteen_configs():
    from unreal_amd.environment.arcade_environment import ArcadeMix
    for bad in ([], [_conf()] * 17, [_conf(), "breakout"], [_conf(), dict(game="duel")], [None]):
        with pytest.raises(ValueError):
            ArcadeMix(bad)
    for K in (1, 16):
        mix = ArcadeMix([_conf()] * K)
        assert len(mix) == K == len(mix.tasks) == len(mix.task_names)
    mix = MM.make_mix(MM.MIX3)
    assert mix.game == "mix" and mix.action_size == 4
    assert [t.game for t in mix.tasks] == ["breakout", "duel", "invaders"]
    assert mix.task_names == ("0:breakout", "1:duel", "2:invaders")


def test_the_block_is_the_tasks_blocks_in_order():
    mix = MM.make_mix(MM.MIX16)
    seed = 0xFEDCBA9876543210
    block = mix.block(seed)
    assert block.dtype == np.int32 and block.shape == (16 * 24,)
    for k, t in enumerate(mix.tasks):
        np.testing.assert_array_equal(block[24 * k:24 * k + 24], t.block(seed))
    assert sorted(set(block[::24].tolist())) == [1, 3, 5]                   # every game
    assert block[1::24].tolist() == [s["action_repeat"] - 1 for s in MM.MIX16]
    assert block[3::24].tolist() == [s["max_episode_steps"] for s in MM.MIX16]


def test_task_of_is_the_global_actor_modulo_the_tasks():
    mix = MM.make_mix(MM.MIX3)
    assert [mix.task_of(g) for g in range(7)] == [0, 1, 2, 0, 1, 2, 0]
    np.testing.assert_array_equal(mix.task_of(np.arange(5) + 4), [1, 2, 0, 1, 2])
    assert mix.task_of(3 * 4096 + 2) == 2
    with pytest.raises(ValueError):
        mix.task_of(-1)
    hosts = MM.host_batch(mix, 5, seed=3, actor_base=4, frames=False)
    assert [h.g for h in hosts] == [4, 5, 6, 7, 8]
    assert [h.c is mix.tasks[k] for h, k in zip(hosts, (1, 2, 0, 1, 2))] == [True] * 5
    assert [type(h) is MM.model_class(h.c) for h in hosts] == [True] * 5


def test_register_arcade_mix_takes_names_and_dicts():
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.arcade_environment import ArcadeMix
    names = ("mixcpu_b", "mixcpu_d", "mixcpu", "mixcpu_bad")
    try:
        Environment.register_arcade_config("mixcpu_b", rows=2)
        Environment.register_arcade_config("mixcpu_d", game="duel", points=3)
        Environment.register_arcade_mix("mixcpu", ["mixcpu_b", dict(game="invaders", alien_rows=2), "mixcpu_d", "mixcpu_b"])
        mix = Environment.arcade_config("mixcpu")
        assert isinstance(mix, ArcadeMix) and len(mix) == 4
        assert mix.tasks[0] is Environment.ARCADE_CONFIG["mixcpu_b"] and mix.tasks[3] is mix.tasks[0]
        assert mix.tasks[1].game == "invaders" and mix.tasks[1].alien_rows == 2 and mix.tasks[2].points == 3
        assert mix.task_names == ("mixcpu_b", "1:invaders", "mixcpu_d", "mixcpu_b")
        assert Environment.get_action_size("arcade", "mixcpu") == 4
        with pytest.raises(KeyError):
            Environment.register_arcade_mix("mixcpu_bad", ["mixcpu_b", "mixcpu_unknown"])
        for bad in ([], ["mixcpu_b"] * 17, ["mixcpu_b", 3], ["mixcpu"], "mixcpu_b", [dict(game="pong")],
                    [dict(game="duel", rows=2)]):
            with pytest.raises(ValueError):
                Environment.register_arcade_mix("mixcpu_bad", bad)
        assert "mixcpu_bad" not in Environment.ARCADE_CONFIG
    finally:
        for n in names:
            Environment.ARCADE_CONFIG.pop(n, None)


def test_the_trainer_options_accept_a_mixture():
    """The option checks see env_type 'arcade', whatever the name holds: a mixture takes what a single game takes."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.train.trainer import Trainer
    try:
        Environment.register_arcade_mix("mixcpu_opts", [dict(s) for s in MM.MIX3])
        assert Trainer.check_rollout_options("arcade", "mixcpu_opts", True, 0.95) == (True, 0.95)
        assert Trainer.check_reuse_options("arcade", 2, 0.2) == (2, 0.2)
        assert Trainer.check_minibatch_options("arcade", 8, 2, 2) == 2
        assert Trainer.check_explore_options("arcade", 0.1)[0] == 0.1
        with pytest.raises(ValueError):
            Trainer.check_depth_prediction("arcade", "mixcpu_opts", True)
    finally:
        Environment.ARCADE_CONFIG.pop("mixcpu_opts", None)


def test_the_batch1_task_is_bounded():
    """Refused before any device memory is asked for."""
    from unreal_amd.environment.arcade_environment import ArcadeEnvironment
    mix = MM.make_mix(MM.MIX3)
    for task in (-1, 3, 1.0, True, None):
        with pytest.raises(ValueError, match="task"):
            ArcadeEnvironment(config=mix, task=task)
    with pytest.raises(ValueError, match="task"):
        ArcadeEnvironment(config=mix.tasks[0], task=1)          # a single game has task 0 only


def test_the_ring_keeps_statistics_only_when_asked():
    from unreal_amd import ops
    import torch
    cpu = torch.device("cpu")                                    # (allocation only: no kernel is involved)
    plain = ops.Ring(4, 2, cpu, arcade=True)
    assert plain.done_return is None and plain.done_episodes is None
    ring = ops.Ring(4, 2, cpu, arcade=True, arcade_stats=True)
    assert ring.done_return.dtype == torch.float32 and ring.done_episodes.dtype == torch.int32
    assert ring.done_return.shape == ring.done_episodes.shape == (4,)
    v = ops.ring_view(ring, 1, 3)
    assert v.done_return.data_ptr() == ring.done_return[1:].data_ptr() and v.done_return.numel() == 2
    assert v.done_episodes.data_ptr() == ring.done_episodes[1:].data_ptr() and v.done_episodes.numel() == 2
    pv = ops.ring_view(plain, 1, 3)
    assert pv.done_return is None and pv.done_episodes is None
    with pytest.raises(ValueError):
        ops.Ring(4, 2, cpu, arcade_stats=True)


def test_the_tool_parses_the_mixture():
    src = open(os.path.join(ROOT, "tools", "train_maze.py")).read()
    assert '"--arcade-mix"' in src and "task_scores()" in src
    tool = os.path.join(ROOT, "tools", "train_maze.py")
    for argv, word in ((["--arcade-mix", "breakout,pong"], "comma list"),
                       (["--arcade-mix", "breakout,duel", "--arcade", "duel"], "three environments"),
                       (["--arcade-mix", ",".join(["duel"] * 17)], "comma list")):
        r = subprocess.run([sys.executable, tool] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 2 and word in r.stderr.decode(), (argv, r.returncode, r.stderr.decode()[-300:])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_and_documented():
    from unreal_amd import _lib, ops
    import re
    protos = _lib.parse_header()
    src = open(os.path.join(ROOT, "include", "unreal_hip.h")).read()
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        plain = protos[name.replace("_mix", "")]
        extra = 1 if name.endswith("reset") else 3                 # n_blocks; and the two statistics arrays
        assert name in protos and len(protos[name]) == len(plain) + extra, name
        assert name in text, name
    defs = dict(re.findall(r"#define (UNREAL_ARCADE_\w+) (\w+)", src))
    assert int(defs["UNREAL_ARCADE_MIX_MAX"]) == ops.ARCADE_MIX_MAX == 16


def test_entries_refuse_bad_arguments_without_a_launch():
    """Fake device pointers: every call below is refused by the host check, so none reaches a kernel."""
    from unreal_amd.build import build_library
    from unreal_amd import _lib
    build_library(verbose=False)
    f = _lib.lib()._fn
    EINVAL = -22
    dev = 1 << 20
    ring = [None] + [dev] * 10 + [None, None] + [dev] * 3    # pos .. score_valid
    heads = {"unreal_arcade_mix_reset": [4, 3, None, None, dev, dev, dev, dev],
             "unreal_arcade_mix_step": [4, 3, dev, None] + ring + [1, 1],
             "unreal_arcade_mix_rollout_step": [4, 3, dev] + ring + [dev] * 4 + [None, None, 0, 0, 4, 0],
             "unreal_arcade_mix_policy_rollout_step": [4, 3, dev, 256] + [dev] * 8 + ring + [dev] * 4 + [None, None, 0, 0, 4, 0]}
    heads["unreal_arcade_mix_rollout_step_tl"] = heads["unreal_arcade_mix_rollout_step"]
    heads["unreal_arcade_mix_policy_rollout_step_tl"] = heads["unreal_arcade_mix_policy_rollout_step"]

    def call(name, n_blocks=3, stats=(dev, dev), tail=None, head=None):
        tail = [dev, n_blocks, 0, dev, dev, dev] if tail is None else tail       # cfg, n_blocks, actor_base, ep_steps ..
        fin = [dev] if name.endswith("_tl") else []
        st = [] if name.endswith("reset") else list(stats)
        return f[name](*(heads[name] if head is None else head), *tail, *fin, *st, None)

    for name in ENTRIES:
        for K in (0, 17, -1, 1 << 20):
            assert call(name, n_blocks=K) == EINVAL, (name, K)
        if not name.endswith("reset"):
            assert call(name, stats=(dev, None)) == EINVAL, name           # one statistics array without the other
            assert call(name, stats=(None, dev)) == EINVAL, name
        # what the plain entries refuse: a null or misaligned block, actor_base < 0, no ep_steps / episode / records, B, H1
        for tail in ([None, 3, 0, dev, dev, dev], [dev + 2, 3, 0, dev, dev, dev], [dev, 3, -1, dev, dev, dev],
                     [dev, 3, 0, None, dev, dev], [dev, 3, 0, dev, None, dev], [dev, 3, 0, dev, dev, None]):
            assert call(name, tail=tail) == EINVAL, (name, tail)
        assert call(name, head=[0] + heads[name][1:]) == EINVAL, name
        assert call(name, head=[4, 1] + heads[name][2:]) == EINVAL, name
    for name in ENTRIES[2:]:                                               # A != 4 in the rollout forms
        assert call(name, head=heads[name][:-2] + [6, 0]) == EINVAL, name
    for name in ENTRIES[4:]:                                               # the _tl forms: a null or misaligned store
        for store in (None, dev + 8):
            assert f[name](*heads[name], dev, 3, 0, dev, dev, dev, store, dev, dev, None) == EINVAL, (name, store)


def test_the_wrappers_check_the_mixture_before_a_launch():
    from unreal_amd import ops
    import torch

    class FakeCuda(object):                                       # what _chk reads of a tensor
        is_cuda, dtype = True, torch.int32

        def __init__(self, n):
            self.n = n

        def is_contiguous(self):
            return True

        def numel(self):
            return self.n

    ring = ops.Ring(4, 2, torch.device("cpu"), arcade=True)
    for K in (0, 17):
        with pytest.raises(ValueError, match="1..16"):
            ops._arcade_args(ring, (FakeCuda(24 * 17), 0, K))
    with pytest.raises(ValueError, match="arcade config"):      # K blocks are K * 24 words
        ops._arcade_args(ring, (FakeCuda(24 * 2), 0, 3))


# ---- the traces of the GPU test, on the models alone --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(MM.TRACE_CASES)))
def test_every_task_of_a_trace_ends_by_the_game_and_by_its_step_limit(case):
    tr = MM.run_trace(case)
    settings, B = MM.TRACE_CASES[case]
    K = len(settings)
    missing = MM.every_ending(case) - tr["endings"]
    assert not missing, sorted(missing)
    # the limits at work are the tasks' own: an actor's ep_steps never passes its task's limit, and reaches it
    limit = np.array([settings[b % K]["max_episode_steps"] for b in range(B)])
    stepped = tr["terminal"] != -7
    cut = np.zeros(B, bool)
    steps = np.zeros(B, np.int64)
    for s in range(MM.TRACE_STEPS):
        steps += stepped[s]
        assert (steps <= limit).all()
        cut |= stepped[s] & (steps == limit)
        steps[stepped[s] & (tr["terminal"][s] == 1)] = 0
    assert all(cut[np.arange(B) % K == k].any() for k in range(K))
    assert len(set(limit.tolist())) == min(K, len({s["max_episode_steps"] for s in settings}))
    # the statistics are not trivial: every task finishes episodes, and some return is not zero
    done = tr["done_episodes"]
    assert all(done[np.arange(B) % K == k].sum() >= 2 for k in range(K))
    assert np.abs(tr["done_return"]).sum() > 0 and int(done.sum()) == int((tr["terminal"] == 1).sum())
    # frames are compared where the issue asks: of every actor up to 19, of the first 8 of 64
    assert tr["frames"].shape[1] == (B if B <= 19 else 8)
