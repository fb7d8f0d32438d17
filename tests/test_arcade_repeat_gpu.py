"""The device arcade's action repeat and paddle-return reward (csrc/arcade.hip) bit for bit against the host
models of tests/repeat_model.py.

The traces (six random ones of 200 actors x 300 agent steps under a 0.9 `active` mask, two scripted ones of 12 actors at
k = 4) are computed once on the models (repeat_model.run_trace) and shared with tests/test_arcade_repeat_cpu.py.  The other
scenarios are those of tests/test_arcade_gpu.py and tests/test_duel_gpu.py, run again on configs with action_repeat = 4 and
return_reward = 2 and with the repeat models in place of the one-tick ones (the `repeat4` fixture): the fused entries against
the two-launch path on views, views and actor_base, Trainer.process against OracleTrainer, Evaluate, the batch-1 environment
stepped past a terminal."""
import numpy as np
import pytest
import torch

try:
    import arcade_model as AM
    import duel_model as DM
    import repeat_model as RM
    import test_arcade_gpu as TA
    import test_duel_gpu as TD
    from test_fp_maze_gpu import _current_frames
except ImportError:            # imported as tests.<module>
    from tests import arcade_model as AM
    from tests import duel_model as DM
    from tests import repeat_model as RM
    from tests import test_arcade_gpu as TA
    from tests import test_duel_gpu as TD
    from tests.test_fp_maze_gpu import _current_frames

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB, PC = 21168, 400
REPEAT4 = dict(action_repeat=4, return_reward=2)


# ---- 1. traces -----------------------------------------------------------------------------------------------------------------
def _run_trace(k):
    """Step a device environment through trace k and compare, after every agent step, every reward, terminal, record, count,
    ep_steps, episode, last action and reward, and for the trace's watched actors the frame and the pixel change."""
    conf, tr = RM.trace_config(k), RM.run_trace(k)
    S, B = tr["acts"].shape
    F = tr["pc"].shape[1]
    env = TD._env(B, 3, conf, seed=RM.TRACE_SEED)          # zeroed ring memory, episode 0: H1 = 4 as run_trace's slots
    ring = env.ring
    assert env.arcade[0][1].item() == conf.action_repeat - 1 and env.arcade[0][18].item() == conf.return_reward
    out_r = torch.zeros(B, dtype=torch.float32, device=DEV)
    out_t = torch.zeros(B, dtype=torch.int32, device=DEV)
    for s in range(S):
        what = "trace %d step %d" % (k, s)
        out_r.fill_(-7.5); out_t.fill_(-7)
        env.process(torch.from_numpy(tr["acts"][s].copy()).to(DEV), torch.from_numpy(tr["active"][s].copy()).to(DEV), out_r,
                    out_t, reset_on_terminal=True)
        np.testing.assert_array_equal(out_r.cpu().numpy(), tr["reward"][s], err_msg=what)
        np.testing.assert_array_equal(out_t.cpu().numpy(), tr["terminal"][s], err_msg=what)
        rec = env.current_records()
        bad = np.flatnonzero((rec != tr["records"][s]).any(1))
        assert not len(bad), "%s: records of actors %s differ: %s, want %s" % (what, bad[:8], rec[bad[0]],
                                                                               tr["records"][s][bad[0]])
        for name in ("count", "ep_steps", "episode", "last_action", "last_reward"):
            np.testing.assert_array_equal(getattr(ring, name).cpu().numpy(), tr[name][s], err_msg="%s %s" % (what, name))
        frames = _current_frames(ring)[:F]
        r_pc = ring.r_pc.view(-1, PC)
        for b in range(F):
            assert (frames[b] == RM.frame_of(conf, tr["records"][s, b]).reshape(-1)).all(), "%s: frame of actor %d" % (what, b)
            if tr["pc_slot"][s, b] >= 0:
                np.testing.assert_array_equal(r_pc[int(tr["pc_slot"][s, b])].cpu().numpy(), tr["pc"][s, b],
                                              err_msg="%s actor %d" % (what, b))
    return tr["events"]


@pytest.mark.parametrize("k", range(len(RM.TRACE_SETTINGS)))
def test_random_steps_match_the_host_model(k):
    """300 random agent steps of 200 actors under an `active` mask, k = 2, 4, 8 on each game."""
    assert RM.TRACE_EVENTS[k] <= _run_trace(k)


@pytest.mark.parametrize("k", [len(RM.TRACE_SETTINGS), len(RM.TRACE_SETTINGS) + 1])
def test_scripted_steps_win_and_time_out_at_four_ticks(k):
    """12 actors follow the ball at k = 4: walls cleared and matches won by skill, and time-outs; every actor's frames."""
    seen = _run_trace(k)
    assert RM.TRACE_EVENTS[k] <= seen and "end_timeout" in seen and seen & {"end_clear", "end_win"}


# ---- 2. a block with word 1 = 0 next to one with word 1 = 3, and the clamp -------------------------------------------------------
@pytest.mark.parametrize("game", ["breakout", "duel"])
def test_a_block_of_one_tick_steps_as_before_next_to_one_of_four(game):
    """Two environments in one process, stepped in turn with the same actions: the default block (words 1 and 18 zero)
    against the one-tick model of tests/arcade_model.py / tests/duel_model.py, as before these words had a meaning, and a
    k = 4 block against the repeat model.  Then word 1 out of range: the kernel clamps it to 0..7."""
    from unreal_amd import ops
    B, H, seed = 16, 3, 4
    short = dict(TD.SHORT) if game == "duel" else dict(TA.SHORT, game="breakout")
    confs = [TA._conf(**short), TA._conf(**dict(short, **REPEAT4))]
    envs = [TD._env(B, H, c, seed=seed) for c in confs]
    one_tick = DM.HostDuel if game == "duel" else AM.HostBreakout
    models = [[one_tick(confs[0], b, seed) for b in range(B)], RM.host_batch(confs[1], B, seed)]
    assert [(e.arcade[0][1].item(), e.arcade[0][18].item()) for e in envs] == [(0, 0), (3, 2)]
    rs = np.random.RandomState(6)
    ends = [0, 0]
    for step in range(60):
        acts = rs.randint(0, 4, B).astype(np.int32)
        dev_acts = torch.from_numpy(acts).to(DEV)
        for k in (0, 1):
            envs[k].process(dev_acts, None, None, None)
            for m, a in zip(models[k], acts):
                if m.process(a)[2]:
                    ends[k] += 1
                    m.reset()
            TA._check_state(envs[k], models[k], "step %d block %d" % (step, k))
    assert min(ends) > 0
    # word 1 = 100 steps as k = 8, word 1 = -5 as k = 1 (ArcadeConfig never builds such blocks)
    for word, k in ((100, 8), (-5, 1)):
        conf = TA._conf(**dict(short, action_repeat=k, return_reward=2))
        env = TD._env(B, H, conf, seed=seed)
        block = env.arcade[0].clone()
        block[1] = word
        hosts = RM.host_batch(conf, B, seed)
        for step in range(30):
            acts = rs.randint(0, 4, B).astype(np.int32)
            ops.arcade_step(env.ring, torch.from_numpy(acts).to(DEV), None, None, None, arcade=(block, 0))
            for m, a in zip(hosts, acts):
                if m.process(a)[2]:
                    m.reset()
            TA._check_state(env, hosts, "word 1 = %d step %d" % (word, step))


# ---- 3. the scenarios of the one-tick GPU tests at action_repeat = 4, return_reward = 2 ------------------------------------------
@pytest.fixture
def repeat4(monkeypatch):
    """Every config the borrowed test builds gets REPEAT4, and every host model it builds is a repeat model.  The borrowed
    files are not edited for this, so the fixture checks both ends itself: before the test that the patches took, after it
    that the test did build a k = 4 config through them.  A borrowed test that compares with host models fails on its own
    if those were one-tick models: their records leave the device's within a few steps at four ticks a step."""
    conf, register = TA._conf, TA._register
    built = []

    def repeat_conf(**kw):
        built.append(kw)
        return conf(**dict(kw, **REPEAT4))

    def repeat_register(name, **kw):
        built.append(kw)
        return register(name, **dict(kw, **REPEAT4))
    for mod in (TA, TD):
        monkeypatch.setattr(mod, "_conf", repeat_conf)
        monkeypatch.setattr(mod, "_register", repeat_register)
    monkeypatch.setattr(AM, "HostBreakout", RM.RepeatBreakout)
    monkeypatch.setattr(DM, "HostDuel", RM.RepeatDuel)
    monkeypatch.setattr(AM, "host_batch", RM.host_batch)
    monkeypatch.setattr(DM, "host_batch", RM.host_batch)
    assert TA._conf().block(0)[[1, 18]].tolist() == [3, 2] and TD._conf(game="duel").block(0)[[1, 18]].tolist() == [3, 2]
    assert type(TA._hosts(TA._conf(), 1, 0)[0]) is RM.RepeatBreakout
    assert type(TD._hosts(TD._conf(game="duel"), 1, 0)[0]) is RM.RepeatDuel
    del built[:]
    yield
    assert built, "the borrowed test built no config through the patched helpers"


@pytest.mark.parametrize("B", [64, 300])
@pytest.mark.parametrize("mod", [TA, TD], ids=["breakout", "duel"])
def test_fused_rollout_steps_are_the_two_launch_paths(repeat4, mod, B):
    """The fused entries against the two-launch path on two views of each environment (the second view's actor_base is
    its first actor), bit for bit."""
    mod.test_fused_rollout_steps_are_the_two_launch_paths(B)


@pytest.mark.parametrize("mod", [TA, TD], ids=["breakout", "duel"])
def test_views_and_actor_base_step_the_same_actors(repeat4, mod):
    mod.test_views_and_actor_base_step_the_same_actors()


def test_a_breakout_and_a_duel_environment_stepped_in_turn(repeat4):
    TD.test_a_breakout_and_a_duel_environment_stepped_in_turn()


@pytest.mark.parametrize("use_lstm,aux", [(True, True), (False, False)])
def test_process_on_breakout_matches_oracle(repeat4, use_lstm, aux):
    """Trainer.process against OracleTrainer(envs=repeat models) at the bars of tests/test_arcade_gpu.py."""
    TA.test_process_on_the_arcade_matches_oracle(use_lstm, aux)


@pytest.mark.parametrize("use_lstm,aux", [(True, True), (False, False)])
def test_process_on_the_duel_matches_oracle(repeat4, use_lstm, aux):
    TD.test_process_on_the_duel_matches_oracle(use_lstm, aux)


@pytest.mark.parametrize("mod", [TA, TD], ids=["breakout", "duel"])
def test_grouped_process_is_the_reference_algorithm(repeat4, mod):
    """groups = B against OracleTrainer.process_async."""
    (mod.test_grouped_process_on_the_arcade_is_the_reference_algorithm if mod is TA else
     mod.test_grouped_process_on_the_duel_is_the_reference_algorithm)()


@pytest.mark.parametrize("mod", [TA, TD], ids=["breakout", "duel"])
def test_evaluate_matches_the_host_model(repeat4, mod):
    """Evaluate(arcade=name) on a k = 4 config: mean_length and the step limit count agent steps, as the model's ep_steps."""
    (mod.test_evaluate_on_the_arcade_matches_the_host_model if mod is TA else
     mod.test_evaluate_on_the_duel_matches_the_host_model)()


@pytest.mark.parametrize("mod", [TA, TD], ids=["breakout", "duel"])
def test_batch1_environment_past_a_terminal(repeat4, mod):
    """The batch-1 environment has no reset on terminal: stepped past one, every step is a single tick, as on the model."""
    mod.test_batch1_environment()
