"""The device arcade's crossing game (csrc/arcade.hip) bit for bit against the host model of
tests/crossing_model.py: resets, four random traces, one at four ticks per agent step and two scripted ones (computed once
on the model, crossing_model.run_trace, and shared with tests/test_crossing_cpu.py, which asserts the events they hold), the
fused rollout entries against the two-launch path on views, the _tl entries, a four-game mixture, one environment of each
of the four games stepped in turn, a crossing block in the self-play and versus entries, Trainer.process against
OracleTrainer, Evaluate and the batch-1 environment."""
import numpy as np
import pytest
import torch

try:
    import arcade_model as AM
    import crossing_model as CM
    import duel_model as DM
    import invaders_model as IM
    import mix_model as MM
    import test_arcade_gpu as TA
    import test_duel_gpu as TD
    import test_invaders_gpu as TI
    from test_trainer_gpu import _cfg, _build
    from test_fp_maze_gpu import _current_frames, _rollout_state
except ImportError:            # imported as tests.<module>
    from tests import arcade_model as AM
    from tests import crossing_model as CM
    from tests import duel_model as DM
    from tests import invaders_model as IM
    from tests import mix_model as MM
    from tests import test_arcade_gpu as TA
    from tests import test_duel_gpu as TD
    from tests import test_invaders_gpu as TI
    from tests.test_trainer_gpu import _cfg, _build
    from tests.test_fp_maze_gpu import _current_frames, _rollout_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB, PC = 21168, 400
_conf, _env, _check_state, _register = TA._conf, TD._env, TA._check_state, TA._register
# short episodes with rewards of both signs: a wide walker under four fast one-car lanes, four ticks a step (a crossing is
# five forward steps), two crossings end the game, a step limit
SHORT = dict(game="crossing", paddle_width=24, knock_back=8, crossings=2, ball_speed=4, serve_wait=1, lanes=CM.FAST_LANES,
             cross_reward=7, hit_reward=-1, action_repeat=4, max_episode_steps=30)


def _hosts(conf, B, seed, actor_base=0, n_frames=None):
    """Host models of an environment built by _env (episode 0: the model's constructor resets once, too)."""
    return [CM.HostCrossing(conf, actor_base + b, seed, frames=n_frames is None or b < n_frames) for b in range(B)]


# ---- 1. resets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 64])
@pytest.mark.parametrize("kw", [dict(paddle_width=4), dict(lanes=[(1, 0, 1, 1)], car_length=4),
                                dict(paddle_width=24, lanes=[(4, 4, 1, 1 - 2 * (l % 2)) for l in range(8)], car_length=16)])
def test_reset_matches_the_host_model(B, kw):
    conf = _conf(game="crossing", **kw)
    env = _env(B, 3, conf, seed=7)
    models = _hosts(conf, B, 7)
    _check_state(env, models, "reset", count=np.zeros(B, np.int32))
    rec = env.current_records()
    assert len(set(map(tuple, rec[:, 5:7]))) == B            # every actor has lane phases of its own
    assert (rec[:, [0, 1, 2, 3, 4]] == [42 - conf.paddle_width // 2, 76, 0, 0, 0]).all() and not rec[:, 7:].any()
    frame = _current_frames(env.ring)[0].reshape(84, 84, 3)
    count = lambda colour: int((frame == colour).all(2).sum())
    assert (count(AM.WHITE), count(AM.BORDER), count(AM.PADDLE)) == (0, 816, 4 * conf.paddle_width)


def test_masked_reset_over_sentinel_slots():
    B = 64
    conf = _conf(game="crossing", paddle_width=4, serve_wait=3)
    env = _env(B, 3, conf, seed=2)
    models = _hosts(conf, B, 2)
    acts = torch.from_numpy(np.random.RandomState(0).randint(1, 4, B).astype(np.int32)).to(DEV)
    for _ in range(12):                                # walk a little: the records are no reset records
        env.process(acts, None, None, None)
        for m, a in zip(models, acts.cpu().numpy()):
            m.process(a)
    before = env.current_records()
    assert (before[:, 4] == 0).all() and ((before[:, 0] != 40) | (before[:, 1] != 76)).any()      # (12 ticks: the counter wrapped)
    env.ring.frames.fill_(0xAB)
    mask = (np.random.RandomState(1).rand(B) < 0.5).astype(np.int32)
    mask[0], mask[1] = 1, 0
    env.reset(torch.from_numpy(mask).to(DEV))
    for m, k in zip(models, mask):
        if k:
            m.reset()
    rec, frames = env.current_records(), _current_frames(env.ring)
    for b, m in enumerate(models):
        np.testing.assert_array_equal(rec[b], m.record())
        if mask[b]:
            np.testing.assert_array_equal(frames[b], m.frame.reshape(-1))
            assert (rec[b, 5:7] != before[b, 5:7]).any()                 # the new episode's draw
        else:
            assert (frames[b] == 0xAB).all() and (rec[b] == before[b]).all()
    np.testing.assert_array_equal(env.ring.episode.cpu().numpy(), [m.episode for m in models])
    np.testing.assert_array_equal(env.ring.ep_steps.cpu().numpy(), [m.ep_steps for m in models])
    idx = env.ring.cur_idx().long().cpu().numpy()      # every slot but the actors' current ones is untouched
    others = np.ones(B * env.ring.H1, bool)
    others[idx] = False
    assert (env.ring.frames.view(-1, FB).cpu().numpy()[others] == 0xAB).all()


# ---- 2. traces -----------------------------------------------------------------------------------------------------------------
def _run_trace(k):
    """Step a device environment through trace k and compare, after every agent step, every reward, terminal, record, count,
    ep_steps, episode, last action and reward, and for the trace's watched actors the frame and the pixel change."""
    conf, tr = CM.trace_config(k), CM.run_trace(k)
    S, B = tr["acts"].shape
    F = tr["pc"].shape[1]
    env = _env(B, 3, conf, seed=CM.TRACE_SEED)             # zeroed ring memory, episode 0: H1 = 4 as run_trace's slots
    ring = env.ring
    assert env.arcade[0][0].item() == 7 and env.arcade[0][1].item() == conf.action_repeat - 1
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
            assert (frames[b] == CM.frame_of(conf, tr["records"][s, b]).reshape(-1)).all(), "%s: frame of actor %d" % (what, b)
            if tr["pc_slot"][s, b] >= 0:
                np.testing.assert_array_equal(r_pc[int(tr["pc_slot"][s, b])].cpu().numpy(), tr["pc"][s, b],
                                              err_msg="%s actor %d" % (what, b))
    return tr["events"]


@pytest.mark.parametrize("k", range(4))
def test_random_steps_match_the_host_model(k):
    """300 random steps of 200 actors under an `active` mask in the four settings; tests/test_crossing_cpu.py checks on the
    model alone that the traces hold CM.TRACE_EVENTS."""
    assert _run_trace(k) & CM.TRACE_EVENTS


def test_random_steps_at_four_ticks_match_the_host_model():
    """The short setting at action_repeat = 4: steps cut short by the tick that reaches the target, rewards summed."""
    assert CM.REPEAT_EVENTS <= _run_trace(4)


def test_scripted_steps_hit_at_either_edge_of_the_walker():
    """What random play does not reach for certain: hits on the walker's first and last column and misses by one pixel at a
    parked lane, the walker stunned under moving cars, the clamps.  Frames and pixel change of every actor."""
    assert CM.SCRIPTED_EVENTS <= _run_trace(5)


def test_scripted_steps_run_past_the_score_row():
    """21 crossings in one episode: the score row stops at 19 blocks, the target ends the game."""
    assert CM.RUNNER_EVENTS <= _run_trace(6)


# ---- 3. fused entries, views, time limits, other games -----------------------------------------------------------------------
@pytest.mark.parametrize("B", [64, 300])
def test_fused_rollout_steps_are_the_two_launch_paths(B, monkeypatch):
    """tests/test_duel_gpu.py's comparison on a crossing config: on two views of each environment (view and actor_base),
    rollout_step == process + rollout_advance and policy_rollout_step == policy_step + rollout_step, bit for bit; it
    asserts terminals and the rewards 0, -1 and 7."""
    monkeypatch.setattr(TD, "SHORT", SHORT)
    TD.test_fused_rollout_steps_are_the_two_launch_paths(B)


def test_views_and_actor_base_step_the_same_actors(monkeypatch):
    """Eight actors as one environment, as two views of one and as two environments with actor_base 0 and 4, then against
    the model (the reset draws are keyed by the global actor)."""
    monkeypatch.setattr(TD, "SHORT", SHORT)
    monkeypatch.setattr(TD, "_hosts", _hosts)
    TD.test_views_and_actor_base_step_the_same_actors()


@pytest.mark.parametrize("mix", [False, True])
def test_tl_entries_flag_the_limit_2_and_the_target_1(mix):
    """The _tl rollout entries, of a single game and of a one-task mixture: the limit of 18 steps is the step in
    which a walker that only walks forward makes the one crossing asked for.  Even actors walk: the target is reached AT
    the limit and flagged 1, nothing is kept; odd ones stand: cut by the limit alone, flagged 2, and their final
    observation is kept."""
    from unreal_amd.environment.arcade_environment import ArcadeMix, BatchedArcadeEnvironment
    B, H, xld, SENTINEL = 6, 3, 264, 0xAB
    conf = _conf(game="crossing", paddle_width=4, ball_speed=4, crossings=1, lanes=[(1, 0, 1, 1)], car_length=4,
                 cross_reward=7, max_episode_steps=18)
    env = BatchedArcadeEnvironment(B, H, DEV, config=ArcadeMix([conf]) if mix else conf, seed=3, final_obs=True)
    env.ring.frames.zero_()
    env.ring.final_obs.fill_(SENTINEL)
    env.ring.episode.fill_(-1)
    env.reset()
    hosts = _hosts(conf, B, 3)
    st = _rollout_state(B, xld)
    acts = np.array([1, 0] * (B // 2), np.int32)
    st["a"].copy_(torch.from_numpy(acts))
    for step in range(18):
        st["active"].fill_(1); st["te"].zero_(); st["n"].zero_()
        env.rollout_step(st["a"], st["r"], st["t"], st["active"], st["log"], st["n"], st["te"], next_idx=st["idx"],
                         next_lar=st["lar"], lar_ld=xld, lar_col0=256, A=4)
        out = [h.process(a) for h, a in zip(hosts, acts)]
        flags = [0 if not o[2] else 1 if h.success else 2 for o, h in zip(out, hosts)]
        np.testing.assert_array_equal(st["t"].cpu().numpy(), flags, err_msg=str(step))
        np.testing.assert_array_equal(st["te"].cpu().numpy(), flags, err_msg=str(step))
        np.testing.assert_array_equal(st["r"].cpu().numpy(), [o[1] for o in out], err_msg=str(step))
    assert flags == [1, 2] * (B // 2) and [o[1] for o in out] == [7, 0] * (B // 2)
    final = env.ring.final_obs.view(B, FB).cpu().numpy()
    for b, h in enumerate(hosts):
        if flags[b] == 2:
            np.testing.assert_array_equal(final[b], h.frame.reshape(-1))
        else:
            assert (final[b] == SENTINEL).all()
        h.reset()
    _check_state(env, hosts, "after the limit")
    assert (env.current_records()[:, 12] == [1, 0] * (B // 2)).all()


def _four_games():
    confs = [_conf(**TA.SHORT), _conf(**TD.SHORT), _conf(**TI.SHORT), _conf(**SHORT)]
    classes = [MM.model_class(c) for c in confs[:3]] + [CM.HostCrossing]
    return confs, classes


def test_a_four_game_mixture_matches_one_model_per_actor():
    """Actor b plays game b % 4 by its own rules: 80 random steps of 19 actors under an `active` mask."""
    from unreal_amd.environment.arcade_environment import ArcadeMix
    B, seed = 19, 6
    confs, classes = _four_games()
    env = _env(B, 3, ArcadeMix(confs), seed=seed)
    assert [env.arcade[0][24 * k].item() for k in range(4)] == [1, 3, 5, 7] and env.arcade[2] == 4
    models = [classes[b % 4](confs[b % 4], b, seed) for b in range(B)]
    rs = np.random.RandomState(8)
    out_r = torch.zeros(B, dtype=torch.float32, device=DEV)
    out_t = torch.zeros(B, dtype=torch.int32, device=DEV)
    ends = [0] * 4
    for step in range(80):
        acts, active = rs.randint(0, 4, B).astype(np.int32), (rs.rand(B) < 0.9).astype(np.int32)
        out_r.fill_(-7.5); out_t.fill_(-7)
        env.process(torch.from_numpy(acts).to(DEV), torch.from_numpy(active).to(DEV), out_r, out_t, track_score=True)
        want_r, want_t = np.full(B, -7.5, np.float32), np.full(B, -7, np.int32)
        for b, m in enumerate(models):
            if active[b]:
                _, r, t, _ = m.process(acts[b])
                want_r[b], want_t[b] = r, int(t)
                if t:
                    ends[b % 4] += 1
                    m.reset()
        np.testing.assert_array_equal(out_r.cpu().numpy(), want_r, err_msg=str(step))
        np.testing.assert_array_equal(out_t.cpu().numpy(), want_t, err_msg=str(step))
        _check_state(env, models, "step %d" % step)
    assert min(ends) > 0
    assert int(env.ring.done_episodes.sum()) == sum(ends)


def test_one_environment_of_each_game_stepped_in_turn():
    """The kernels branch on the block's game id: the four games in one process, stepped alternately with the same
    actions; all stay equal to their models, so nothing leaks across the branches."""
    B, H, seed = 16, 3, 4
    confs, classes = _four_games()
    envs = [_env(B, H, c, seed=seed) for c in confs]
    models = [[cls(c, b, seed) for b in range(B)] for c, cls in zip(confs, classes)]
    assert [e.arcade[0][0].item() for e in envs] == [1, 3, 5, 7]
    rs = np.random.RandomState(6)
    ends = [0, 0, 0, 0]
    for step in range(60):
        acts = rs.randint(0, 4, B).astype(np.int32)
        dev_acts = torch.from_numpy(acts).to(DEV)
        for k in range(4):
            envs[k].process(dev_acts, None, None, None)
            for m, a in zip(models[k], acts):
                if m.process(a)[2]:
                    ends[k] += 1
                    m.reset()
            _check_state(envs[k], models[k], "step %d game %d" % (step, k))
    assert min(ends) > 0


@pytest.mark.parametrize("family", ["selfplay", "versus"])
def test_a_crossing_block_is_inert_in_the_two_paddle_entries(family):
    """The self-play and versus kernels have no branch for the game: with a crossing block they write nothing."""
    from unreal_amd import ops
    from unreal_amd.environment.arcade_environment import ArcadeSelfPlay, BatchedArcadeEnvironment
    B = 8
    env = BatchedArcadeEnvironment(B, 2, DEV, config=ArcadeSelfPlay(), seed=1, versus=family == "versus")
    block = torch.from_numpy(_conf(**SHORT).block(1)).to(DEV)
    assert block[0].item() == ops.ARCADE_CROSSING == 7
    arcade = (block,) + env.arcade[1:]
    ring = env.ring
    ring.frames.fill_(0x5A)
    ring.r_pc.zero_()                                  # (torch.empty: stale bytes may be NaNs, which equal nothing)
    before = {k: getattr(ring, k).clone() for k in TD.ARRAYS}
    z = lambda dt, v: torch.full((B,), v, dtype=dt, device=DEV)
    st = _rollout_state(B, 264)
    outs = dict(r=z(torch.float32, -7.5), t=z(torch.int32, -7))
    ops.arcade_reset(ring, None, arcade=arcade)
    ops.arcade_step(ring, z(torch.int32, 1), None, outs["r"], outs["t"], arcade=arcade)
    ops.arcade_rollout_step(ring, z(torch.int32, 1), outs["r"], outs["t"], st["active"], st["log"], st["n"], st["te"],
                            next_idx=st["idx"], arcade=arcade)
    torch.cuda.synchronize()
    for k, t in before.items():
        assert torch.equal(getattr(ring, k), t), k
    assert (outs["r"] == -7.5).all() and (outs["t"] == -7).all()
    assert (st["active"] == 1).all() and not st["log"].any() and not st["n"].any() and not st["idx"].any()


# ---- 4. trainer, evaluation, batch 1 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_lstm,aux", [(True, True), (False, False)])
def test_process_on_crossing_matches_oracle(use_lstm, aux, monkeypatch):
    """Trainer.process against OracleTrainer with one host model per actor (tests/test_duel_gpu.py's test on a crossing
    config, at its bars, which are those of tests/test_forage_maze_gpu.py; rewards 7 and -1)."""
    monkeypatch.setattr(TD, "SHORT", SHORT)
    monkeypatch.setattr(DM, "host_batch", CM.host_batch)
    TD.test_process_on_the_duel_matches_oracle(use_lstm, aux)


def test_grouped_process_on_crossing_is_the_reference_algorithm(monkeypatch):
    """groups = B: one process() call = B sequential single-actor passes, against OracleTrainer.process_async."""
    monkeypatch.setattr(TD, "SHORT", SHORT)
    monkeypatch.setattr(DM, "host_batch", CM.host_batch)
    TD.test_grouped_process_on_the_duel_is_the_reference_algorithm()


def test_evaluate_on_crossing_matches_the_host_model():
    """Evaluate(arcade=name): rewards / terminals of every step agree with the host model replaying the device's actions,
    and the statistics are those of the models' first episodes."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.evaluate import Evaluate
    name = "crossing_eval"
    conf = _register(name, **dict(SHORT, max_episode_steps=40))
    try:
        cfg = _cfg(True, False, 40, 20)
        net, _, _, _ = _build(cfg, 1, seed=31, env_type="arcade", env_name=name)
        B, seed = 32, 0x5EED
        ev = Evaluate(net, batch_size=B, device=DEV, seed=seed, arcade=name)
        assert not net.lar_bounded
        log = []
        inner = ev.env.process

        def recording(actions, active, out_reward, out_terminal, **kw):
            inner(actions, active, out_reward, out_terminal, **kw)
            log.append((actions.cpu().numpy().copy(), out_reward.cpu().numpy().copy(), out_terminal.cpu().numpy().copy()))
        ev.env.process = recording
        res = ev.process(0, one_episode_per_actor=True)
        hosts = CM.host_batch(conf, B, seed=seed)
        for h in hosts:
            h.reset()
        first, ret, start = [None] * B, [0] * B, [list(h.totals) for h in hosts]
        for step, (acts, rew, term) in enumerate(log):
            for b, h in enumerate(hosts):
                _, r, t, _ = h.process(acts[b])
                assert (float(r), int(t)) == (float(rew[b]), int(term[b])), (step, b)
                ret[b] += r
                if t:
                    if first[b] is None:
                        first[b] = (ret[b], h.ep_steps, h.totals[0] - start[b][0], h.totals[1] - start[b][1], h.success)
                    ret[b], start[b] = 0, list(h.totals)
                    h.reset()
        assert None not in first
        col = lambda i: np.array([f[i] for f in first], np.float64)
        assert sorted(res) == sorted(("episodes", "success_rate", "mean_return", "return_std", "mean_length", "timeouts",
                                      "crossings_per_episode", "hits_per_episode"))
        assert res["episodes"] == B and res["timeouts"] == B - int(col(4).sum())
        for key, want in (("success_rate", col(4).mean()), ("mean_return", col(0).mean()), ("return_std", col(0).std()),
                          ("mean_length", col(1).mean()), ("crossings_per_episode", col(2).mean()),
                          ("hits_per_episode", col(3).mean())):
            assert abs(res[key] - want) < 1e-9, (key, res[key], want)
        assert col(2).sum() > 0 and col(3).sum() > 0, first
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


def test_batch1_environment_also_past_a_terminal():
    """Environment.create_environment('arcade', name): 160 steps of images, rewards, terminals and pixel change of the
    host model; no reset on terminal (the caller resets), and a game that is stepped past either kind of terminal goes on:
    the count runs past the target, the step counter past the limit."""
    from unreal_amd.environment.environment import Environment
    name = "crossing_batch1"
    conf = _register(name, **dict(SHORT, paddle_width=4, crossings=1, max_episode_steps=25))
    try:
        env = Environment.create_environment("arcade", name)
        host = CM.HostCrossing(conf, 0, 0)
        host.reset()
        np.testing.assert_array_equal(env.last_state["image"], host.last_state["image"])
        rs = np.random.RandomState(2)
        n_term, past, kinds, past_kinds = 0, 0, set(), set()
        for step in range(160):
            a = int(rs.randint(0, 4)) if n_term % 2 else 1             # every other episode only walks: it reaches the target
            image, reward, terminal, pc = env.process(a)
            _, r, t, pc_h = host.process(a)
            np.testing.assert_array_equal(image, host.last_state["image"], err_msg=str(step))
            assert (reward, terminal) == (r, t), step
            np.testing.assert_array_equal(pc, pc_h, err_msg=str(step))
            assert (env.last_action, env.last_reward) == (a, r)
            if terminal:
                assert env._last_full_state["success"] == host.success
                kinds.add(host.success)
                past += 1
                if past < 8:                           # seven more steps of an ended game
                    past_kinds.add(host.success)
                    continue
                n_term += 1
                past = 0
                env.reset()
                host.reset()
                np.testing.assert_array_equal(env.last_state["image"], host.last_state["image"])
        assert n_term > 2 and kinds == {True, False} and past_kinds == {True, False}
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)
