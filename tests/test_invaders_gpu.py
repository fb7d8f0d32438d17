"""The device arcade's invaders game (csrc/arcade.hip) bit for bit against the host model of
tests/invaders_model.py: resets, three random traces, one at four ticks per agent step and a scripted one (computed once on
the model, invaders_model.run_trace, and shared with tests/test_invaders_cpu.py, which asserts the events they hold), the
fused rollout entries against the two-launch path on views, one environment of each of the three games stepped in turn,
Trainer.process against OracleTrainer, Evaluate and the batch-1 environment."""
import numpy as np
import pytest
import torch

try:
    import arcade_model as AM
    import duel_model as DM
    import invaders_model as IM
    import test_arcade_gpu as TA
    import test_duel_gpu as TD
    from test_trainer_gpu import _cfg, _build
    from test_fp_maze_gpu import _current_frames
except ImportError:            # imported as tests.<module>
    from tests import arcade_model as AM
    from tests import duel_model as DM
    from tests import invaders_model as IM
    from tests import test_arcade_gpu as TA
    from tests import test_duel_gpu as TD
    from tests.test_trainer_gpu import _cfg, _build
    from tests.test_fp_maze_gpu import _current_frames

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB, PC = 21168, 400
_conf, _env, _check_state, _register = TA._conf, TD._env, TA._check_state, TA._register
# short episodes with rewards of both signs: one row that comes down fast (an invasion after 76 ticks at the latest), two
# lives under many fast bombs, a fast shot, a step limit
SHORT = dict(game="invaders", alien_rows=1, lives=2, paddle_width=24, ball_speed=4, bomb_period=2, bomb_speed=4,
             march_period=1, descend=8, serve_wait=1, alien_rewards=(7,), life_reward=-1, max_episode_steps=30)


def _hosts(conf, B, seed, actor_base=0, n_frames=None):
    """Host models of an environment built by _env (episode 0: the model's constructor resets once, too)."""
    return [IM.HostInvaders(conf, actor_base + b, seed, frames=n_frames is None or b < n_frames) for b in range(B)]


# ---- 1. resets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 64])
@pytest.mark.parametrize("kw", [dict(), dict(alien_rows=1, lives=5, paddle_width=4), dict(alien_rows=4, lives=1, paddle_width=24)])
def test_reset_matches_the_host_model(B, kw):
    conf = _conf(game="invaders", **kw)
    env = _env(B, 3, conf, seed=7)
    models = _hosts(conf, B, 7)
    _check_state(env, models, "reset", count=np.zeros(B, np.int32))
    frame = _current_frames(env.ring)[0].reshape(84, 84, 3)
    count = lambda colour: int((frame == colour).all(2).sum())
    # row 0 of the aliens has the cannon's colour
    assert (count(AM.WHITE), count(AM.BORDER), count(AM.PADDLE), count(IM.BOMB)) == \
        (4 * conf.lives, 816 - 4 * conf.lives, 2 * conf.paddle_width + 8 * 24, 0)
    for r in range(1, conf.alien_rows):
        assert count(AM.ROW_COLOURS[r]) == 8 * 24


def test_masked_reset_over_sentinel_slots():
    B = 64
    conf = _conf(game="invaders", serve_wait=0, bomb_period=2, march_period=1)
    env = _env(B, 3, conf, seed=2)
    models = _hosts(conf, B, 2)
    acts = torch.from_numpy(np.random.RandomState(0).randint(0, 4, B).astype(np.int32)).to(DEV)
    for _ in range(12):                                # march, fire and drop a little: the records are no reset records
        env.process(acts, None, None, None)
        for m, a in zip(models, acts.cpu().numpy()):
            m.process(a)
    before = env.current_records()
    assert (before[:, 3] != 10).all() and (before[:, 13] != 0).all() and (before[:, 2] != 0).any()
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
    conf, tr = IM.trace_config(k), IM.run_trace(k)
    S, B = tr["acts"].shape
    F = tr["pc"].shape[1]
    env = _env(B, 3, conf, seed=IM.TRACE_SEED)             # zeroed ring memory, episode 0: H1 = 4 as run_trace's slots
    ring = env.ring
    assert env.arcade[0][0].item() == 5 and env.arcade[0][1].item() == conf.action_repeat - 1
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
            assert (frames[b] == IM.frame_of(conf, tr["records"][s, b]).reshape(-1)).all(), "%s: frame of actor %d" % (what, b)
            if tr["pc_slot"][s, b] >= 0:
                np.testing.assert_array_equal(r_pc[int(tr["pc_slot"][s, b])].cpu().numpy(), tr["pc"][s, b],
                                              err_msg="%s actor %d" % (what, b))
    return tr["events"]


@pytest.mark.parametrize("k", range(3))
def test_random_steps_match_the_host_model(k):
    """300 random steps of 200 actors under an `active` mask in the three settings; tests/test_invaders_cpu.py checks on the
    model alone that the traces hold IM.TRACE_EVENTS."""
    assert _run_trace(k) & IM.TRACE_EVENTS


def test_random_steps_at_four_ticks_match_the_host_model():
    """The small setting at action_repeat = 4: steps cut short by the tick that ends the game, rewards summed."""
    assert IM.REPEAT_EVENTS <= _run_trace(3)


def test_scripted_steps_clear_waves_are_invaded_and_time_out():
    """What random play does not reach in 300 steps: 12 actors that sweep and fire, stand still, or stop after the lower
    row.  Frames and pixel change of every actor."""
    assert IM.SCRIPTED_EVENTS <= _run_trace(4)


# ---- 3. fused entries, views, other games ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [64, 300])
def test_fused_rollout_steps_are_the_two_launch_paths(B, monkeypatch):
    """tests/test_duel_gpu.py's comparison on an invaders config: on two views of each environment (view and actor_base),
    rollout_step == process + rollout_advance and policy_rollout_step == policy_step + rollout_step, bit for bit; it
    asserts terminals and the rewards 0, -1 and 7."""
    monkeypatch.setattr(TD, "SHORT", SHORT)
    TD.test_fused_rollout_steps_are_the_two_launch_paths(B)


def test_views_and_actor_base_step_the_same_actors(monkeypatch):
    """Eight actors as one environment, as two views of one and as two environments with actor_base 0 and 4, then against
    the model (the bomb draws are keyed by the global actor)."""
    monkeypatch.setattr(TD, "SHORT", SHORT)
    monkeypatch.setattr(TD, "_hosts", _hosts)
    TD.test_views_and_actor_base_step_the_same_actors()


def test_one_environment_of_each_game_stepped_in_turn():
    """The kernels branch on the block's game id: the three games in one process, stepped alternately with the same
    actions; all stay equal to their models, so nothing leaks across the branches."""
    B, H, seed = 16, 3, 4
    confs = [_conf(**TA.SHORT), _conf(**TD.SHORT), _conf(**SHORT)]
    envs = [_env(B, H, c, seed=seed) for c in confs]
    models = [TD._hosts(confs[0], B, seed), TD._hosts(confs[1], B, seed), _hosts(confs[2], B, seed)]
    assert [e.arcade[0][0].item() for e in envs] == [1, 3, 5]
    rs = np.random.RandomState(6)
    ends = [0, 0, 0]
    for step in range(60):
        acts = rs.randint(0, 4, B).astype(np.int32)
        dev_acts = torch.from_numpy(acts).to(DEV)
        for k in (0, 1, 2):
            envs[k].process(dev_acts, None, None, None)
            for m, a in zip(models[k], acts):
                if m.process(a)[2]:
                    ends[k] += 1
                    m.reset()
            _check_state(envs[k], models[k], "step %d game %d" % (step, k))
    assert min(ends) > 0


# ---- 4. trainer, evaluation, batch 1 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_lstm,aux", [(True, True), (False, False)])
def test_process_on_invaders_matches_oracle(use_lstm, aux, monkeypatch):
    """Trainer.process against OracleTrainer with one host model per actor (tests/test_duel_gpu.py's test on an invaders
    config, at its bars, which are those of tests/test_forage_maze_gpu.py; rewards 7 and -1)."""
    monkeypatch.setattr(TD, "SHORT", SHORT)
    monkeypatch.setattr(DM, "host_batch", IM.host_batch)
    TD.test_process_on_the_duel_matches_oracle(use_lstm, aux)


def test_grouped_process_on_invaders_is_the_reference_algorithm(monkeypatch):
    """groups = B: one process() call = B sequential single-actor passes, against OracleTrainer.process_async."""
    monkeypatch.setattr(TD, "SHORT", SHORT)
    monkeypatch.setattr(DM, "host_batch", IM.host_batch)
    TD.test_grouped_process_on_the_duel_is_the_reference_algorithm()


def test_evaluate_on_invaders_matches_the_host_model():
    """Evaluate(arcade=name): rewards / terminals of every step agree with the host model replaying the device's actions,
    and the statistics are those of the models' first episodes."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.evaluate import Evaluate
    name = "invaders_eval"
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
        hosts = IM.host_batch(conf, B, seed=seed)
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
                                      "aliens_per_episode", "lives_lost_per_episode"))
        assert res["episodes"] == B and res["timeouts"] == B - int(col(4).sum())
        for key, want in (("success_rate", col(4).mean()), ("mean_return", col(0).mean()), ("return_std", col(0).std()),
                          ("mean_length", col(1).mean()), ("aliens_per_episode", col(2).mean()),
                          ("lives_lost_per_episode", col(3).mean())):
            assert abs(res[key] - want) < 1e-9, (key, res[key], want)
        assert col(2).sum() > 0 and col(3).sum() > 0, first
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


def test_batch1_environment_also_past_a_terminal():
    """Environment.create_environment('arcade', name): 100 steps of images, rewards, terminals and pixel change of the
    host model; no reset on terminal (the caller resets), and a game that is stepped past its terminal goes on."""
    from unreal_amd.environment.environment import Environment
    name = "invaders_batch1"
    conf = _register(name, **dict(SHORT, max_episode_steps=60))
    try:
        env = Environment.create_environment("arcade", name)
        host = IM.HostInvaders(conf, 0, 0)
        host.reset()
        np.testing.assert_array_equal(env.last_state["image"], host.last_state["image"])
        rs = np.random.RandomState(2)
        n_term, past = 0, 0
        for step in range(100):
            a = int(rs.randint(0, 4))
            image, reward, terminal, pc = env.process(a)
            _, r, t, pc_h = host.process(a)
            np.testing.assert_array_equal(image, host.last_state["image"], err_msg=str(step))
            assert (reward, terminal) == (r, t), step
            np.testing.assert_array_equal(pc, pc_h, err_msg=str(step))
            assert (env.last_action, env.last_reward) == (a, r)
            if terminal:
                assert env._last_full_state["success"] == host.success
                past += 1
                if n_term == 0 and past < 12:          # the first terminal: eleven more steps of an ended game
                    continue
                n_term += 1
                past = 0
                env.reset()
                host.reset()
                np.testing.assert_array_equal(env.last_state["image"], host.last_state["image"])
        assert n_term > 1
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)
