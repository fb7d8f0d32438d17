"""The device arcade (csrc/arcade.hip) bit for bit against the host model of tests/arcade_model.py: resets,
random and scripted traces with every event of the rules, the fused rollout entries against the two-launch path, views and
actor_base, a block of another game, Trainer.process against OracleTrainer, Evaluate and the batch-1 environment."""
import numpy as np
import pytest
import torch

try:
    import arcade_model as AM
    from test_trainer_gpu import _cfg, _build, _feed_draws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL
    from test_maze_config_gpu import RING_ARRAYS
    from test_fp_maze_gpu import _current_frames, _rollout_state
except ImportError:            # imported as tests.<module>
    from tests import arcade_model as AM
    from tests.test_trainer_gpu import _cfg, _build, _feed_draws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL
    from tests.test_maze_config_gpu import RING_ARRAYS
    from tests.test_fp_maze_gpu import _current_frames, _rollout_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB, PC = 21168, 400
ARRAYS = RING_ARRAYS + ("ep_steps", "episode", "arcade")
# short episodes with every kind of reward: one life, a fast ball that serves itself, a step limit
SHORT = dict(rows=2, row_rewards=(7, 1), lives=1, paddle_width=24, ball_speed=4, serve_wait=1, life_reward=-1,
             max_episode_steps=30)


def _conf(**kw):
    from unreal_amd.environment.arcade_environment import ArcadeConfig
    return ArcadeConfig(**kw)


def _env(B, H, conf, seed=0, **kw):
    from unreal_amd.environment.arcade_environment import BatchedArcadeEnvironment
    env = BatchedArcadeEnvironment(B, H, DEV, config=conf, seed=seed, **kw)
    assert env.frame_scale == 1.0 / 255.0 and env.objective_size == 0
    env.ring.frames.zero_()           # (torch.empty: slots no step has written would hold stale allocator bytes)
    env.ring.r_pc.zero_()
    env.reset()
    return env


def _hosts(conf, B, seed, actor_base=0, n_frames=None):
    """Host models of an environment built by _env: its constructor and _env each reset once (episode 1)."""
    models = [AM.HostBreakout(conf, actor_base + b, seed, frames=n_frames is None or b < n_frames) for b in range(B)]
    for m in models:
        m.reset()
    return models


def _check_state(env, models, what, count=None):
    ring = env.ring
    if count is not None:
        np.testing.assert_array_equal(ring.count.cpu().numpy(), count, err_msg=what)
    rec = env.current_records()
    want = np.stack([m.record() for m in models])
    bad = np.flatnonzero((rec != want).any(1))
    assert not len(bad), "%s: records of actors %s differ: %s, want %s" % (what, bad[:8], rec[bad[0]], want[bad[0]])
    np.testing.assert_array_equal(ring.ep_steps.cpu().numpy(), [m.ep_steps for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.episode.cpu().numpy(), [m.episode for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.last_action.cpu().numpy(), [m.last_action for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.last_reward.cpu().numpy(), np.array([m.last_reward for m in models], np.float32),
                                  err_msg=what)
    seeing = [b for b, m in enumerate(models) if m.frames]
    got = _current_frames(ring)[seeing]
    want = np.stack([models[b].frame.reshape(-1) for b in seeing])
    bad = np.flatnonzero((got != want).any(1))
    assert not len(bad), "%s: frames of actors %s differ" % (what, [seeing[i] for i in bad[:8]])


# ---- 1. resets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 64])
@pytest.mark.parametrize("kw", [dict(), dict(rows=1, lives=5, paddle_width=4), dict(rows=3, lives=1, paddle_width=24)])
def test_reset_matches_the_host_model(B, kw):
    conf = _conf(**kw)
    env = _env(B, 3, conf, seed=7)
    models = _hosts(conf, B, 7)
    _check_state(env, models, "reset", count=np.zeros(B, np.int32))
    frame = _current_frames(env.ring)[0].reshape(84, 84, 3)
    assert int((frame == AM.WHITE).all(2).sum()) == 4 * conf.lives and int((frame == AM.BORDER).all(2).sum()) == 816 - 4 * conf.lives


def test_masked_reset_over_sentinel_slots():
    B = 64
    conf = _conf(rows=4)
    env = _env(B, 3, conf, seed=2)
    models = _hosts(conf, B, 2)
    acts = torch.from_numpy(np.random.RandomState(0).randint(0, 4, B).astype(np.int32)).to(DEV)
    for _ in range(12):                                # serve and fly a little: the records are no reset records
        env.process(acts, None, None, None)
        for m, a in zip(models, acts.cpu().numpy()):
            m.process(a)
    before = env.current_records()
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
    # every slot but the actors' current ones is untouched
    idx = env.ring.cur_idx().long().cpu().numpy()
    others = np.ones(B * env.ring.H1, bool)
    others[idx] = False
    assert (env.ring.frames.view(-1, FB).cpu().numpy()[others] == 0xAB).all()


# ---- 2. traces -----------------------------------------------------------------------------------------------------------------
def _run_trace(conf, B, steps, choose, n_frames, seed=AM.TRACE_SEED):
    """Step the device and the models together; compare every record, reward, terminal, count, ep_steps and episode at
    every step, and frames and pixel change of the first n_frames actors.  choose(step, models) -> (actions, active).
    -> the events seen."""
    H = 3
    env = _env(B, H, conf, seed=seed)
    ring, H1 = env.ring, H + 1
    models = _hosts(conf, B, seed, n_frames=n_frames)
    out_r = torch.zeros(B, dtype=torch.float32, device=DEV)
    out_t = torch.zeros(B, dtype=torch.int32, device=DEV)
    count, prev_term = np.zeros(B, np.int64), np.zeros(B, bool)
    seen = set()
    for s in range(steps):
        acts, active = choose(s, models)
        out_r.fill_(-7.5); out_t.fill_(-7)
        env.process(torch.from_numpy(acts).to(DEV), torch.from_numpy(active).to(DEV), out_r, out_t, reset_on_terminal=True)
        want_r, want_t = np.full(B, -7.5, np.float32), np.full(B, -7, np.int32)
        pcs = {}
        for b, m in enumerate(models):
            if not active[b]:
                continue
            _, r, t, pc = m.process(acts[b])
            seen |= m.events
            want_r[b], want_t[b] = r, int(t)
            if b < n_frames:
                pcs[b] = (b * H1 + count[b] % H1, pc)
            if not (t and count[b] > 0 and prev_term[b]):
                count[b] += 1
            prev_term[b] = t
            if t:
                m.reset()
        what = "step %d" % s
        np.testing.assert_array_equal(out_r.cpu().numpy(), want_r, err_msg=what)
        np.testing.assert_array_equal(out_t.cpu().numpy(), want_t, err_msg=what)
        _check_state(env, models, what, count=count)
        r_pc = ring.r_pc.view(-1, PC)
        for b, (slot, pc) in pcs.items():
            np.testing.assert_array_equal(r_pc[slot].cpu().numpy(), pc.reshape(-1), err_msg="%s actor %d" % (what, b))
    return seen


@pytest.mark.parametrize("k", range(len(AM.TRACE_SETTINGS)))
def test_random_steps_match_the_host_model(k):
    """300 random steps of 200 actors under an `active` mask; tests/test_arcade_cpu.py checks on the model alone that
    the trace holds these events."""
    acts, active = AM.trace_inputs(k)
    seen = _run_trace(_conf(**AM.TRACE_SETTINGS[k]), AM.TRACE_B, AM.TRACE_STEPS, lambda s, models: (acts[s], active[s]),
                      AM.TRACE_FRAMES)
    assert AM.TRACE_EVENTS[k] <= seen, AM.TRACE_EVENTS[k] - seen


def test_scripted_steps_clear_the_wall_and_time_out():
    """The two endings no random trace reaches: a policy that follows the ball clears one row; a looping ball runs into
    max_episode_steps.  Frames and pixel change of every actor."""
    B = AM.SCRIPTED_B

    def choose(s, models):
        return np.array([AM.follow_ball(m) for m in models], np.int32), np.ones(B, np.int32)
    seen = _run_trace(_conf(**AM.SCRIPTED_SETTING), B, AM.SCRIPTED_STEPS, choose, B)
    assert AM.SCRIPTED_EVENTS <= seen, AM.SCRIPTED_EVENTS - seen


# ---- 3. fused entries, views, actor_base, other games ------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [64, 300])
def test_fused_rollout_steps_are_the_two_launch_paths(B):
    """On two views of each environment (index_parent): rollout_step == process + rollout_advance (+ cur_idx and the
    LSTM-input columns), and policy_rollout_step == policy_step + rollout_step, bit for bit: actions, pi, V, ring, records
    and the next step's rows."""
    from unreal_amd import ops
    H, A, xld = 4, 4, 264
    rs = np.random.RandomState(B)
    dev = lambda a, dt: torch.from_numpy(np.asarray(a)).to(DEV, dt)
    Wp = dev(rs.uniform(-.3, .3, 256 * A), torch.float32); bp = dev(rs.uniform(-.1, .1, A), torch.float32)
    Wv = dev(rs.uniform(-.3, .3, 256), torch.float32); bv = dev(rs.uniform(-.1, .1, 1), torch.float32)
    conf = _conf(**SHORT)
    envs = [_env(B, H, conf, seed=9) for _ in range(3)]
    cut = B // 3
    views = [[e.view(0, cut), e.view(cut, B)] for e in envs]
    st = [_rollout_state(B, xld) for _ in envs]
    n_term, n_rew = 0, set()
    for step in range(40):
        X = dev(rs.uniform(-1, 1, (B, 256)), torch.float32).view(-1)
        u = dev(rs.uniform(0, 1, B), torch.float64)
        for k, (e, s) in enumerate(zip(envs, st)):
            for v, (b0, b1) in zip(views[k], ((0, cut), (cut, B))):
                sl = {n: t[b0:b1] for n, t in s.items() if n not in ("pi", "lar")}
                pi, lar = s["pi"][A * b0:A * b1], s["lar"][b0 * xld:b1 * xld]
                nxt = dict(next_idx=sl["idx"], next_lar=lar, lar_ld=xld, lar_col0=256, A=A)
                if k == 0:
                    ops.policy_step(b1 - b0, A, X[b0 * 256:], 256, Wp, bp, Wv, bv, u[b0:b1], pi, sl["v"], sl["a"])
                    act_before = sl["active"].clone()
                    v.process(sl["a"], act_before, sl["r"], sl["t"], reset_on_terminal=True, track_score=True)
                    ops.rollout_advance(b1 - b0, sl["t"], sl["active"], sl["log"], sl["n"], sl["te"])
                    v.ring.cur_idx(out=sl["idx"], base_actor=b0)
                elif k == 1:
                    ops.policy_step(b1 - b0, A, X[b0 * 256:], 256, Wp, bp, Wv, bv, u[b0:b1], pi, sl["v"], sl["a"])
                    v.rollout_step(sl["a"], sl["r"], sl["t"], sl["active"], sl["log"], sl["n"], sl["te"],
                                   index_parent=True, **nxt)
                else:
                    feat = X[b0 * 256:b1 * 256]
                    net = type("Net", (), {"p": dict(W_base_fc_p=Wp, b_base_fc_p=bp, W_base_fc_v=Wv, b_base_fc_v=bv)})
                    v.policy_rollout_step(net, feat, 256, u[b0:b1], pi, sl["v"], sl["a"], sl["r"], sl["t"], sl["active"],
                                          sl["log"], sl["n"], sl["te"], index_parent=True, **nxt)
        for name in ARRAYS:
            for e in envs[1:]:
                assert torch.equal(getattr(envs[0].ring, name), getattr(e.ring, name)), (step, name)
        for key in ("active", "log", "n", "te", "a", "pi", "v", "idx"):
            for s in st[1:]:
                assert torch.equal(st[0][key], s[key]), (step, key)
        live = st[0]["log"].bool()
        for key in ("r", "t"):
            for s in st[1:]:
                assert torch.equal(st[0][key][live], s[key][live]), (step, key)
        assert torch.equal(st[1]["lar"], st[2]["lar"]), step
        lar = st[1]["lar"].view(B, xld)[:, 256:256 + A + 1].cpu().numpy()
        la, lr = envs[0].ring.last_action.cpu().numpy(), envs[0].ring.last_reward.cpu().numpy()
        np.testing.assert_array_equal(lar[:, :A], np.eye(A, dtype=np.float32)[la], err_msg=str(step))
        np.testing.assert_array_equal(lar[:, A], lr, err_msg=str(step))
        n_term += int(st[0]["te"].sum())
        n_rew |= set(st[0]["r"][live].cpu().numpy().tolist())
        if step % 10 == 9:
            for s in st:
                s["active"].fill_(1); s["te"].zero_(); s["n"].zero_()
    assert n_term > 0 and {0.0, -1.0} <= n_rew, (n_term, n_rew)
    assert int(envs[0].ring.episode.max()) > 1


def test_views_and_actor_base_step_the_same_actors():
    """Eight actors as one environment, as two views of one, and as two environments of four with actor_base 0 and 4."""
    from unreal_amd.environment.arcade_environment import BatchedArcadeEnvironment
    B, H = 8, 3
    conf = _conf(**SHORT)
    whole, viewed = _env(B, H, conf, seed=5), _env(B, H, conf, seed=5)
    halves = [_env(4, H, conf, seed=5, actor_base=b0, actors_total=B) for b0 in (0, 4)]
    views = [viewed.view(0, 3), viewed.view(3, B)]
    assert isinstance(views[0], BatchedArcadeEnvironment) and views[1].arcade[1] == 3 and views[1].base_actor == 3
    with pytest.raises(ValueError):
        BatchedArcadeEnvironment(4, H, DEV, config=conf, actor_base=6, actors_total=B)
    rs = np.random.RandomState(3)
    z = lambda dt: torch.zeros(B, dtype=dt, device=DEV)
    outs = [(z(torch.float32), z(torch.int32)) for _ in range(3)]
    for step in range(60):
        acts = torch.from_numpy(rs.randint(0, 4, B).astype(np.int32)).to(DEV)
        whole.process(acts, None, *outs[0], track_score=True)
        for v, (b0, b1) in zip(views, ((0, 3), (3, B))):
            v.process(acts[b0:b1], None, outs[1][0][b0:b1], outs[1][1][b0:b1], track_score=True)
        for e, b0 in zip(halves, (0, 4)):
            e.process(acts[b0:b0 + 4], None, outs[2][0][b0:b0 + 4], outs[2][1][b0:b0 + 4], track_score=True)
        for name in ARRAYS:
            a = getattr(whole.ring, name)
            assert torch.equal(a, getattr(viewed.ring, name)), (step, name)
            assert torch.equal(a, torch.cat([getattr(e.ring, name) for e in halves])), (step, name)
        for o in outs[1:]:
            assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]), step
    assert int(whole.ring.episode.min()) > 1 and len(set(whole.current_records()[:, 1].tolist())) > 2


def test_a_block_of_another_game_writes_nothing():
    from unreal_amd import ops
    B = 8
    env = _env(B, 2, _conf(), seed=1)
    block = env.arcade[0].clone()
    block[0] = 2
    other = (block, 0)
    env.ring.frames.fill_(0x5A)
    names = ARRAYS + ("_cur",)
    before = {n: getattr(env.ring, n).clone() for n in names}
    z = lambda dt, v: torch.full((B,), v, dtype=dt, device=DEV)
    st = _rollout_state(B, 264)
    outs = dict(r=z(torch.float32, -7.5), t=z(torch.int32, -7))
    ops.arcade_reset(env.ring, None, arcade=other)
    ops.arcade_step(env.ring, z(torch.int32, 1), None, outs["r"], outs["t"], arcade=other)
    ops.arcade_rollout_step(env.ring, z(torch.int32, 1), outs["r"], outs["t"], st["active"], st["log"], st["n"], st["te"],
                            next_idx=st["idx"], arcade=other)
    torch.cuda.synchronize()
    for n, t in before.items():
        assert torch.equal(getattr(env.ring, n), t), n
    assert (outs["r"] == -7.5).all() and (outs["t"] == -7).all()
    assert (st["active"] == 1).all() and not st["log"].any() and not st["n"].any() and not st["idx"].any()
    with pytest.raises(ValueError):
        ops.arcade_rollout_step(env.ring, z(torch.int32, 1), outs["r"], outs["t"], st["active"], st["log"], st["n"], st["te"],
                                A=6, arcade=env.arcade)


# ---- 4. trainer, evaluation, batch 1 -----------------------------------------------------------------------------------------
def _register(name, **kw):
    from unreal_amd.environment.environment import Environment
    Environment.register_arcade_config(name, **kw)
    return Environment.ARCADE_CONFIG[name]


@pytest.mark.parametrize("use_lstm,aux", [(True, True), (False, False)])
def test_process_on_the_arcade_matches_oracle(use_lstm, aux):
    """Trainer.process against OracleTrainer with one host model per actor (rewards 7, 1, -1: the LSTM input's reward
    column unbounded), at the bars of tests/test_forage_maze_gpu.py."""
    from unreal_amd.environment.environment import Environment
    from oracle.trainer import OracleTrainer, ExplicitDraws
    name = "arcade_short_%d%d" % (use_lstm, aux)
    conf = _register(name, **SHORT)
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(use_lstm, aux, H, T)
        cfg["initial_learning_rate"] = 7.0711e-4
        net, applier, tr, draws = _build(cfg, B, seed=3, env_type="arcade", env_name=name)
        assert tr.action_size == 4 and not net.lar_bounded and tr.rp_mode == 0 and tr.objective_size == 0
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = AM.host_batch(conf, B, seed=tr.seed)
        orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=hosts)
        while not tr._full:
            tr.process(None, 0)
        for step_u in draws.log:
            for b in range(B):
                edraws[b].action_u.append(float(step_u[b]))
        orc.fill()
        np.testing.assert_array_equal(tr.ring.count.cpu().numpy(), [a.exp.count for a in orc.actors])
        np.testing.assert_array_equal(tr.environment.current_records(), [h.record() for h in hosts])
        rewards, n_term = set(), 0
        for it in range(4):
            draws.log.clear()
            lr = tr._anneal_learning_rate(0)
            tr.compute_gradients()
            g_dev = {k: v.detach().cpu().double().numpy().copy() for k, v in net.g.items()}
            tr.last_grad_norm = applier.step(net.params.flat, net.grads.flat, lr)
            losses_dev = tr._publish_losses()
            _feed_draws(cfg, draws.log, edraws, T, B)
            steps_o, infos, losses_o, mean_g, norm_o = orc.process_batched(0)
            n_dev = tr.n_steps.cpu().numpy()
            acts = tr.actions.cpu().numpy().reshape(T, B)
            rews = tr.rewards.cpu().numpy().reshape(T, B)
            assert int(n_dev.sum()) == steps_o
            for b in range(B):
                n = infos[b]["n"]
                assert n_dev[b] == n
                assert list(acts[:n, b]) == infos[b]["actions"]
                assert list(rews[:n, b]) == [float(r) for r in infos[b]["rewards"]]
                assert bool(tr.terminal_end.cpu()[b]) == infos[b]["terminal_end"]
                rewards |= set(float(r) for r in infos[b]["rewards"])
                n_term += infos[b]["terminal_end"]
            for key in ("policy_loss", "value_loss", "pc_loss", "vr_loss", "rp_loss", "total_loss"):
                if key not in losses_dev or key not in losses_o[0]:
                    continue
                want = np.mean([l[key] for l in losses_o])
                assert abs(losses_dev[key] - want) <= LOSS_ATOL + LOSS_RTOL * abs(want), (it, key, losses_dev[key], want)
            for (pname, _), gref in zip(orc.params.items(), mean_g):
                gr = gref.numpy().reshape(-1)
                assert np.abs(g_dev[pname] - gr).max() <= GRAD_ATOL + GRAD_REL * np.abs(gr).max(), (it, pname)
            assert abs(float(tr.last_grad_norm.cpu()[0]) - norm_o) <= 1e-4 * max(1.0, norm_o)
            np.testing.assert_array_equal(tr.environment.current_records(), [h.record() for h in hosts])
        assert n_term > 0 and -1.0 in rewards, (n_term, rewards)
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


def test_grouped_process_on_the_arcade_is_the_reference_algorithm():
    """groups = B: one process() call = B sequential single-actor passes, against OracleTrainer.process_async."""
    from unreal_amd.environment.environment import Environment
    from oracle.trainer import OracleTrainer, ExplicitDraws
    name = "arcade_short_grouped"
    conf = _register(name, **SHORT)
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(True, True, H, T)
        cfg["initial_learning_rate"] = 7.0711e-4
        net, applier, tr, draws = _build(cfg, B, seed=13, env_type="arcade", env_name=name, groups=B)
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = AM.host_batch(conf, B, seed=tr.seed)
        orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=hosts)
        while not tr._full:
            tr.process(None, 0)
        for k, u in enumerate(draws.log):
            edraws[k % B].action_u.append(float(u[0]))
        orc.fill()
        np.testing.assert_array_equal(tr.full_ring.count.cpu().numpy(), [a.exp.count for a in orc.actors])
        global_t, n_scores = 0, 0
        for it in range(3):
            draws.log.clear()
            steps_dev, score_dev = tr.process(None, global_t)
            assert len(draws.log) == 5 * B
            steps_o = 0
            for b in range(B):
                lg = draws.log[5 * b:5 * b + 5]
                edraws[b].action_u = [float(x) for x in lg[0]]
                edraws[b].seq_starts = [int(lg[1][0]), int(lg[2][0])]
                edraws[b].rp_coin, edraws[b].rp_u = [int(lg[3][0])], [float(lg[4][0])]
                d, sc, _ = orc.process_async(b, global_t + b * T)
                steps_o += d
                n_scores += sc is not None
                edraws[b].action_u = []
            assert steps_dev == steps_o
            for pname, ref in orc.params.items():
                got = net.p[pname].cpu().double().numpy()
                want = ref.numpy().reshape(-1)
                assert np.abs(got - want).max() <= 2e-6 + 2e-5 * np.abs(want).max(), (it, pname)
            np.testing.assert_array_equal(tr.full_environment.current_records(), [h.record() for h in hosts])
            global_t += steps_dev
        assert n_scores > 0
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


def test_evaluate_on_the_arcade_matches_the_host_model():
    """Evaluate(arcade=name): rewards / terminals of every step agree with the host model replaying the device's actions,
    and the statistics are those of the models' first episodes."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.evaluate import Evaluate
    name = "arcade_eval"
    conf = _register(name, rows=1, row_rewards=(3,), lives=2, paddle_width=24, ball_speed=4, serve_wait=1, life_reward=-1,
                     max_episode_steps=40)
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
        hosts = AM.host_batch(conf, B, seed=seed)
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
                        first[b] = (ret[b], h.ep_steps, h.totals[0] - start[b][0], h.totals[1] - start[b][1], h.success,
                                    "end_timeout" in h.events)
                    ret[b], start[b] = 0, list(h.totals)
                    h.reset()
        assert None not in first
        col = lambda i: np.array([f[i] for f in first], np.float64)
        assert res["episodes"] == B and res["timeouts"] == B - int(col(4).sum())
        for key, want in (("success_rate", col(4).mean()), ("mean_return", col(0).mean()), ("return_std", col(0).std()),
                          ("mean_length", col(1).mean()), ("bricks_per_episode", col(2).mean()),
                          ("lives_lost_per_episode", col(3).mean())):
            assert abs(res[key] - want) < 1e-9, (key, res[key], want)
        assert col(3).sum() > 0 and set(col(1).tolist()) != {40.0}, first
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


def test_batch1_environment():
    """Environment.create_environment('arcade', name): 100 steps of images, rewards, terminals and pixel change of the
    host model; no reset on terminal (the caller resets), and a game that is stepped past its terminal goes on."""
    from unreal_amd.environment.environment import Environment
    name = "arcade_batch1"
    conf = _register(name, rows=2, row_rewards=(7, 1), lives=2, paddle_width=24, ball_speed=4, serve_wait=2, life_reward=-1,
                     max_episode_steps=60)
    try:
        env = Environment.create_environment("arcade", name)
        host = AM.HostBreakout(conf, 0, 0)
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
                if n_term == 0 and past < 4:           # the first terminal: three more steps before the reset
                    continue
                n_term += 1
                past = 0
                env.reset()
                host.reset()
                np.testing.assert_array_equal(env.last_state["image"], host.last_state["image"])
        assert n_term > 1
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)
