"""The device arcade's duel (csrc/arcade.hip) bit for bit against the host model of tests/duel_model.py: resets,
random and scripted traces with every event of the rules, the fused rollout entries against the two-launch path, views and
actor_base, a block of no game, a Breakout and a duel environment stepped in turn, Trainer.process against OracleTrainer,
Evaluate and the batch-1 environment."""
import numpy as np
import pytest
import torch

try:
    import arcade_model as AM
    import duel_model as DM
    from test_arcade_gpu import _conf, _check_state, _register, ARRAYS, SHORT as BREAKOUT_SHORT
    from test_trainer_gpu import _cfg, _build, _feed_draws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL
    from test_fp_maze_gpu import _current_frames, _rollout_state
except ImportError:            # imported as tests.<module>
    from tests import arcade_model as AM
    from tests import duel_model as DM
    from tests.test_arcade_gpu import _conf, _check_state, _register, ARRAYS, SHORT as BREAKOUT_SHORT
    from tests.test_trainer_gpu import _cfg, _build, _feed_draws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL
    from tests.test_fp_maze_gpu import _current_frames, _rollout_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB, PC = 21168, 400
# short episodes with rewards of both signs: two points, a fast ball that serves itself towards either side, a narrow slow
# opponent (a ball served upwards is usually a point won), a step limit
SHORT = dict(game="duel", points=2, paddle_width=24, ball_speed=4, serve_wait=1, opponent_width=4, opponent_speed=1,
             win_reward=7, lose_reward=-1, max_episode_steps=30)


def _env(B, H, conf, seed=0, **kw):
    """A device environment in the state its constructor leaves (episode 0), over zeroed ring memory."""
    from unreal_amd.environment.arcade_environment import BatchedArcadeEnvironment
    env = BatchedArcadeEnvironment(B, H, DEV, config=conf, seed=seed, **kw)
    assert env.frame_scale == 1.0 / 255.0 and env.objective_size == 0
    env.ring.frames.zero_()           # (torch.empty: slots no step has written would hold stale allocator bytes)
    env.ring.r_pc.zero_()
    env.ring.episode.fill_(-1)        # as before the constructor's reset: the traces start in episode 0, as
    env.reset()                       # tests/test_duel_cpu.py runs them on the model
    return env


def _hosts(conf, B, seed, actor_base=0, n_frames=None):
    """Host models of an environment built by _env (episode 0: the model's constructor resets once, too)."""
    cls = DM.HostDuel if conf.game == "duel" else AM.HostBreakout
    return [cls(conf, actor_base + b, seed, frames=n_frames is None or b < n_frames) for b in range(B)]


# ---- 1. resets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 64])
@pytest.mark.parametrize("kw", [dict(), dict(paddle_width=4, opponent_width=24), dict(paddle_width=24, opponent_width=4)])
def test_reset_matches_the_host_model(B, kw):
    conf = _conf(game="duel", **kw)
    env = _env(B, 3, conf, seed=7)
    models = _hosts(conf, B, 7)
    _check_state(env, models, "reset", count=np.zeros(B, np.int32))
    frame = _current_frames(env.ring)[0].reshape(84, 84, 3)
    count = lambda colour: int((frame == colour).all(2).sum())
    assert (count(AM.WHITE), count(AM.BORDER), count(AM.PADDLE), count(DM.OPPONENT)) == \
        (0, 816, 2 * conf.paddle_width, 2 * conf.opponent_width)


def test_masked_reset_over_sentinel_slots():
    B = 64
    conf = _conf(game="duel", opponent_speed=3)
    env = _env(B, 3, conf, seed=2)
    models = _hosts(conf, B, 2)
    acts = torch.from_numpy(np.random.RandomState(0).randint(0, 4, B).astype(np.int32)).to(DEV)
    for _ in range(12):                                # serve and fly a little: the records are no reset records
        env.process(acts, None, None, None)
        for m, a in zip(models, acts.cpu().numpy()):
            m.process(a)
    before = env.current_records()
    assert (before[:, 6] != 36).any() and (before[:, 5] < 0).any()
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
def _run_trace(conf, B, steps, choose, n_frames, seed=DM.TRACE_SEED):
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


@pytest.mark.parametrize("k", range(len(DM.TRACE_SETTINGS)))
def test_random_steps_match_the_host_model(k):
    """300 random steps of 200 actors under an `active` mask; tests/test_duel_cpu.py checks on the model alone that the
    trace holds these events."""
    acts, active = DM.trace_inputs(k)
    seen = _run_trace(_conf(**DM.TRACE_SETTINGS[k]), DM.TRACE_B, DM.TRACE_STEPS, lambda s, models: (acts[s], active[s]),
                      DM.TRACE_FRAMES)
    assert DM.TRACE_EVENTS[k] <= seen, DM.TRACE_EVENTS[k] - seen


def test_scripted_steps_win_matches_and_time_out():
    """The ending no random trace reaches, and matches won: a policy that follows the ball beats a slow opponent; a rally
    that never ends runs into max_episode_steps.  Frames and pixel change of every actor."""
    B = DM.SCRIPTED_B

    def choose(s, models):
        return np.array([AM.follow_ball(m) for m in models], np.int32), np.ones(B, np.int32)
    seen = _run_trace(_conf(**DM.SCRIPTED_SETTING), B, DM.SCRIPTED_STEPS, choose, B)
    assert DM.SCRIPTED_EVENTS <= seen, DM.SCRIPTED_EVENTS - seen


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
    assert n_term > 0 and {0.0, -1.0, 7.0} <= n_rew, (n_term, n_rew)
    assert int(envs[0].ring.episode.max()) > 0


def test_views_and_actor_base_step_the_same_actors():
    """Eight actors as one environment, as two views of one, and as two environments of four with actor_base 0 and 4."""
    B, H = 8, 3
    conf = _conf(**SHORT)
    whole, viewed = _env(B, H, conf, seed=5), _env(B, H, conf, seed=5)
    halves = [_env(4, H, conf, seed=5, actor_base=b0, actors_total=B) for b0 in (0, 4)]
    views = [viewed.view(0, 3), viewed.view(3, B)]
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
    assert int(whole.ring.episode.min()) > 0
    _check_state(whole, _replay(conf, B, 5, 3, 60), "the whole environment against the model")


def _replay(conf, B, seed, action_seed, steps):
    """The models after `steps` steps of the random actions of RandomState(action_seed), reset at every terminal."""
    models = _hosts(conf, B, seed)
    rs = np.random.RandomState(action_seed)
    for _ in range(steps):
        acts = rs.randint(0, 4, B)
        for m, a in zip(models, acts):
            if m.process(a)[2]:
                m.reset()
    return models


def test_a_block_of_no_game_writes_nothing():
    from unreal_amd import ops
    B = 8
    env = _env(B, 2, _conf(game="duel"), seed=1)
    names = ARRAYS + ("_cur",)
    z = lambda dt, v: torch.full((B,), v, dtype=dt, device=DEV)
    for game in (4, 2, 0, -3):
        block = env.arcade[0].clone()
        block[0] = game
        other = (block, 0)
        env.ring.frames.fill_(0x5A)
        before = {n: getattr(env.ring, n).clone() for n in names}
        st = _rollout_state(B, 264)
        outs = dict(r=z(torch.float32, -7.5), t=z(torch.int32, -7))
        ops.arcade_reset(env.ring, None, arcade=other)
        ops.arcade_step(env.ring, z(torch.int32, 1), None, outs["r"], outs["t"], arcade=other)
        ops.arcade_rollout_step(env.ring, z(torch.int32, 1), outs["r"], outs["t"], st["active"], st["log"], st["n"],
                                st["te"], next_idx=st["idx"], arcade=other)
        torch.cuda.synchronize()
        for n, t in before.items():
            assert torch.equal(getattr(env.ring, n), t), (game, n)
        assert (outs["r"] == -7.5).all() and (outs["t"] == -7).all()
        assert (st["active"] == 1).all() and not st["log"].any() and not st["n"].any() and not st["idx"].any()
    with pytest.raises(ValueError):
        ops.arcade_rollout_step(env.ring, z(torch.int32, 1), outs["r"], outs["t"], st["active"], st["log"], st["n"], st["te"],
                                A=6, arcade=env.arcade)


def test_a_breakout_and_a_duel_environment_stepped_in_turn():
    """The kernels branch on the block's game id: one environment of each game in one process, stepped alternately with
    the same actions; both stay equal to their models, so nothing leaks across the branch."""
    B, H, seed = 16, 3, 4
    confs = [_conf(**BREAKOUT_SHORT), _conf(**SHORT)]
    envs = [_env(B, H, c, seed=seed) for c in confs]
    models = [_hosts(c, B, seed) for c in confs]
    assert [e.arcade[0][0].item() for e in envs] == [1, 3]
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
            _check_state(envs[k], models[k], "step %d game %d" % (step, k))
    assert min(ends) > 0


# ---- 4. trainer, evaluation, batch 1 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_lstm,aux", [(True, True), (False, False)])
def test_process_on_the_duel_matches_oracle(use_lstm, aux):
    """Trainer.process against OracleTrainer with one host model per actor (rewards 7 and -1: the LSTM input's reward
    column unbounded and of either sign), at the bars of tests/test_arcade_gpu.py."""
    from unreal_amd.environment.environment import Environment
    from oracle.trainer import OracleTrainer, ExplicitDraws
    name = "duel_short_%d%d" % (use_lstm, aux)
    conf = _register(name, **SHORT)
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(use_lstm, aux, H, T)
        cfg["initial_learning_rate"] = 7.0711e-4
        net, applier, tr, draws = _build(cfg, B, seed=3, env_type="arcade", env_name=name)
        assert tr.action_size == 4 and not net.lar_bounded and tr.rp_mode == 0 and tr.objective_size == 0
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = DM.host_batch(conf, B, seed=tr.seed)
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
        assert n_term > 0 and rewards & {7.0, -1.0}, (n_term, rewards)
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


def test_grouped_process_on_the_duel_is_the_reference_algorithm():
    """groups = B: one process() call = B sequential single-actor passes, against OracleTrainer.process_async."""
    from unreal_amd.environment.environment import Environment
    from oracle.trainer import OracleTrainer, ExplicitDraws
    name = "duel_short_grouped"
    conf = _register(name, **SHORT)
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(True, True, H, T)
        cfg["initial_learning_rate"] = 7.0711e-4
        net, applier, tr, draws = _build(cfg, B, seed=13, env_type="arcade", env_name=name, groups=B)
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = DM.host_batch(conf, B, seed=tr.seed)
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


def test_evaluate_on_the_duel_matches_the_host_model():
    """Evaluate(arcade=name): rewards / terminals of every step agree with the host model replaying the device's actions,
    and the statistics are those of the models' first episodes."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.evaluate import Evaluate
    name = "duel_eval"
    conf = _register(name, game="duel", points=2, paddle_width=24, ball_speed=4, serve_wait=1, opponent_width=4,
                     opponent_speed=1, win_reward=3, lose_reward=-1, max_episode_steps=40)
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
        hosts = DM.host_batch(conf, B, seed=seed)
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
                                    "end_timeout" in h.events, "end_lose" in h.events)
                    ret[b], start[b] = 0, list(h.totals)
                    h.reset()
        assert None not in first
        col = lambda i: np.array([f[i] for f in first], np.float64)
        assert sorted(res) == sorted(("episodes", "success_rate", "mean_return", "return_std", "mean_length", "timeouts",
                                      "losses", "points_won_per_episode", "points_lost_per_episode"))
        assert res["episodes"] == B and res["timeouts"] == int(col(5).sum()) and res["losses"] == int(col(6).sum())
        assert int(col(4).sum() + col(5).sum() + col(6).sum()) == B
        for key, want in (("success_rate", col(4).mean()), ("mean_return", col(0).mean()), ("return_std", col(0).std()),
                          ("mean_length", col(1).mean()), ("points_won_per_episode", col(2).mean()),
                          ("points_lost_per_episode", col(3).mean())):
            assert abs(res[key] - want) < 1e-9, (key, res[key], want)
        assert col(2).sum() + col(3).sum() > 0 and set(col(1).tolist()) != {40.0}, first
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


def test_batch1_environment():
    """Environment.create_environment('arcade', name): 100 steps of images, rewards, terminals and pixel change of the
    host model; no reset on terminal (the caller resets), and a game that is stepped past its terminal goes on."""
    from unreal_amd.environment.environment import Environment
    name = "duel_batch1"
    conf = _register(name, game="duel", points=1, paddle_width=24, ball_speed=4, serve_wait=2, opponent_width=4,
                     opponent_speed=1, win_reward=7, lose_reward=-1, max_episode_steps=60)
    try:
        env = Environment.create_environment("arcade", name)
        host = DM.HostDuel(conf, 0, 0)
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
                if n_term == 0 and past < 12:          # the first terminal: eleven more steps (a serve, a second point)
                    continue
                n_term += 1
                past = 0
                env.reset()
                host.reset()
                np.testing.assert_array_equal(env.last_state["image"], host.last_state["image"])
        assert n_term > 1
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)
