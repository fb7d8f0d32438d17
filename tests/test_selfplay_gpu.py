"""The device arcade's self-play duel (csrc/arcade.hip) bit for bit against the host model of
tests/selfplay_model.py: resets, the four random traces (tests/test_selfplay_cpu.py shows they hold every event), the fused
entries against the two-launch path, the time-limit forms, views and actor_base, the launcher's refusals,
Trainer.process against OracleTrainer, grouped and minibatched runs, Evaluate against the scripted opponent and head to
head."""
import numpy as np
import pytest
import torch

try:
    import arcade_model as AM
    import duel_model as DM
    import selfplay_model as SM
    from test_arcade_gpu import _check_state, ARRAYS
    from test_trainer_gpu import _cfg, _build, _feed_draws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL
    from test_fp_maze_gpu import _current_frames, _rollout_state
    from test_arcade_mix_gpu import _build_options
except ImportError:            # imported as tests.<module>
    from tests import arcade_model as AM
    from tests import duel_model as DM
    from tests import selfplay_model as SM
    from tests.test_arcade_gpu import _check_state, ARRAYS
    from tests.test_trainer_gpu import _cfg, _build, _feed_draws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL
    from tests.test_fp_maze_gpu import _current_frames, _rollout_state
    from tests.test_arcade_mix_gpu import _build_options

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB, PC = 21168, 400
# short matches with rewards of both signs and magnitudes above 1: two points, a fast ball that serves itself, a step limit
SHORT = dict(points=2, paddle_width=24, ball_speed=4, serve_wait=1, win_reward=7, lose_reward=-3, max_episode_steps=30)
# the time-limit setting: at 11 steps random play ends matches by the limit, by a point in the last allowed step and earlier
TL = dict(points=1, paddle_width=4, ball_speed=4, serve_wait=1, win_reward=7, lose_reward=-3, max_episode_steps=11)


def _sp(**kw):
    from unreal_amd.environment.arcade_environment import ArcadeSelfPlay
    return ArcadeSelfPlay(**kw)


def _env(B, H, conf, seed=0, **kw):
    """A device environment in the state its constructor leaves (episode 0), over zeroed ring memory."""
    from unreal_amd.environment.arcade_environment import BatchedArcadeEnvironment
    env = BatchedArcadeEnvironment(B, H, DEV, config=conf, seed=seed, **kw)
    env.ring.frames.zero_()
    env.ring.r_pc.zero_()
    env.ring.episode.fill_(-1)
    env.reset()
    return env


def _seats(conf, B, seed, actor_base=0, n_frames=None):
    return [SM.HostSeat(conf, actor_base + b, seed, frames=n_frames is None or b < n_frames) for b in range(B)]


def _mirrored(env):
    rec = env.current_records()
    np.testing.assert_array_equal(rec[1::2], SM.mirror(rec[0::2]))
    return rec


# ---- 1. resets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 6, 64])
def test_reset_matches_the_host_model(B):
    conf = _sp(paddle_width=8)
    env = _env(B, 3, conf, seed=7)
    assert len(env.arcade) == 3
    _check_state(env, _seats(conf, B, 7), "reset", count=np.zeros(B, np.int32))
    rec = _mirrored(env)
    assert (rec[0::2, 2] == 0).all() and (rec[1::2, 2] == 86).all() and (rec[:, [0, 6]] == 38).all()
    frames = _current_frames(env.ring)
    for b in (0, 1):                                   # both seats see themselves at the bottom in the paddle's red
        f = frames[b].reshape(84, 84, 3)
        count = lambda colour: int((f == colour).all(2).sum())
        assert (count(AM.WHITE), count(AM.BORDER), count(AM.PADDLE), count(DM.OPPONENT)) == (0, 816, 16, 16)
        assert (f[78:80, 38:46] == AM.PADDLE).all() and (f[8:10, 38:46] == DM.OPPONENT).all()


def test_masked_reset_over_sentinel_slots_resets_whole_pairs():
    B = 64
    conf = _sp(paddle_speed=5)
    env = _env(B, 3, conf, seed=2)
    seats = _seats(conf, B, 2)
    rs = np.random.RandomState(0)
    for _ in range(12):                                # serve and fly a little: the records are no reset records
        acts = rs.randint(0, 4, B).astype(np.int32)
        env.process(torch.from_numpy(acts).to(DEV), None, None, None)
        SM.step_pairs(seats, acts)
    before = _mirrored(env)
    assert (before[:, 6] != 36).any() and (before[:, 5] < 0).any()
    env.ring.frames.fill_(0xAB)
    mask = (np.random.RandomState(1).rand(B) < 0.3).astype(np.int32)
    mask[0:6] = (1, 0, 0, 1, 0, 0)                     # seat 0 alone, seat 1 alone, neither
    env.reset(torch.from_numpy(mask).to(DEV))
    pair = np.repeat(mask[0::2] | mask[1::2], 2)
    assert 0 < pair.sum() < B and (pair != mask).any()
    for s, k in zip(seats, pair):
        if k:
            s.reset()
    rec, frames = _mirrored(env), _current_frames(env.ring)
    for b, s in enumerate(seats):
        np.testing.assert_array_equal(rec[b], s.record())
        if pair[b]:
            np.testing.assert_array_equal(frames[b], s.frame.reshape(-1))
        else:
            assert (frames[b] == 0xAB).all() and (rec[b] == before[b]).all()
    np.testing.assert_array_equal(env.ring.episode.cpu().numpy(), [s.episode for s in seats])
    np.testing.assert_array_equal(env.ring.ep_steps.cpu().numpy(), [s.ep_steps for s in seats])
    idx = env.ring.cur_idx().long().cpu().numpy()      # every slot but the reset actors' current ones is untouched
    others = np.ones(B * env.ring.H1, bool)
    others[idx[pair.astype(bool)]] = False
    assert (env.ring.frames.view(-1, FB).cpu().numpy()[others] == 0xAB).all()


# ---- 2. traces -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(SM.TRACE_SETTINGS)))
def test_random_steps_match_the_host_model(k):
    """300 random steps of 64 actors (32 games) under an `active` mask: every step compares both seats' records, rewards,
    terminals, ep_steps and episode of all actors, frames and pixel change of the first three pairs, and the mirror."""
    conf = _sp(**SM.TRACE_SETTINGS[k])
    B, H = SM.TRACE_B, 3
    H1 = H + 1
    n_frames = 2 * SM.TRACE_PAIR_FRAMES
    acts, active = SM.trace_inputs(k)
    env = _env(B, H, conf, seed=SM.TRACE_SEED)
    ring = env.ring
    seats = _seats(conf, B, SM.TRACE_SEED, n_frames=n_frames)
    out_r = torch.zeros(B, dtype=torch.float32, device=DEV)
    out_t = torch.zeros(B, dtype=torch.int32, device=DEV)
    count, prev_term = np.zeros(B, np.int64), np.zeros(B, bool)
    seen, n_idle_half = set(), 0
    for s in range(SM.TRACE_STEPS):
        out_r.fill_(-7.5); out_t.fill_(-7)
        env.process(torch.from_numpy(acts[s]).to(DEV), torch.from_numpy(active[s]).to(DEV), out_r, out_t,
                    reset_on_terminal=True)
        want_r, want_t = np.full(B, -7.5, np.float32), np.full(B, -7, np.int32)
        pcs = {}
        out = SM.step_pairs(seats, acts[s], active[s])
        for b, (r, t, pc, stepped) in enumerate(out):
            if not stepped:
                n_idle_half += int(active[s][b])       # an active seat whose partner is not: idle
                continue
            seen |= seats[b].events
            want_r[b], want_t[b] = r, int(t)
            if b < n_frames:
                pcs[b] = (b * H1 + count[b] % H1, pc)
            if not (t and count[b] > 0 and prev_term[b]):
                count[b] += 1
            prev_term[b] = t
            if t:
                seats[b].reset()
        what = "trace %d step %d" % (k, s)
        np.testing.assert_array_equal(out_r.cpu().numpy(), want_r, err_msg=what)
        np.testing.assert_array_equal(out_t.cpu().numpy(), want_t, err_msg=what)
        _check_state(env, seats, what, count=count)
        _mirrored(env)
        r_pc = ring.r_pc.view(-1, PC)
        for b, (slot, pc) in pcs.items():
            np.testing.assert_array_equal(r_pc[slot].cpu().numpy(), pc.reshape(-1), err_msg="%s actor %d" % (what, b))
    assert n_idle_half > 0
    if k == 1:                                         # this trace alone holds every event (tests/test_selfplay_cpu.py)
        assert seen >= SM.EVERY_EVENT, SM.EVERY_EVENT - seen


# ---- 3. fused entries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tl", [False, True])
@pytest.mark.parametrize("B", [2, 64])
def test_fused_policy_steps_are_the_two_launch_path(B, tl):
    """policy_rollout_step == policy_step + rollout_step, bit for bit: actions, pi, V, ring (with the final observations),
    records and the next step's rows; the records stay mirror images, so both workgroups of a pair drew the same actions."""
    from unreal_amd import ops
    H, A, xld = 4, 4, 264
    rs = np.random.RandomState(B)
    dev = lambda a, dt: torch.from_numpy(np.asarray(a)).to(DEV, dt)
    Wp = dev(rs.uniform(-.3, .3, 256 * A), torch.float32); bp = dev(rs.uniform(-.1, .1, A), torch.float32)
    Wv = dev(rs.uniform(-.3, .3, 256), torch.float32); bv = dev(rs.uniform(-.1, .1, 1), torch.float32)
    net = type("Net", (), {"p": dict(W_base_fc_p=Wp, b_base_fc_p=bp, W_base_fc_v=Wv, b_base_fc_v=bv)})
    conf = _sp(**TL)
    envs = [_env(B, H, conf, seed=9, final_obs=tl) for _ in range(2)]
    assert (envs[0].ring.final_obs is not None) == tl
    st = [_rollout_state(B, xld) for _ in envs]
    flags, n_rew = set(), set()
    for step in range(60 if B == 2 else 30):
        X = dev(rs.uniform(-1, 1, (B, 256)), torch.float32).view(-1)
        u = dev(rs.uniform(0, 1, B), torch.float64)
        for k, (e, s) in enumerate(zip(envs, st)):
            nxt = dict(next_idx=s["idx"], next_lar=s["lar"], lar_ld=xld, lar_col0=256, A=A)
            if k == 0:
                ops.policy_step(B, A, X, 256, Wp, bp, Wv, bv, u, s["pi"], s["v"], s["a"])
                e.rollout_step(s["a"], s["r"], s["t"], s["active"], s["log"], s["n"], s["te"], **nxt)
            else:
                e.policy_rollout_step(net, X, 256, u, s["pi"], s["v"], s["a"], s["r"], s["t"], s["active"], s["log"],
                                      s["n"], s["te"], **nxt)
        for name in ARRAYS:
            assert torch.equal(getattr(envs[0].ring, name), getattr(envs[1].ring, name)), (step, name)
        for key in ("active", "log", "n", "te", "a", "pi", "v", "idx", "lar"):
            assert torch.equal(st[0][key], st[1][key]), (step, key)
        live = st[0]["log"].bool()
        for key in ("r", "t"):
            assert torch.equal(st[0][key][live], st[1][key][live]), (step, key)
        _mirrored(envs[1])
        act = st[1]["active"].cpu().numpy()
        assert (act[0::2] == act[1::2]).all()
        flags |= set(st[1]["te"].cpu().numpy().tolist())
        n_rew |= set(st[1]["r"][live].cpu().numpy().tolist())
        if step % 10 == 9:
            for s in st:
                s["active"].fill_(1); s["te"].zero_(); s["n"].zero_()
    if B == 64:                                        # (one game alone need not end every way in 60 steps)
        assert flags == ({0, 1, 2} if tl else {0, 1}), flags
        assert {0.0, -3.0, 7.0} <= n_rew, n_rew
    assert flags & {1, 2}, flags
    assert int(envs[0].ring.episode.max()) > 0


# ---- 4. time limits ------------------------------------------------------------------------------------------------------------
def test_time_limits_flag_both_seats_and_keep_each_seats_final_observation():
    """The _tl rollout step: a match cut by the step limit flags both seats 2 and keeps each seat's own final observation,
    byte for byte the model's; a match point in the last allowed step is flagged 1 and stores nothing."""
    B, H = 16, 3
    conf = _sp(**TL)
    env = _env(B, H, conf, seed=3, final_obs=True)
    ring = env.ring
    seats = _seats(conf, B, 3)
    st = _rollout_state(B, 264)
    rs = np.random.RandomState(4)
    fin_want = np.full((B, FB), 0xCD, np.uint8)
    ring.final_obs.fill_(0xCD)
    kinds = {"cut": 0, "last": 0, "early": 0}
    for step in range(60):
        acts = rs.randint(0, 4, B).astype(np.int32)
        st["active"].fill_(1); st["te"].zero_()
        st["r"].fill_(-7.5); st["t"].fill_(-7)
        env.rollout_step(torch.from_numpy(acts).to(DEV), st["r"], st["t"], st["active"], st["log"], st["n"], st["te"],
                         next_idx=st["idx"])
        out = SM.step_pairs(seats, acts)
        want_t = np.zeros(B, np.int32)
        for b, (r, t, pc, _) in enumerate(out):
            if t:
                g = seats[b].game
                cut = not g.ended()
                want_t[b] = 2 if cut else 1
                if b % 2 == 0:
                    kinds["cut" if cut else "last" if g.ep_steps == conf.max_episode_steps else "early"] += 1
                if cut:
                    fin_want[b] = seats[b].frame.reshape(-1)
                seats[b].reset()
        what = "step %d" % step
        np.testing.assert_array_equal(st["t"].cpu().numpy(), want_t, err_msg=what)
        np.testing.assert_array_equal(st["te"].cpu().numpy(), want_t, err_msg=what)
        np.testing.assert_array_equal(st["r"].cpu().numpy(), [o[0] for o in out], err_msg=what)
        np.testing.assert_array_equal(st["active"].cpu().numpy(), (want_t == 0).astype(np.int32), err_msg=what)
        assert (want_t[0::2] == want_t[1::2]).all()
        _check_state(env, seats, what)
        np.testing.assert_array_equal(ring.final_obs.view(B, FB).cpu().numpy(), fin_want, err_msg=what)
    assert min(kinds.values()) > 0, kinds
    # the two seats of a cut pair kept different frames: each its own view
    kept = [b for b in range(0, B, 2) if (fin_want[b] != 0xCD).any()]
    assert kept and any((fin_want[b] != fin_want[b + 1]).any() for b in kept)


# ---- 5. views, actor_base ------------------------------------------------------------------------------------------------------
def test_views_and_actor_base_step_the_same_actors():
    """Eight actors as one environment, as two views of one cut at an even index, and as two environments of four with
    actor_base 0 and 4."""
    B, H = 8, 3
    conf = _sp(**SHORT)
    whole, viewed = _env(B, H, conf, seed=5), _env(B, H, conf, seed=5)
    halves = [_env(4, H, conf, seed=5, actor_base=b0, actors_total=B) for b0 in (0, 4)]
    assert halves[1].arcade[1] == 4
    cuts = ((0, 2), (2, B))
    views = [viewed.view(*c) for c in cuts]
    assert views[1].arcade[1:] == (2, "selfplay")
    rs = np.random.RandomState(3)
    z = lambda dt: torch.zeros(B, dtype=dt, device=DEV)
    outs = [(z(torch.float32), z(torch.int32)) for _ in range(3)]
    seats = _seats(conf, B, 5)
    for step in range(60):
        acts_h = rs.randint(0, 4, B).astype(np.int32)
        acts = torch.from_numpy(acts_h).to(DEV)
        whole.process(acts, None, *outs[0], track_score=True)
        for v, (b0, b1) in zip(views, cuts):
            v.process(acts[b0:b1], None, outs[1][0][b0:b1], outs[1][1][b0:b1], track_score=True)
        for e, b0 in zip(halves, (0, 4)):
            e.process(acts[b0:b0 + 4], None, outs[2][0][b0:b0 + 4], outs[2][1][b0:b0 + 4], track_score=True)
        for name in ARRAYS:
            a = getattr(whole.ring, name)
            assert torch.equal(a, getattr(viewed.ring, name)), (step, name)
            assert torch.equal(a, torch.cat([getattr(e.ring, name) for e in halves])), (step, name)
        for o in outs[1:]:
            assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]), step
        for b, (r, t, pc, _) in enumerate(SM.step_pairs(seats, acts_h)):
            if t:
                seats[b].reset()
    assert int(whole.ring.episode.min()) > 0
    _check_state(whole, seats, "the whole environment against the model")


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_the_launcher_refuses_odd_counts_and_a_block_of_another_game_is_inert():
    from unreal_amd import ops
    from unreal_amd._lib import UnrealLibError
    B = 8
    env = _env(B, 2, _sp(), seed=1)
    names = ARRAYS
    z = lambda n, dt, v: torch.full((n,), v, dtype=dt, device=DEV)
    block = env.arcade[0]

    def attempt(ring, arcade, n, expect_error):
        ring.frames.fill_(0x5A)
        before = {k: getattr(ring, k).clone() for k in names}
        st = _rollout_state(n, 264)
        outs = dict(r=z(n, torch.float32, -7.5), t=z(n, torch.int32, -7))
        calls = (lambda: ops.arcade_reset(ring, None, arcade=arcade),
                 lambda: ops.arcade_step(ring, z(n, torch.int32, 1), None, outs["r"], outs["t"], arcade=arcade),
                 lambda: ops.arcade_rollout_step(ring, z(n, torch.int32, 1), outs["r"], outs["t"], st["active"], st["log"],
                                                 st["n"], st["te"], next_idx=st["idx"], arcade=arcade))
        for c in calls:
            if expect_error:
                with pytest.raises(UnrealLibError, match="-22"):
                    c()
            else:
                c()
        torch.cuda.synchronize()
        for k, t in before.items():
            assert torch.equal(getattr(ring, k), t), (arcade[1:], k)
        assert (outs["r"] == -7.5).all() and (outs["t"] == -7).all()
        assert (st["active"] == 1).all() and not st["log"].any() and not st["n"].any() and not st["idx"].any()

    attempt(env.ring, (block, 1, ops.ARCADE_SELFPLAY), B, True)                  # odd actor_base
    attempt(env.ring, (block, 7, ops.ARCADE_SELFPLAY), B, True)
    odd = ops.ring_view(env.ring, 0, 3)                                          # odd B
    attempt(odd, (block, 0, ops.ARCADE_SELFPLAY), 3, True)
    attempt(ops.ring_view(env.ring, 2, 3), (block, 2, ops.ARCADE_SELFPLAY), 1, True)
    for game in (1, 5, 4, 2, 0, -3):                                             # Breakout's, invaders', no game's
        other = block.clone()
        other[0] = game
        attempt(env.ring, (other, 0, ops.ARCADE_SELFPLAY), B, False)
    from unreal_amd.environment.arcade_environment import BatchedArcadeEnvironment
    for kw in (dict(batch=3), dict(batch=4, actor_base=1, actors_total=6)):
        with pytest.raises(ValueError, match="pairs"):
            BatchedArcadeEnvironment(history_size=2, device=DEV, config=_sp(), **kw)
    with pytest.raises(ValueError, match="odd"):
        env.view(1, 3)


# ---- 7. the trainer ------------------------------------------------------------------------------------------------------------
def _register(name, **kw):
    from unreal_amd.environment.environment import Environment
    Environment.register_arcade_selfplay(name, **kw)
    return Environment.ARCADE_CONFIG[name]


@pytest.mark.parametrize("use_lstm,aux", [(True, True), (False, False)])
def test_process_on_selfplay_matches_oracle(use_lstm, aux):
    """Trainer.process against OracleTrainer with one HostSeat per actor, the partner's actions scripted from what the
    device recorded (the ring's r_action after the fill, tr.actions after each pass); rewards 7 and -3; the bars and shape
    of tests/test_duel_gpu.py's test_process_on_the_duel_matches_oracle."""
    from unreal_amd.environment.environment import Environment
    from oracle.trainer import OracleTrainer, ExplicitDraws
    name = "selfplay_short_%d%d" % (use_lstm, aux)
    conf = _register(name, **SHORT)
    try:
        B, H, T = 4, 40, 20
        cfg = _cfg(use_lstm, aux, H, T)
        cfg["initial_learning_rate"] = 7.0711e-4
        net, applier, tr, draws = _build(cfg, B, seed=3, env_type="arcade", env_name=name)
        assert tr.selfplay and tr.action_size == 4 and not net.lar_bounded and tr.rp_mode == 0
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = SM.host_batch(conf, B, seed=tr.seed, scripts=[[] for _ in range(B)])
        orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=hosts)
        while not tr._full:
            tr.process(None, 0)
        for step_u in draws.log:
            for b in range(B):
                edraws[b].action_u.append(float(step_u[b]))
        count = tr.ring.count.cpu().numpy()
        r_action = tr.ring.r_action.view(B, tr.ring.H1).cpu().numpy()
        assert (count == H).all()
        for b in range(B):
            hosts[b].partner.extend(int(a) for a in r_action[b ^ 1, :count[b ^ 1]])
        orc.fill()
        assert not any(h.partner for h in hosts)
        np.testing.assert_array_equal(count, [a.exp.count for a in orc.actors])
        np.testing.assert_array_equal(_mirrored(tr.environment), [h.record() for h in hosts])
        rewards, n_term = set(), 0
        for it in range(4):
            draws.log.clear()
            lr = tr._anneal_learning_rate(0)
            tr.compute_gradients()
            g_dev = {k: v.detach().cpu().double().numpy().copy() for k, v in net.g.items()}
            tr.last_grad_norm = applier.step(net.params.flat, net.grads.flat, lr)
            losses_dev = tr._publish_losses()
            _feed_draws(cfg, draws.log, edraws, T, B)
            n_dev = tr.n_steps.cpu().numpy()
            acts = tr.actions.cpu().numpy().reshape(T, B)
            rews = tr.rewards.cpu().numpy().reshape(T, B)
            assert (n_dev[0::2] == n_dev[1::2]).all()
            for b in range(B):
                hosts[b].partner.extend(int(a) for a in acts[:n_dev[b ^ 1], b ^ 1])
            steps_o, infos, losses_o, mean_g, norm_o = orc.process_batched(0)
            assert not any(h.partner for h in hosts)
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
            np.testing.assert_array_equal(_mirrored(tr.environment), [h.record() for h in hosts])
        assert n_term > 0 and {7.0, -3.0} <= rewards, (n_term, rewards)
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


@pytest.mark.parametrize("options", [dict(groups=2), dict(reuse_epochs=2, reuse_minibatches=2)])
def test_grouped_and_minibatched_runs_keep_the_pairs(options):
    """groups = 2 with two actors a group, and 2 x 2 minibatched reuse passes, at B = 4, three process() calls each: the
    records stay mirror images and are the model's replayed on the device's recorded actions; every loss is finite."""
    from unreal_amd.environment.environment import Environment
    name = "selfplay_options"
    conf = _register(name, **dict(SHORT, max_episode_steps=9))
    try:
        Bn, T = 4, 5
        net, applier, tr = _build_options(name, Bn, T, 50, **options)
        Bg = Bn // tr.groups
        assert tr.selfplay and Bg % 2 == 0
        seats = _seats(conf, Bn, tr.seed, n_frames=0)
        n_term = [0]
        fill, roll = tr._fill_group, tr.compute_gradients

        def play(b0, rows):
            for acts in rows:                                      # rows of the group's Bg actions
                full = np.zeros(Bn, np.int64)
                full[b0:b0 + Bg] = acts
                active = np.zeros(Bn, np.int32)
                active[b0:b0 + Bg] = 1
                for b, (r, t, pc, stepped) in enumerate(SM.step_pairs(seats, full, active)):
                    if stepped and t:
                        n_term[0] += 1
                        seats[b].reset()

        def filling():
            fill()
            play(tr.group * Bg, [tr.actions[:Bg].cpu().numpy()])

        def rolling():
            roll()
            acts = tr.actions.cpu().numpy().reshape(T, Bg)
            n = tr.n_steps.cpu().numpy()
            assert (n[0::2] == n[1::2]).all()
            for j in range(0, Bg, 2):                              # a pair leaves the rollout together
                b0 = tr.group * Bg + j
                for t in range(n[j]):
                    full, active = np.zeros(Bn, np.int64), np.zeros(Bn, np.int32)
                    full[b0:b0 + 2], active[b0:b0 + 2] = acts[t, j:j + 2], 1
                    for b, (r, term, pc, stepped) in enumerate(SM.step_pairs(seats, full, active)):
                        if stepped and term:
                            assert t == n[j] - 1
                            n_term[0] += 1
                            seats[b].reset()
        tr._fill_group, tr.compute_gradients = filling, rolling
        while not tr._full:
            tr.process(None, 0)
        for s in seats:                                            # the trainer resets every actor when the replay is full
            s.reset()
        np.testing.assert_array_equal(_mirrored(tr.full_environment), [s.record() for s in seats])
        for call in range(3):
            steps, _ = tr.process(None, call * 40)
            assert 0 < steps <= Bn * T
            l = tr.last_losses
            assert all(np.isfinite(v) for v in l.values()), l
            np.testing.assert_array_equal(_mirrored(tr.full_environment), [s.record() for s in seats])
            np.testing.assert_array_equal(tr.full_ring.ep_steps.cpu().numpy(), [s.ep_steps for s in seats])
        assert n_term[0] > 0 and bool(torch.isfinite(net.params.flat).all())
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


# ---- 8. evaluation -------------------------------------------------------------------------------------------------------------
EVAL = dict(points=2, paddle_width=24, ball_speed=4, serve_wait=1, opponent_speed=1, win_reward=3, lose_reward=-1,
            max_episode_steps=40)


def _eval_net(name, seed=31):
    cfg = _cfg(True, False, 40, 20)
    net, _, _, _ = _build(cfg, 2, seed=seed, env_type="arcade", env_name=name)
    return net


def test_evaluate_on_a_selfplay_name_plays_the_scripted_opponent():
    from unreal_amd.environment.environment import Environment
    from unreal_amd.evaluate import Evaluate
    name = "selfplay_eval"
    conf = _register(name, **EVAL)
    Environment.register_arcade_config(name + "_duel", game="duel", opponent_width=EVAL["paddle_width"], **EVAL)
    try:
        net = _eval_net(name)
        res = Evaluate(net, batch_size=32, device=DEV, seed=0x5EED, arcade=name).process(0, one_episode_per_actor=True)
        want = Evaluate(net, batch_size=32, device=DEV, seed=0x5EED, arcade=name + "_duel").process(
            0, one_episode_per_actor=True)
        assert res == want and "versus" not in res and res["episodes"] == 32
        assert res["points_won_per_episode"] + res["points_lost_per_episode"] > 0
        env = Environment.create_environment("arcade", name)       # the batch-1 surface: seat 0 against the script
        assert env._env.config is conf.scripted and len(env._env.arcade) == 2
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)
        Environment.ARCADE_CONFIG.pop(name + "_duel", None)


def test_evaluate_versus_plays_two_networks_head_to_head():
    from unreal_amd.environment.environment import Environment
    from unreal_amd.evaluate import Evaluate
    name = "selfplay_versus"
    _register(name, **EVAL)
    try:
        net = _eval_net(name)
        other = _eval_net(name, seed=32)                           # another policy
        B = 16
        mine = np.array([(b % 2) == ((b // 2) % 2) for b in range(B)])
        results = []
        for _ in range(2):
            ev = Evaluate(net, batch_size=B, device=DEV, seed=0x5EED, arcade=name, versus=other)
            assert len(ev.env.arcade) == 3
            res = ev.process(12)
            rec = _mirrored(ev.env)
            results.append((res, rec))
        assert results[0][0] == results[1][0] and (results[0][1] == results[1][1]).all()      # deterministic
        res, rec = results[0]
        assert res["versus"] is True and res["episodes"] >= 12
        assert sorted(res) == sorted(("episodes", "success_rate", "mean_return", "return_std", "mean_length", "timeouts",
                                      "losses", "points_won_per_episode", "points_lost_per_episode", "versus"))
        n = res["episodes"]
        assert round(res["success_rate"] * n) + res["losses"] + res["timeouts"] == n
        # the points of the counted episodes: the totals' gain on `network`'s rows less the running episodes' scores
        assert round(res["points_won_per_episode"] * n) == int((rec[mine, 10] - rec[mine, 7]).sum())
        assert round(res["points_lost_per_episode"] * n) == int((rec[mine, 11] - rec[mine, 8]).sum())
        assert rec[mine, 10].sum() + rec[mine, 11].sum() > 0
        # a copy of the network on the other side, greedy play: every pair's seats stay mirror images
        ev = Evaluate(net, batch_size=B, device=DEV, seed=1, greedy=True, arcade=name, versus=_eval_net(name))
        res = ev.process(8)
        _mirrored(ev.env)
        assert res["versus"] is True and round(res["success_rate"] * res["episodes"]) + res["losses"] + res["timeouts"] == \
            res["episodes"]
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)
