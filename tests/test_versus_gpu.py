"""The versus step of the device arcade (csrc/arcade.hip): one learner per game, the other paddle an input.  Bit
for bit against the host model of tests/selfplay_model.py (learner b is HostSeat 2 (base + b), the opponent's view HostSeat
2 (base + b) + 1) and against the self-play entries on the device: resets, the four random traces, the fused entries against
the two-launch path, the time-limit forms, views and an odd actor_base, inert blocks; then the trainer's opponent pool."""
import numpy as np
import pytest
import torch

try:
    import selfplay_model as SM
    from test_arcade_gpu import _check_state, ARRAYS
    from test_fp_maze_gpu import _current_frames, _rollout_state
    from test_selfplay_gpu import _sp, _env, _seats, SHORT, TL
except ImportError:            # imported as tests.<module>
    from tests import selfplay_model as SM
    from tests.test_arcade_gpu import _check_state, ARRAYS
    from tests.test_fp_maze_gpu import _current_frames, _rollout_state
    from tests.test_selfplay_gpu import _sp, _env, _seats, SHORT, TL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB, PC = 21168, 400
OPP = ("actions", "frames", "last_action", "last_reward")


def _venv(B, H, conf, seed=0, **kw):
    """A versus environment in the state its constructor leaves (episode 0), over zeroed ring memory."""
    env = _env(B, H, conf, seed=seed, versus=True, **kw)
    assert len(env.arcade) == 4 and env.arcade[2] == "versus" and env.arcade[3] is env.opponent
    return env


def _games(conf, B, seed, actor_base=0, n_frames=None):
    """Both seats of the games [actor_base, actor_base + B): 2 B HostSeats, seat 0 of game b at index 2 b."""
    return _seats(conf, 2 * B, seed, 2 * actor_base, None if n_frames is None else 2 * n_frames)


def _pair_acts(acts, opp, active=None):
    """Learner and opponent actions per game -> the interleaved rows SM.step_pairs takes."""
    B = len(acts)
    both = np.zeros(2 * B, np.int32)
    both[0::2], both[1::2] = acts, opp
    return both, None if active is None else np.repeat(np.asarray(active), 2)


def _check_opponent(env, seats, what, n_frames=None):
    o = env.opponent
    np.testing.assert_array_equal(o.last_action.cpu().numpy(), [s.last_action for s in seats[1::2]], err_msg=what)
    np.testing.assert_array_equal(o.last_reward.cpu().numpy(), np.array([s.last_reward for s in seats[1::2]], np.float32),
                                  err_msg=what)
    got = o.frames.view(-1, FB).cpu().numpy()
    for b in range(env.B if n_frames is None else min(n_frames, env.B)):
        assert (got[b] == seats[2 * b + 1].frame.reshape(-1)).all(), "%s: the opponent's frame of game %d differs" % (what, b)


# ---- 1. resets ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 64])
def test_reset_matches_the_host_model(B):
    conf = _sp(paddle_width=8)
    env = _venv(B, 3, conf, seed=7)
    seats = _games(conf, B, 7)
    _check_state(env, seats[0::2], "reset", count=np.zeros(B, np.int32))
    _check_opponent(env, seats, "reset")
    rec = env.current_records()
    assert (rec[:, 2] == 0).all() and (rec[:, [0, 6]] == 38).all()


def test_masked_reset_over_sentinels_touches_the_masked_games_only():
    B = 9
    conf = _sp(paddle_speed=5)
    env = _venv(B, 3, conf, seed=2)
    seats = _games(conf, B, 2)
    rs = np.random.RandomState(0)
    for _ in range(12):                                # serve and fly a little: the records are no reset records
        acts, opp = rs.randint(0, 4, B).astype(np.int32), rs.randint(0, 4, B).astype(np.int32)
        env.opponent.actions.copy_(torch.from_numpy(opp))
        env.process(torch.from_numpy(acts).to(DEV), None, None, None)
        SM.step_pairs(seats, _pair_acts(acts, opp)[0])
    _check_state(env, seats[0::2], "before the reset")
    _check_opponent(env, seats, "before the reset")
    before = env.current_records()
    env.ring.frames.fill_(0xAB)
    env.opponent.frames.fill_(0xAB)
    env.opponent.last_action.fill_(-5); env.opponent.last_reward.fill_(-5.5); env.opponent.actions.fill_(-5)
    env.ring.last_action.fill_(-6)
    mask = np.array([1, 0, 0, 1, 1, 0, 0, 0, 1], np.int32)
    env.reset(torch.from_numpy(mask).to(DEV))
    m = mask.astype(bool)
    for b in np.flatnonzero(m):
        seats[2 * b].reset(); seats[2 * b + 1].reset()
    rec, frames = env.current_records(), _current_frames(env.ring)
    opp_frames = env.opponent.frames.view(B, FB).cpu().numpy()
    for b in range(B):
        np.testing.assert_array_equal(rec[b], seats[2 * b].record())
        if m[b]:
            np.testing.assert_array_equal(frames[b], seats[2 * b].frame.reshape(-1))
            np.testing.assert_array_equal(opp_frames[b], seats[2 * b + 1].frame.reshape(-1))
        else:
            assert (frames[b] == 0xAB).all() and (opp_frames[b] == 0xAB).all() and (rec[b] == before[b]).all()
    np.testing.assert_array_equal(env.opponent.last_action.cpu().numpy(), np.where(m, 0, -5))
    np.testing.assert_array_equal(env.opponent.last_reward.cpu().numpy(), np.where(m, 0, -5.5).astype(np.float32))
    np.testing.assert_array_equal(env.ring.last_action.cpu().numpy(), np.where(m, 0, -6))
    assert (env.opponent.actions == -5).all()
    np.testing.assert_array_equal(env.ring.episode.cpu().numpy(), [s.episode for s in seats[0::2]])
    idx = env.ring.cur_idx().long().cpu().numpy()      # every slot but the reset games' current ones is untouched
    others = np.ones(B * env.ring.H1, bool)
    others[idx[m]] = False
    assert (env.ring.frames.view(-1, FB).cpu().numpy()[others] == 0xAB).all()


# ---- 2. traces -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(SM.TRACE_SETTINGS)))
def test_random_steps_match_the_host_model_and_the_selfplay_entries(k):
    """The 300 steps of self-play trace k as 32 versus games: the learners play the trace's even columns, the opponents its
    odd ones, a game is active when both seats of the pair are.  Every step compares the learners with HostSeat 2 i, the
    opponent's words with HostSeat 2 i + 1, and everything with a 64-seat self-play environment stepped on the same trace:
    the versus ring of game i is the self-play ring of actor 2 i, opp_frames[i] actor 2 i + 1's current frame."""
    conf = _sp(**SM.TRACE_SETTINGS[k])
    B, H = SM.TRACE_B // 2, 3
    H1 = H + 1
    nf = SM.TRACE_PAIR_FRAMES
    acts, active = SM.trace_inputs(k)
    env = _venv(B, H, conf, seed=SM.TRACE_SEED)
    pairs = _env(2 * B, H, conf, seed=SM.TRACE_SEED)
    ring = env.ring
    seats = _games(conf, B, SM.TRACE_SEED, n_frames=nf)
    f32 = lambda n: torch.zeros(n, dtype=torch.float32, device=DEV)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)
    out_r, out_t, sp_r, sp_t = f32(B), i32(B), f32(2 * B), i32(2 * B)
    count, prev_term = np.zeros(B, np.int64), np.zeros(B, bool)
    n_idle = 0
    for s in range(SM.TRACE_STEPS):
        both = active[s][0::2] & active[s][1::2]
        out_r.fill_(-7.5); out_t.fill_(-7); sp_r.fill_(-7.5); sp_t.fill_(-7)
        env.opponent.actions.copy_(torch.from_numpy(acts[s][1::2].copy()))
        env.process(torch.from_numpy(acts[s][0::2].copy()).to(DEV), torch.from_numpy(both.copy()).to(DEV), out_r, out_t,
                    reset_on_terminal=True)
        pairs.process(torch.from_numpy(acts[s]).to(DEV), torch.from_numpy(active[s]).to(DEV), sp_r, sp_t,
                      reset_on_terminal=True)
        want_r, want_t = np.full(B, -7.5, np.float32), np.full(B, -7, np.int32)
        pcs = {}
        out = SM.step_pairs(seats, acts[s], active[s])
        for i in range(B):
            r, t, pc, stepped = out[2 * i]
            if not stepped:
                n_idle += 1
                continue
            want_r[i], want_t[i] = r, int(t)
            if i < nf:
                pcs[i] = (i * H1 + count[i] % H1, pc)
            if not (t and count[i] > 0 and prev_term[i]):
                count[i] += 1
            prev_term[i] = t
            if t:
                seats[2 * i].reset(); seats[2 * i + 1].reset()
        what = "trace %d step %d" % (k, s)
        np.testing.assert_array_equal(out_r.cpu().numpy(), want_r, err_msg=what)
        np.testing.assert_array_equal(out_t.cpu().numpy(), want_t, err_msg=what)
        _check_state(env, seats[0::2], what, count=count)
        _check_opponent(env, seats, what, n_frames=nf)
        r_pc = ring.r_pc.view(-1, PC)
        for i, (slot, pc) in pcs.items():
            np.testing.assert_array_equal(r_pc[slot].cpu().numpy(), pc.reshape(-1), err_msg="%s game %d" % (what, i))
        # the self-play entries on the device
        assert torch.equal(out_r, sp_r[0::2]) and torch.equal(out_t, sp_t[0::2]), what
        if s % 25 == 24 or s == SM.TRACE_STEPS - 1:    # (whole-ring comparisons: every 25th step covers every slot's history)
            for name in ARRAYS:
                a, p = getattr(ring, name), getattr(pairs.ring, name)
                per = a.numel() // B
                assert torch.equal(a.view(B, per), p.view(2 * B, per)[0::2]), (what, name)
            cur = pairs.ring.frames.view(-1, FB)[pairs.ring.cur_idx().long()]
            assert torch.equal(env.opponent.frames.view(B, FB), cur[1::2]), what
            assert torch.equal(env.opponent.last_action, pairs.ring.last_action[1::2]), what
            assert torch.equal(env.opponent.last_reward, pairs.ring.last_reward[1::2]), what
    assert n_idle > 0 and int(ring.episode.max()) > 0


# ---- 3. fused entries ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tl", [False, True])
@pytest.mark.parametrize("B", [3, 64])
def test_fused_policy_steps_are_the_two_launch_path(B, tl):
    """policy_rollout_step == policy_step + rollout_step, bit for bit: actions, pi, V, ring (with the final observations),
    records, the next step's rows and the opponent's three arrays."""
    from unreal_amd import ops
    H, A, xld = 4, 4, 264
    rs = np.random.RandomState(B)
    dev = lambda a, dt: torch.from_numpy(np.asarray(a)).to(DEV, dt)
    Wp = dev(rs.uniform(-.3, .3, 256 * A), torch.float32); bp = dev(rs.uniform(-.1, .1, A), torch.float32)
    Wv = dev(rs.uniform(-.3, .3, 256), torch.float32); bv = dev(rs.uniform(-.1, .1, 1), torch.float32)
    net = type("Net", (), {"p": dict(W_base_fc_p=Wp, b_base_fc_p=bp, W_base_fc_v=Wv, b_base_fc_v=bv)})
    conf = _sp(**TL)
    envs = [_venv(B, H, conf, seed=9, final_obs=tl) for _ in range(2)]
    assert (envs[0].ring.final_obs is not None) == tl
    st = [_rollout_state(B, xld) for _ in envs]
    flags, n_rew = set(), set()
    for step in range(60 if B == 3 else 30):
        X = dev(rs.uniform(-1, 1, (B, 256)), torch.float32).view(-1)
        u = dev(rs.uniform(0, 1, B), torch.float64)
        opp = dev(rs.randint(0, 4, B), torch.int32)
        for k, (e, s) in enumerate(zip(envs, st)):
            e.opponent.actions.copy_(opp)
            nxt = dict(next_idx=s["idx"], next_lar=s["lar"], lar_ld=xld, lar_col0=256, A=A)
            if k == 0:
                ops.policy_step(B, A, X, 256, Wp, bp, Wv, bv, u, s["pi"], s["v"], s["a"])
                e.rollout_step(s["a"], s["r"], s["t"], s["active"], s["log"], s["n"], s["te"], **nxt)
            else:
                e.policy_rollout_step(net, X, 256, u, s["pi"], s["v"], s["a"], s["r"], s["t"], s["active"], s["log"],
                                      s["n"], s["te"], **nxt)
        for name in ARRAYS:
            assert torch.equal(getattr(envs[0].ring, name), getattr(envs[1].ring, name)), (step, name)
        for name in OPP:
            assert torch.equal(getattr(envs[0].opponent, name), getattr(envs[1].opponent, name)), (step, name)
        for key in ("active", "log", "n", "te", "a", "pi", "v", "idx", "lar"):
            assert torch.equal(st[0][key], st[1][key]), (step, key)
        live = st[0]["log"].bool()
        for key in ("r", "t"):
            assert torch.equal(st[0][key][live], st[1][key][live]), (step, key)
        flags |= set(st[1]["te"].cpu().numpy().tolist())
        n_rew |= set(st[1]["r"][live].cpu().numpy().tolist())
        if step % 10 == 9:
            for s in st:
                s["active"].fill_(1); s["te"].zero_(); s["n"].zero_()
    if B == 64:                                        # (three games alone need not end every way in 60 steps)
        assert flags == ({0, 1, 2} if tl else {0, 1}), flags
        assert 0.0 in n_rew and n_rew & {-3.0, 7.0}, n_rew     # (a match of 11 steps at the most: the serve decides who scores)
    assert flags & {1, 2}, flags
    assert int(envs[0].ring.episode.max()) > 0


# ---- 4. time limits ------------------------------------------------------------------------------------------------------------
def test_time_limits_flag_two_keep_the_learners_final_observation_and_the_opponent_sees_the_next_match():
    """The _tl rollout step at an 11-step limit: a match cut by the limit is flagged 2 and keeps the learner's final
    observation, byte for byte the model's; a match point in the last allowed step is flagged 1 and stores nothing; after
    either, opp_frames holds the next match's first frame; an idle actor's opponent words stay."""
    B, H = 9, 3
    conf = _sp(**TL)
    env = _venv(B, H, conf, seed=3, final_obs=True)
    ring = env.ring
    seats = _games(conf, B, 3)
    st = _rollout_state(B, 264)
    rs = np.random.RandomState(4)
    fin_want = np.full((B, FB), 0xCD, np.uint8)
    ring.final_obs.fill_(0xCD)
    kinds = {"cut": 0, "last": 0, "early": 0}
    first = seats[1].frame.copy()                      # a reset record's view from seat 1
    for step in range(70):
        acts, opp = rs.randint(0, 4, B).astype(np.int32), rs.randint(0, 4, B).astype(np.int32)
        st["active"].fill_(1); st["te"].zero_()
        idle = step % 7 == 3
        if idle:                                       # game 0 sits this step out
            st["active"][0] = 0
            keep = [getattr(env.opponent, n).clone() for n in OPP[1:]]
        st["r"].fill_(-7.5); st["t"].fill_(-7)
        env.opponent.actions.copy_(torch.from_numpy(opp))
        env.rollout_step(torch.from_numpy(acts).to(DEV), st["r"], st["t"], st["active"], st["log"], st["n"], st["te"],
                         next_idx=st["idx"])
        both, active = _pair_acts(acts, opp, [0 if idle and b == 0 else 1 for b in range(B)])
        out = SM.step_pairs(seats, both, active)
        want_t = np.zeros(B, np.int32)
        for b in range(B):
            r, t, pc, stepped = out[2 * b]
            if stepped and t:
                g = seats[2 * b].game
                cut = not g.ended()
                want_t[b] = 2 if cut else 1
                kinds["cut" if cut else "last" if g.ep_steps == conf.max_episode_steps else "early"] += 1
                if cut:
                    fin_want[b] = seats[2 * b].frame.reshape(-1)
                seats[2 * b].reset(); seats[2 * b + 1].reset()
                np.testing.assert_array_equal(seats[2 * b + 1].frame, first)
        what = "step %d" % step
        live = np.array([o[3] for o in out[0::2]])
        np.testing.assert_array_equal(st["t"].cpu().numpy()[live], want_t[live], err_msg=what)
        np.testing.assert_array_equal(st["te"].cpu().numpy(), want_t, err_msg=what)
        np.testing.assert_array_equal(st["r"].cpu().numpy()[live], [o[0] for o in out[0::2] if o[3]], err_msg=what)
        _check_state(env, seats[0::2], what)
        _check_opponent(env, seats, what)
        if idle:
            for n, t in zip(OPP[1:], keep):
                per = t.numel() // B
                assert torch.equal(getattr(env.opponent, n)[:per], t[:per]), (what, n)
        np.testing.assert_array_equal(ring.final_obs.view(B, FB).cpu().numpy(), fin_want, err_msg=what)
    assert min(kinds.values()) > 0, kinds


# ---- 5. views, actor_base ------------------------------------------------------------------------------------------------------
def test_views_and_an_odd_actor_base_step_the_same_games():
    """Six games as one environment, as the views [0, 1), [1, 4), [4, 6) of one, and as environments of 1 and 5 games with
    actor_base 0 and 1; against each other and the model."""
    B, H = 6, 3
    conf = _sp(**SHORT)
    whole, viewed = _venv(B, H, conf, seed=5), _venv(B, H, conf, seed=5)
    bases = (0, 1)
    parts = [_venv(n, H, conf, seed=5, actor_base=b0, actors_total=B) for b0, n in zip(bases, (1, 5))]
    assert parts[1].arcade[1] == 1
    cuts = ((0, 1), (1, 4), (4, B))
    views = [viewed.view(*c) for c in cuts]
    assert views[1].arcade[1] == 1 and views[1].B == 3 and views[1].opponent.frames.numel() == 3 * FB
    rs = np.random.RandomState(3)
    z = lambda dt: torch.zeros(B, dtype=dt, device=DEV)
    outs = [(z(torch.float32), z(torch.int32)) for _ in range(3)]
    seats = _games(conf, B, 5)
    for step in range(60):
        acts_h, opp_h = rs.randint(0, 4, B).astype(np.int32), rs.randint(0, 4, B).astype(np.int32)
        acts, opp = torch.from_numpy(acts_h).to(DEV), torch.from_numpy(opp_h).to(DEV)
        whole.opponent.actions.copy_(opp); viewed.opponent.actions.copy_(opp)
        whole.process(acts, None, *outs[0], track_score=True)
        for v, (b0, b1) in zip(views, cuts):
            v.process(acts[b0:b1], None, outs[1][0][b0:b1], outs[1][1][b0:b1], track_score=True)
        for e, b0 in zip(parts, bases):
            e.opponent.actions.copy_(opp[b0:b0 + e.B])
            e.process(acts[b0:b0 + e.B], None, outs[2][0][b0:b0 + e.B], outs[2][1][b0:b0 + e.B], track_score=True)
        for name in ARRAYS:
            a = getattr(whole.ring, name)
            assert torch.equal(a, getattr(viewed.ring, name)), (step, name)
            assert torch.equal(a, torch.cat([getattr(e.ring, name) for e in parts])), (step, name)
        for name in OPP:
            a = getattr(whole.opponent, name)
            assert torch.equal(a, getattr(viewed.opponent, name)), (step, name)
            assert torch.equal(a, torch.cat([getattr(e.opponent, name) for e in parts])), (step, name)
        for o in outs[1:]:
            assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]), step
        for b, (r, t, pc, _) in enumerate(SM.step_pairs(seats, _pair_acts(acts_h, opp_h)[0])):
            if t:
                seats[b].reset()
    assert int(whole.ring.episode.min()) > 0
    _check_state(whole, seats[0::2], "the whole environment against the model")
    _check_opponent(whole, seats, "the whole environment against the model")


# ---- 6. inert blocks -----------------------------------------------------------------------------------------------------------
def test_a_block_of_another_game_is_inert_and_other_configs_are_refused():
    from unreal_amd import ops
    from unreal_amd.environment.arcade_environment import BatchedArcadeEnvironment, ArcadeConfig
    B = 5
    env = _venv(B, 2, _sp(), seed=1)
    ring, o = env.ring, env.opponent
    z = lambda n, dt, v: torch.full((n,), v, dtype=dt, device=DEV)
    for game in (1, 5, 4, 2, 0, -3):                                             # Breakout's, invaders', no game's
        other = env.arcade[0].clone()
        other[0] = game
        arcade = (other,) + env.arcade[1:]
        ring.frames.fill_(0x5A); o.frames.fill_(0x5A); o.last_action.fill_(-5); o.last_reward.fill_(-5.5)
        before = {k: getattr(ring, k).clone() for k in ARRAYS}
        st = _rollout_state(B, 264)
        outs = dict(r=z(B, torch.float32, -7.5), t=z(B, torch.int32, -7))
        ops.arcade_reset(ring, None, arcade=arcade)
        ops.arcade_step(ring, z(B, torch.int32, 1), None, outs["r"], outs["t"], arcade=arcade)
        ops.arcade_rollout_step(ring, z(B, torch.int32, 1), outs["r"], outs["t"], st["active"], st["log"], st["n"], st["te"],
                                next_idx=st["idx"], arcade=arcade)
        torch.cuda.synchronize()
        for k, t in before.items():
            assert torch.equal(getattr(ring, k), t), (game, k)
        assert (o.frames == 0x5A).all() and (o.last_action == -5).all() and (o.last_reward == -5.5).all()
        assert (outs["r"] == -7.5).all() and (outs["t"] == -7).all()
        assert (st["active"] == 1).all() and not st["log"].any() and not st["n"].any() and not st["idx"].any()
    for conf in (ArcadeConfig(game="duel"), ArcadeConfig()):
        with pytest.raises(ValueError, match="versus"):
            BatchedArcadeEnvironment(4, 2, DEV, config=conf, versus=True)


# ---- 7. the trainer's opponent pool ----------------------------------------------------------------------------------------------
def _register(name, **kw):
    from unreal_amd.environment.environment import Environment
    Environment.register_arcade_selfplay(name, **kw)
    return Environment.ARCADE_CONFIG[name]


def _build_pool(name, B, T, H, use_lstm=True, aux=True, lr=7.0711e-4, draws=None, seed=21, net_seed=4, **options):
    """A prepared trainer on the self-play game `name`, handed back before the replay fills (the caller hooks it first)."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer
    Environment.action_size = -1
    net = UnrealModel(4, 0, -1, use_lstm, aux, aux, aux, 0.05, 0.001, DEV, seed=net_seed)
    applier = RMSPropApplier(None, decay=0.99, momentum=0.0, epsilon=0.1, clip_norm=40.0, device=DEV)
    tr = Trainer(0, net, lr, None, applier, "arcade", name, use_lstm, aux, aux, aux, 0.05, 0.001, T, T, 0.99, 0.9, H,
                 10 ** 6, DEV, batch_size=B, seed=seed, draws=draws, **options)
    tr.prepare()
    return net, applier, tr


def _step_game(seats, i, a, oa):
    """One step of game i of the model with both actions (a terminal resets) -> (the learner's reward, terminal)."""
    s0, s1 = seats[2 * i], seats[2 * i + 1]
    s0.partner, s1.partner = [int(oa)], [int(a)]
    _, r, t, _ = s0.process(int(a))
    s1.process(int(oa))
    if t:
        s0.reset(); s1.reset()
    return r, t


@pytest.mark.parametrize("use_lstm,aux", [(True, True), (False, False)])
def test_process_with_a_pool_matches_oracle(use_lstm, aux):
    """Trainer(opponent_pool=2, opponent_snapshot_every=1) against OracleTrainer with one HostSeat(conf, 2 b) per actor whose
    partner is scripted from what the device recorded: the opponents' actions of the fill, tr.opponent_actions after each
    pass; rewards 7 and -3; the bars and shape of tests/test_selfplay_gpu.py's test_process_on_selfplay_matches_oracle."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.train.trainer import PhiloxDraws
    from oracle.trainer import OracleTrainer, ExplicitDraws
    try:
        from test_trainer_gpu import _cfg, _feed_draws, RecordingDraws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL
    except ImportError:
        from tests.test_trainer_gpu import _cfg, _feed_draws, RecordingDraws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL
    name = "versus_short_%d%d" % (use_lstm, aux)
    conf = _register(name, **SHORT)
    try:
        B, H, T = 4, 40, 20
        cfg = _cfg(use_lstm, aux, H, T)
        cfg["initial_learning_rate"] = 7.0711e-4
        draws = RecordingDraws(PhiloxDraws(0xA3C, 0))
        net, applier, tr = _build_pool(name, B, T, H, use_lstm, aux, draws=draws, seed=0xA3C, net_seed=3,
                                       opponent_pool=2, opponent_snapshot_every=1)
        assert tr.selfplay and tr.opponent_pool == 2 and tr.environment.opponent is not None and not net.lar_bounded
        assert tr._split is None
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = [SM.HostSeat(conf, 2 * b, tr.seed, partner=[]) for b in range(B)]
        orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=hosts)
        fill, played = tr._fill_group, []

        def filling():
            fill()
            played.append(tr.opponent_actions[:B].cpu().numpy().copy())
        tr._fill_group = filling
        while not tr._full:
            tr.process(None, 0)
        for step_u in draws.log:
            for b in range(B):
                edraws[b].action_u.append(float(step_u[b]))
        for b in range(B):
            hosts[b].partner.extend(int(row[b]) for row in played)
        orc.fill()
        assert not any(h.partner for h in hosts)
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
            n_dev = tr.n_steps.cpu().numpy()
            acts = tr.actions.cpu().numpy().reshape(T, B)
            opp = tr.opponent_actions.cpu().numpy().reshape(T, B)
            rews = tr.rewards.cpu().numpy().reshape(T, B)
            for b in range(B):
                hosts[b].partner.extend(int(a) for a in opp[:n_dev[b], b])
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
            for (pname, _), gref in zip(orc.params.items(), mean_g):     # (every figure is printed before any is judged)
                gr = gref.numpy().reshape(-1)
                err = np.abs(g_dev[pname] - gr)
                print("update %d %-16s max |error| %.3e at %d, bar %.3e, max |gradient| %.3e" % (
                    it, pname, err.max(), int(err.argmax()), GRAD_ATOL + GRAD_REL * np.abs(gr).max(), np.abs(gr).max()))
            for (pname, _), gref in zip(orc.params.items(), mean_g):
                gr = gref.numpy().reshape(-1)
                assert np.abs(g_dev[pname] - gr).max() <= GRAD_ATOL + GRAD_REL * np.abs(gr).max(), (it, pname)
            assert abs(float(tr.last_grad_norm.cpu()[0]) - norm_o) <= 1e-4 * max(1.0, norm_o)
            np.testing.assert_array_equal(tr.environment.current_records(), [h.record() for h in hosts])
        assert n_term > 0 and {7.0, -3.0} <= rewards, (n_term, rewards)
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


def _filled(name, B=4, T=5, H=12, **kw):
    net, applier, tr = _build_pool(name, B, T, H, **kw)
    while not tr._full:
        tr.process(None, 0)
    return net, applier, tr


def test_the_opponents_play_what_their_weights_say():
    """After a process() call, step 0's opponent actions recomputed from the saved opponent frames, last action / reward,
    LSTM state and uniforms with tr.opponent(k)'s own encode_rows / lstm_step / policy_step, slot by slot; the two slots
    hold different weights in the checked call (slot 0 the learner's after an update, slot 1 the initial ones)."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import PathWS
    name = "versus_weights"
    _register(name, **SHORT)
    try:
        B, K = 6, 2
        net, applier, tr = _filled(name, B=B, lr=1e-2, opponent_pool=K, opponent_snapshot_every=100)
        Bk = B // K
        first = net.params.flat.clone()
        tr.process(None, 0)
        assert tr.updates == 1 and tr.opponent_ages() == [1, 1] and not torch.equal(net.params.flat, first)
        o = tr.full_environment.opponent
        saved = {n: getattr(o, n).clone() for n in ("frames", "last_action", "last_reward")}
        c, h = tr.full_opp_c.clone(), tr.full_opp_h.clone()
        start = net.params.flat.clone()
        tr.process(None, 0)
        assert torch.equal(tr.opponent(0).params.flat, start) and torch.equal(tr.opponent(1).params.flat, first)
        assert not torch.equal(start, first)
        got = tr.opponent_actions[:B].cpu().numpy()
        for k in range(K):
            onet = tr.opponent(k)
            ring = type("R", (), {})()
            ring.frames = saved["frames"][k * Bk * FB:(k + 1) * Bk * FB].contiguous()
            ring.frame_shape, ring.frame_stride = (84, 84), FB
            ring.last_action = saved["last_action"][k * Bk:(k + 1) * Bk].contiguous()
            ring.last_reward = saved["last_reward"][k * Bk:(k + 1) * Bk].contiguous()
            ws = PathWS(Bk, Bk, DEV, save_c1=False, lstm=True, xld=onet.xld, **onet.ws_kw)
            ws.frame_idx[:Bk].copy_(torch.arange(Bk, dtype=torch.int32))
            ws.c0.copy_(c[k * Bk * 256:(k + 1) * Bk * 256]); ws.h0.copy_(h[k * Bk * 256:(k + 1) * Bk * 256])
            onet.refresh_shadows()
            onet.begin_pass()
            onet.encode_rows(ring, ws, 0, Bk, lar_from_ring=False, save_c1=False, lstm_x=False)
            onet.lstm_step(ws, 0, Bk, fused_x=True)
            feat, ld = onet.features(ws, 0)
            z = lambda n, dt: torch.zeros(n, dtype=dt, device=DEV)
            pi, v, a = z(Bk * 4, torch.float32), z(Bk, torch.float32), z(Bk, torch.int32)
            onet.policy_step(Bk, feat, ld, tr.opp_u[k * Bk:(k + 1) * Bk].contiguous(), pi, v, a)
            np.testing.assert_array_equal(a.cpu().numpy(), got[k * Bk:(k + 1) * Bk], err_msg="slot %d" % k)
            assert abs(float(pi.view(Bk, 4).sum(1).mean()) - 1.0) < 1e-5
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


def test_the_pool_follows_its_rule():
    """K = 2, N = 1, a learning rate that moves the weights.  After each of four calls slot 0 equals the learner's parameters
    at the call's start, slot 1 the learner's as the test saves them at the scheduled update (with N = 1 every call's end),
    and the two differ; inside a call, before its update, slot 0 is the learner and slot 1 the previous snapshot."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.train.trainer import Trainer
    name = "versus_rule"
    _register(name, **SHORT)
    try:
        net, applier, tr = _filled(name, lr=1e-2, opponent_pool=2, opponent_snapshot_every=1)
        initial = net.params.flat.clone()
        assert all(torch.equal(tr.opponent(k).params.flat, initial) for k in range(2)) and tr.opponent_ages() == [0, 0]
        seen = []
        roll = tr.compute_gradients

        def rolling():                                   # inside the call, before its update
            seen.append((tr.opponent(0).params.flat.clone(), tr.opponent(1).params.flat.clone()))
            roll()
        tr.compute_gradients = rolling
        scheduled = initial                              # what slot 1 holds: the weights at the last snapshot
        for call in range(4):
            start = net.params.flat.clone()
            assert Trainer.opponent_snapshot(2, 1, tr.updates + 1, tr.opponent_snapshots) == (1, call + 1)
            tr.process(None, 0)
            assert tr.updates == call + 1 and tr.opponent_snapshots == call + 1
            s0, s1 = seen[-1]
            assert torch.equal(s0, start) and torch.equal(s1, scheduled), call
            scheduled = net.params.flat.clone()                   # N = 1: the call's end takes a snapshot into slot 1
            assert torch.equal(tr.opponent(0).params.flat, start), call
            assert torch.equal(tr.opponent(1).params.flat, scheduled), call
            assert not torch.equal(tr.opponent(0).params.flat, tr.opponent(1).params.flat), call
            assert tr.opponent_ages() == [1, 0]
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


@pytest.mark.parametrize("options", [dict(groups=2), dict(reuse_epochs=2, reuse_minibatches=2)])
def test_grouped_and_minibatched_runs_with_a_pool(options):
    """groups = 2, and 2 x 2 minibatched reuse passes, at B = 4 and K = 2, three process() calls each: the records and the
    rollouts' rewards are the model's replayed on the device's recorded actions of both paddles; every loss is finite."""
    from unreal_amd.environment.environment import Environment
    name = "versus_options"
    conf = _register(name, **dict(SHORT, max_episode_steps=9))
    try:
        Bn, T = 4, 5
        net, applier, tr = _build_pool(name, Bn, T, 50, opponent_pool=2, opponent_snapshot_every=1, **options)
        Bg = Bn // tr.groups
        seats = _games(conf, Bn, tr.seed, n_frames=0)
        n_term = [0]
        fill, roll = tr._fill_group, tr.compute_gradients

        def filling():
            fill()
            a, oa = tr.actions[:Bg].cpu().numpy(), tr.opponent_actions[:Bg].cpu().numpy()
            for j in range(Bg):
                n_term[0] += _step_game(seats, tr.group * Bg + j, a[j], oa[j])[1]

        def rolling():
            roll()
            acts = tr.actions.cpu().numpy().reshape(T, Bg)
            opp = tr.opponent_actions.cpu().numpy().reshape(T, Bg)
            rews = tr.rewards.cpu().numpy().reshape(T, Bg)
            n = tr.n_steps.cpu().numpy()
            for j in range(Bg):
                for t in range(n[j]):
                    r, term = _step_game(seats, tr.group * Bg + j, acts[t, j], opp[t, j])
                    assert r == rews[t, j], (tr.group, j, t)
                    assert term == (t == n[j] - 1 and bool(tr.terminal_end.cpu()[j])), (tr.group, j, t)
                    n_term[0] += term
        tr._fill_group, tr.compute_gradients = filling, rolling
        while not tr._full:
            tr.process(None, 0)
        for s in seats:                                            # the trainer resets every actor when the replay is full
            s.reset()
        np.testing.assert_array_equal(tr.full_environment.current_records(), [s.record() for s in seats[0::2]])
        per_call = tr.groups * tr.reuse_epochs * tr.reuse_minibatches
        for call in range(3):
            steps, _ = tr.process(None, call * 40)
            assert 0 < steps <= Bn * T and tr.updates == (call + 1) * per_call
            l = tr.last_losses
            assert all(np.isfinite(v) for v in l.values()), l
            np.testing.assert_array_equal(tr.full_environment.current_records(), [s.record() for s in seats[0::2]])
            np.testing.assert_array_equal(tr.full_ring.ep_steps.cpu().numpy(), [s.ep_steps for s in seats[0::2]])
            _check_opponent(tr.full_environment, seats, "call %d" % call, n_frames=0)
        assert tr.opponent_snapshots == 3 * per_call and tr.opponent_ages() == [per_call, 0]
        assert n_term[0] > 0 and bool(torch.isfinite(net.params.flat).all())
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


def test_scores_a_checkpoint_round_trip_and_evaluate(tmp_path):
    """opponent_scores() against the record words; a checkpoint restores the pool, u, s and the slots' ages bit for bit over
    a wrecked trainer; Evaluate(net, arcade=name, versus=tr.opponent(1)) runs and its episode counts add up."""
    from unreal_amd import checkpoint
    from unreal_amd.environment.environment import Environment
    from unreal_amd.evaluate import Evaluate
    name = "versus_run"
    _register(name, **dict(SHORT, points=1))               # a match is one point: the fill and every call finish some
    try:
        B, K = 8, 4
        net, applier, tr = _filled(name, B=B, H=30, lr=1e-2, opponent_pool=K, opponent_snapshot_every=1)

        def blocks(rec):
            return [dict(slot=k, won=int(rec[2 * k:2 * k + 2, 12].sum()), lost=int(rec[2 * k:2 * k + 2, 13].sum()))
                    for k in range(K)]
        rec0 = tr.full_environment.current_records()
        assert tr.opponent_scores(reset=True) == blocks(rec0) and rec0[:, 12:14].sum() > 0   # the fill's matches
        assert tr.opponent_scores() == blocks(np.zeros_like(rec0))
        for _ in range(2):
            tr.process(None, 0)
        rec1 = tr.full_environment.current_records()
        assert tr.opponent_scores(reset=False) == blocks(rec1 - rec0) and (rec1 - rec0)[:, 12:14].sum() > 0
        assert tr.opponent_scores(reset=True) == blocks(rec1 - rec0)
        assert tr.opponent_scores() == blocks(np.zeros_like(rec0))
        state = tr.opponent_state()
        assert (state["updates"], state["snapshots"], len(state["params"])) == (2, 2, K) and tr.opponent_ages() == [1, 1, 0, 2]
        assert len({float(f.double().sum()) for f in state["params"]}) > 1   # the pool holds different networks
        want = net.params.flat.clone()
        checkpoint.save(str(tmp_path), net, applier, 80, 1.0, opponents=state)
        # wreck what the checkpoint carries, then restore it
        net.params.flat.zero_(); applier.ms.fill_(3.0)
        for k in range(K):
            tr.opponent(k).params.flat.fill_(0.5)
        tr.updates, tr.opponent_snapshots, tr._opp_taken = 99, 77, [5] * K
        assert checkpoint.restore(str(tmp_path), net, applier, opponents=tr)[0] == 80
        back = tr.opponent_state()
        assert torch.equal(net.params.flat, want)
        assert all(torch.equal(a, b) for a, b in zip(back["params"], state["params"]))
        assert (back["updates"], back["snapshots"], back["taken"]) == (state["updates"], state["snapshots"], state["taken"])
        assert tr.opponent_ages() == [1, 1, 0, 2]
        tr.process(None, 0)                                # and the restored trainer goes on
        assert tr.updates == 3 and tr.opponent_ages() == [1, 2, 1, 0]

        res = Evaluate(net, batch_size=8, device=DEV, seed=5, arcade=name, versus=tr.opponent(1)).process(6)
        n = res["episodes"]
        assert res["versus"] is True and n >= 6
        assert round(res["success_rate"] * n) + res["losses"] + res["timeouts"] == n
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


def test_two_runs_repeat_bit_for_bit_and_a_restored_run_continues_the_uninterrupted_one(tmp_path):
    """Two runs with one seed give bit-identical parameters and pools, and a run continued from a checkpoint equals the
    uninterrupted one after two more calls.  At the shape at which the trainer itself repeats bit for bit (one
    actor, the auxiliary heads off): B = 1, so K = 1, the present self alone.  Measured on this tree, three pairs of runs of
    four calls each, parameters differing in a pair: B = 1 with K = 1 (LSTM or feed-forward) 0 / 0 / 0; without a pool the
    duel at B = 2, groups = 2: 3 / 3 / 0; K = 1 at B = 2, groups = 2: 98 / 1 / 2; K = 2 at B = 4, groups = 2: 60 / 198 /
    219 -- last bits, with identical actions of both paddles in every pair (the float atomics of the weight-gradient
    kernels, with or without a pool)."""
    from unreal_amd import checkpoint
    from unreal_amd.environment.environment import Environment
    name = "versus_repeat"
    _register(name, **dict(SHORT, points=1))
    try:
        kw = dict(B=1, H=12, aux=False, lr=1e-2, opponent_pool=1, opponent_snapshot_every=1)
        snap = lambda net, tr: [net.params.flat.clone(), tr.opponent(0).params.flat.clone(), tr.full_opp_c.clone(),
                                tr.full_ring.arcade.clone(), tr.full_environment.opponent.frames.clone()]
        net, applier, tr = _filled(name, **kw)
        for _ in range(2):
            tr.process(None, 0)
        middle = snap(net, tr)
        state = tr.opponent_state()
        assert (state["updates"], state["snapshots"]) == (2, 0) and tr.opponent_ages() == [1]
        checkpoint.save(str(tmp_path), net, applier, 80, 1.0, opponents=state)
        for _ in range(2):
            tr.process(None, 0)
        final = snap(net, tr)
        assert not torch.equal(final[0], middle[0]) and torch.equal(final[1], tr.opponent(0).params.flat)

        net2, applier2, tr2 = _filled(name, **kw)                     # the same run again, to the checkpoint's call
        for _ in range(2):
            tr2.process(None, 0)
        for a, b in zip(middle, snap(net2, tr2)):
            assert torch.equal(a, b)
        net2.params.flat.zero_(); applier2.ms.fill_(3.0); tr2.opponent(0).params.flat.fill_(0.5)
        tr2.updates, tr2.opponent_snapshots = 99, 77
        assert checkpoint.restore(str(tmp_path), net2, applier2, opponents=tr2)[0] == 80
        assert (tr2.updates, tr2.opponent_snapshots) == (2, 0)
        for _ in range(2):
            tr2.process(None, 0)
        for a, b in zip(final, snap(net2, tr2)):
            assert torch.equal(a, b)
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)
