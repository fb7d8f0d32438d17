"""Game mixtures on the device (csrc/arcade.hip): one config block per actor, global actor g on task g mod K.
Everything rests on one property: actor g of a mixture plays what actor g of a single-game environment of its task with the
same seed plays, so the host model is one existing game model per actor (tests/mix_model.py).  The tasks are the three
games' short settings with max_episode_steps 30 / 20 / 25 and action_repeat 1 / 4 / 2 (tests/mix_model.py says why the four
ticks are the duel's); tests/test_arcade_mix_cpu.py shows on the models alone that every task of every trace below ends
episodes both by the game and by its own step limit."""
import numpy as np
import pytest
import torch

try:
    import mix_model as MM
    from test_trainer_gpu import _cfg, _build, _feed_draws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL
    from test_maze_config_gpu import RING_ARRAYS
    from test_fp_maze_gpu import _current_frames, _rollout_state
except ImportError:            # imported as tests.<module>
    from tests import mix_model as MM
    from tests.test_trainer_gpu import _cfg, _build, _feed_draws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL
    from tests.test_maze_config_gpu import RING_ARRAYS
    from tests.test_fp_maze_gpu import _current_frames, _rollout_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB, PC = 21168, 400
A, XLD = 4, 264
SENTINEL = 0xAB
ARRAYS = RING_ARRAYS + ("ep_steps", "episode", "arcade")
STATS = ("done_return", "done_episodes")


def _dev(a, dt):
    return torch.from_numpy(np.array(a)).to(DEV, dt)           # (a copy: the shared traces are read-only)


def _env(B, H, conf, seed=0, **kw):
    """Frames zeroed (torch.empty: slots no step has written would hold stale allocator bytes), the final-observation
    slots at a sentinel, episode 1 (the constructor's reset and this one), as the models of MM.simulate."""
    from unreal_amd.environment.arcade_environment import BatchedArcadeEnvironment
    env = BatchedArcadeEnvironment(B, H, DEV, config=conf, seed=seed, **kw)
    env.ring.frames.zero_()
    env.ring.r_pc.zero_()
    if env.ring.final_obs is not None:
        env.ring.final_obs.fill_(SENTINEL)
    env.reset()
    return env


def _hosts(mix, B, seed, actor_base=0):
    models = MM.host_batch(mix, B, seed, actor_base=actor_base)
    for m in models:
        m.reset()
    return models


def _policy(rs):
    Wp = _dev(rs.uniform(-.3, .3, 256 * A), torch.float32); bp = _dev(rs.uniform(-.1, .1, A), torch.float32)
    Wv = _dev(rs.uniform(-.3, .3, 256), torch.float32); bv = _dev(rs.uniform(-.1, .1, 1), torch.float32)
    return type("Net", (), {"p": dict(W_base_fc_p=Wp, b_base_fc_p=bp, W_base_fc_v=Wv, b_base_fc_v=bv)})


def _same_rings(a, b, what, names=ARRAYS):
    for name in names:
        assert torch.equal(getattr(a.ring, name), getattr(b.ring, name)), (what, name)


# ---- 1. K = 1 is the plain path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["step", "rollout", "policy", "rollout_tl", "policy_tl"])
@pytest.mark.parametrize("game", range(3))
def test_one_task_is_the_plain_entry_bit_for_bit(game, form):
    """The same config, seed and random inputs through the plain entries and through the _mix entries with one block: 40
    steps of 5 actors under an `active` mask, a masked reset on the way; every ring array, record and frame (the
    final-observation store with them), and every rollout word."""
    from unreal_amd import ops
    from unreal_amd.environment.arcade_environment import ArcadeConfig, ArcadeMix
    B, H = 5, 3
    conf = ArcadeConfig(**MM.MIX3[game])
    tl = form.endswith("_tl")
    envs = [_env(B, H, c, seed=11, final_obs=tl) for c in (conf, ArcadeMix([conf]))]
    assert len(envs[0].arcade) == 2 and envs[1].arcade[2] == 1 and envs[0].ring.done_return is None
    called = []
    inner = ops._call
    try:
        ops._call = lambda name, *a: (called.append(name), inner(name, *a))[1]
        _same_rings(*envs, "reset")
        rs = np.random.RandomState(100 * game + len(form))
        net = _policy(rs)
        st = [_rollout_state(B, XLD) for _ in envs]
        n_term = 0
        for step in range(40):
            acts = _dev(rs.randint(0, 4, B).astype(np.int32), torch.int32)
            mask = _dev((rs.rand(B) < 0.8).astype(np.int32), torch.int32)
            X = _dev(rs.uniform(-1, 1, B * 256).astype(np.float32), torch.float32)
            u = _dev(rs.uniform(0, 1, B), torch.float64)
            for e, s in zip(envs, st):
                nxt = dict(next_idx=s["idx"], next_lar=s["lar"], lar_ld=XLD, lar_col0=256, A=A)
                if step == 36:
                    e.reset(mask)
                if form == "step":
                    e.process(acts, mask, s["r"], s["t"], reset_on_terminal=True, track_score=True)
                    continue
                s["active"].copy_(mask); s["te"].zero_(); s["n"].zero_()
                if form.startswith("rollout"):
                    e.rollout_step(acts, s["r"], s["t"], s["active"], s["log"], s["n"], s["te"], **nxt)
                else:
                    e.policy_rollout_step(net, X, 256, u, s["pi"], s["v"], s["a"], s["r"], s["t"], s["active"], s["log"],
                                          s["n"], s["te"], **nxt)
            _same_rings(*envs, step)
            for key in st[0]:
                assert torch.equal(st[0][key], st[1][key]), (step, key)
            n_term += int((st[0]["t"] != 0).sum())
        assert n_term > 0 and int(envs[0].ring.episode.max()) > 1
        assert int(envs[1].ring.done_episodes.sum()) > 0           # (the one task's statistics are kept as any task's)
    finally:
        ops._call = inner
    arcade_calls = [n for n in called if n.startswith("unreal_arcade")]
    assert any("_mix" in n for n in arcade_calls) and any("_mix" not in n for n in arcade_calls)
    assert {n.replace("_mix", "") for n in arcade_calls if "_mix" in n} == {n for n in arcade_calls if "_mix" not in n}


# ---- 2. traces against the models -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(MM.TRACE_CASES)))
def test_traces_match_one_model_per_actor(case):
    """120 random steps under an `active` mask with resets on terminal: K = 3 at 3, 7 and 64 actors, K = 16 at 19."""
    tr = MM.run_trace(case)
    mix, B = MM.trace_mix(case), MM.TRACE_CASES[case][1]
    F, H1 = tr["frames"].shape[1], MM.TRACE_H1
    env = _env(B, H1 - 1, mix, seed=MM.TRACE_SEEDS[case][0])
    ring = env.ring
    np.testing.assert_array_equal(env.task_of_actor(), np.arange(B) % len(mix))
    out_r = torch.zeros(B, dtype=torch.float32, device=DEV)
    out_t = torch.zeros(B, dtype=torch.int32, device=DEV)
    for s in range(MM.TRACE_STEPS):
        out_r.fill_(-7.5); out_t.fill_(-7)
        env.process(_dev(tr["acts"][s], torch.int32), _dev(tr["active"][s], torch.int32), out_r, out_t,
                    reset_on_terminal=True, track_score=True)
        what = "step %d" % s
        np.testing.assert_array_equal(out_r.cpu().numpy(), tr["reward"][s], err_msg=what)
        np.testing.assert_array_equal(out_t.cpu().numpy(), tr["terminal"][s], err_msg=what)
        rec = env.current_records()
        bad = np.flatnonzero((rec != tr["records"][s]).any(1))
        assert not len(bad), "%s: records of actors %s differ: %s, want %s" % (what, bad[:8], rec[bad[0]], tr["records"][s][bad[0]])
        for name, got in (("count", ring.count), ("ep_steps", ring.ep_steps), ("episode", ring.episode),
                          ("last_action", ring.last_action), ("last_reward", ring.last_reward)):
            np.testing.assert_array_equal(got.cpu().numpy(), tr[name][s], err_msg="%s %s" % (what, name))
        frames = _current_frames(ring)[:F]
        bad = np.flatnonzero((frames != tr["frames"][s]).any(1))
        assert not len(bad), "%s: frames of actors %s differ" % (what, bad[:8])
        r_pc = ring.r_pc.view(-1, PC).cpu().numpy()
        for b in range(F):
            if tr["pc_slot"][s, b] >= 0:
                np.testing.assert_array_equal(r_pc[tr["pc_slot"][s, b]], tr["pc"][s, b], err_msg="%s actor %d" % (what, b))
    np.testing.assert_array_equal(ring.done_return.cpu().numpy().astype(np.float64), tr["done_return"])
    np.testing.assert_array_equal(ring.done_episodes.cpu().numpy(), tr["done_episodes"])


# ---- 3. masked reset ------------------------------------------------------------------------------------------------------------
def test_masked_reset_over_sentinel_slots():
    B, seed = 8, 2
    mix = MM.make_mix(MM.MIX3)
    env = _env(B, 3, mix, seed=seed)
    models = _hosts(mix, B, seed)
    rs = np.random.RandomState(0)
    for _ in range(12):                                # serve and fly a little: the records are no reset records
        acts = rs.randint(0, 4, B).astype(np.int32)
        env.process(_dev(acts, torch.int32), None, None, None, reset_on_terminal=False)
        for m, a in zip(models, acts):
            m.process(a)
    before = env.current_records()
    np.testing.assert_array_equal(before, [m.record() for m in models])
    env.ring.frames.fill_(SENTINEL)
    mask = np.array([1, 0, 1, 0, 1, 1, 0, 0], np.int32)           # every task reset on one actor and kept on another
    env.reset(_dev(mask, torch.int32))
    for m, k in zip(models, mask):
        if k:
            m.reset()
    rec, frames = env.current_records(), _current_frames(env.ring)
    for b, m in enumerate(models):
        np.testing.assert_array_equal(rec[b], m.record())
        if mask[b]:
            np.testing.assert_array_equal(frames[b], m.frame.reshape(-1))
        else:
            assert (frames[b] == SENTINEL).all() and (rec[b] == before[b]).all()
    np.testing.assert_array_equal(env.ring.episode.cpu().numpy(), [m.episode for m in models])
    np.testing.assert_array_equal(env.ring.ep_steps.cpu().numpy(), [m.ep_steps for m in models])
    idx = env.ring.cur_idx().long().cpu().numpy()
    others = np.ones(B * env.ring.H1, bool)
    others[idx] = False
    assert (env.ring.frames.view(-1, FB).cpu().numpy()[others] == SENTINEL).all()


# ---- 4. views and actor_base ------------------------------------------------------------------------------------------------------
def test_views_and_actor_base_step_the_same_actors():
    """Eight actors of a five-task mixture as one environment, as the views [0, 3) + [3, 8) of one, and as two environments
    with actor_base 0 and 3: the second view's first actor is task 3.  Identical, and the models'."""
    from unreal_amd.environment.arcade_environment import BatchedArcadeEnvironment
    B, H, cut, seed = 8, 3, 3, 5
    mix = MM.make_mix(MM.MIX16[:5])
    whole, viewed = _env(B, H, mix, seed=seed), _env(B, H, mix, seed=seed)
    parts = [_env(n, H, mix, seed=seed, actor_base=b0, actors_total=B) for b0, n in ((0, cut), (cut, B - cut))]
    views = [viewed.view(0, cut), viewed.view(cut, B)]
    assert isinstance(views[1], BatchedArcadeEnvironment) and views[1].arcade[1:] == (cut, 5) and views[1].base_actor == cut
    np.testing.assert_array_equal(views[1].task_of_actor(), [3, 4, 0, 1, 2])
    np.testing.assert_array_equal(parts[1].task_of_actor(), [3, 4, 0, 1, 2])
    models = _hosts(mix, B, seed)
    rs = np.random.RandomState(3)
    z = lambda dt: torch.zeros(B, dtype=dt, device=DEV)
    outs = [(z(torch.float32), z(torch.int32)) for _ in range(3)]
    spans = ((0, cut), (cut, B))
    n_term = np.zeros(5, np.int64)
    for step in range(60):
        a = rs.randint(0, 4, B).astype(np.int32)
        acts = _dev(a, torch.int32)
        whole.process(acts, None, *outs[0], track_score=True)
        for v, (b0, b1) in zip(views, spans):
            v.process(acts[b0:b1], None, outs[1][0][b0:b1], outs[1][1][b0:b1], track_score=True)
        for e, (b0, b1) in zip(parts, spans):
            e.process(acts[b0:b1], None, outs[2][0][b0:b1], outs[2][1][b0:b1], track_score=True)
        for name in ARRAYS + STATS:
            w = getattr(whole.ring, name)
            assert torch.equal(w, getattr(viewed.ring, name)), (step, name)
            assert torch.equal(w, torch.cat([getattr(e.ring, name) for e in parts])), (step, name)
        for o in outs[1:]:
            assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]), step
        want_r, want_t = [], []
        for b, m in enumerate(models):
            _, r, t, _ = m.process(a[b])
            want_r.append(r); want_t.append(int(t))
            if t:
                n_term[b % 5] += 1
                m.reset()
        np.testing.assert_array_equal(outs[0][0].cpu().numpy(), np.array(want_r, np.float32), err_msg=str(step))
        np.testing.assert_array_equal(outs[0][1].cpu().numpy(), want_t, err_msg=str(step))
        np.testing.assert_array_equal(whole.current_records(), [m.record() for m in models], err_msg=str(step))
    assert (n_term > 0).all(), n_term
    np.testing.assert_array_equal(whole.ring.done_episodes.cpu().numpy(), [m.episode - 1 for m in models])


# ---- 5. fused forms -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tl", [False, True])
def test_fused_rollout_steps_are_the_two_launch_paths(tl):
    """On two views of each environment (index_parent; the second starts at task 1): rollout_step == process +
    rollout_advance (+ cur_idx and the LSTM-input columns), and policy_rollout_step == policy_step + rollout_step, bit for
    bit, statistics included.  With a final-observation store there is no two-launch step form: the two _tl forms against
    each other, and everything but the flags against the forms without the store."""
    from unreal_amd import ops
    B, H, cut, K = 8, 4, 4, 3
    mix = MM.make_mix(MM.MIX3)
    rs = np.random.RandomState(17)
    net = _policy(rs)
    p = net.p
    kinds = ("rollout", "policy") if tl else ("process", "rollout", "policy")
    envs = [_env(B, H, mix, seed=9, final_obs=tl) for _ in kinds]
    spans = ((0, cut), (cut, B))
    views = [[e.view(*sp) for sp in spans] for e in envs]
    st = [_rollout_state(B, XLD) for _ in envs]
    n_term, flags = np.zeros(K, np.int64), set()
    for step in range(90):
        X = _dev(rs.uniform(-1, 1, B * 256).astype(np.float32), torch.float32)
        u = _dev(rs.uniform(0, 1, B), torch.float64)
        for kind, vs, s in zip(kinds, views, st):
            for v, (b0, b1) in zip(vs, spans):
                sl = {n: t[b0:b1] for n, t in s.items() if n not in ("pi", "lar")}
                pi, lar = s["pi"][A * b0:A * b1], s["lar"][b0 * XLD:b1 * XLD]
                nxt = dict(next_idx=sl["idx"], next_lar=lar, lar_ld=XLD, lar_col0=256, A=A)
                if kind != "policy":
                    ops.policy_step(b1 - b0, A, X[b0 * 256:], 256, p["W_base_fc_p"], p["b_base_fc_p"], p["W_base_fc_v"],
                                    p["b_base_fc_v"], u[b0:b1], pi, sl["v"], sl["a"])
                if kind == "process":
                    v.process(sl["a"], sl["active"].clone(), sl["r"], sl["t"], reset_on_terminal=True, track_score=True)
                    ops.rollout_advance(b1 - b0, sl["t"], sl["active"], sl["log"], sl["n"], sl["te"])
                    v.ring.cur_idx(out=sl["idx"], base_actor=b0)
                elif kind == "rollout":
                    v.rollout_step(sl["a"], sl["r"], sl["t"], sl["active"], sl["log"], sl["n"], sl["te"], index_parent=True,
                                   **nxt)
                else:
                    v.policy_rollout_step(net, X[b0 * 256:b1 * 256], 256, u[b0:b1], pi, sl["v"], sl["a"], sl["r"], sl["t"],
                                          sl["active"], sl["log"], sl["n"], sl["te"], index_parent=True, **nxt)
        for e in envs[1:]:
            _same_rings(envs[0], e, step, ARRAYS + STATS)
        live = st[0]["log"].bool()
        for s in st[1:]:
            for key in ("active", "log", "n", "te", "a", "pi", "v", "idx"):
                assert torch.equal(st[0][key], s[key]), (step, key)
            for key in ("r", "t"):
                assert torch.equal(st[0][key][live], s[key][live]), (step, key)
        assert torch.equal(st[-2]["lar"], st[-1]["lar"]), step
        te = st[0]["te"].cpu().numpy()
        for b in np.flatnonzero(te):
            n_term[b % K] += 1
        flags |= set(te.tolist())
        if step % 10 == 9:
            for s in st:
                s["active"].fill_(1); s["te"].zero_(); s["n"].zero_()
    assert (n_term > 0).all(), n_term
    assert flags == ({0, 1, 2} if tl else {0, 1}), flags


def test_tl_forms_cut_every_task_at_its_own_limit():
    """Trace 1 (K = 3, 7 actors) through the _tl rollout entries on two views, the trace's `active` mask as the rollout's
    own: an episode cut by its task's limit is flagged 2 and leaves the model's frame in final_obs, one the game ends is
    flagged 1 and leaves the store alone.  The policy form (a head that draws the scripted action) does the same."""
    case = 1
    tr = MM.run_trace(case)
    mix, B = MM.trace_mix(case), MM.TRACE_CASES[case][1]
    cut = 4
    spans = ((0, cut), (cut, B))
    Wp = np.zeros((256, A), np.float32)
    Wp[np.arange(A), np.arange(A)] = 100.0
    net = type("Net", (), {"p": dict(W_base_fc_p=_dev(Wp.reshape(-1), torch.float32), b_base_fc_p=torch.zeros(A, device=DEV),
                                     W_base_fc_v=torch.zeros(256, device=DEV), b_base_fc_v=torch.zeros(1, device=DEV))})
    u = torch.full((B,), 0.5, dtype=torch.float64, device=DEV)
    for fused in (False, True):
        env = _env(B, MM.TRACE_H1 - 1, mix, seed=MM.TRACE_SEEDS[case][0], final_obs=True)
        views = [env.view(*sp) for sp in spans]
        st = _rollout_state(B, XLD)
        want_final = np.full((B, FB), SENTINEL, np.uint8)
        seen = set()
        for s in range(MM.TRACE_STEPS):
            st["active"].copy_(_dev(tr["active"][s], torch.int32)); st["te"].zero_(); st["n"].zero_()
            st["t"].fill_(-7); st["r"].fill_(-7.5)
            X = np.zeros((B, 256), np.float32)
            X[np.arange(B), tr["acts"][s]] = 1.0
            X = _dev(X.reshape(-1), torch.float32)
            for v, (b0, b1) in zip(views, spans):
                sl = {n: t[b0:b1] for n, t in st.items() if n not in ("pi", "lar")}
                if fused:
                    v.policy_rollout_step(net, X[b0 * 256:b1 * 256], 256, u[b0:b1], st["pi"][A * b0:A * b1], sl["v"], sl["a"],
                                          sl["r"], sl["t"], sl["active"], sl["log"], sl["n"], sl["te"], index_parent=True)
                else:
                    sl["a"].copy_(_dev(tr["acts"][s][b0:b1], torch.int32))
                    v.rollout_step(sl["a"], sl["r"], sl["t"], sl["active"], sl["log"], sl["n"], sl["te"], index_parent=True)
            what = "fused %s step %d" % (fused, s)
            flags = tr["flags"][s]
            np.testing.assert_array_equal(st["t"].cpu().numpy(), flags, err_msg=what)
            np.testing.assert_array_equal(st["te"].cpu().numpy(), np.maximum(flags, 0), err_msg=what)
            np.testing.assert_array_equal(st["r"].cpu().numpy(), tr["reward"][s], err_msg=what)
            np.testing.assert_array_equal(env.current_records(), tr["records"][s], err_msg=what)
            for b in range(B):
                if (s, b) in tr["final"]:
                    want_final[b] = tr["final"][(s, b)]
                if flags[b] > 0:
                    seen.add((b % len(mix), int(flags[b])))
            got = env.ring.final_obs.view(B, FB).cpu().numpy()
            bad = np.flatnonzero((got != want_final).any(1))
            assert not len(bad), "%s: final-observation slots of actors %s differ" % (what, bad)
        assert seen == {(k, f) for k in range(len(mix)) for f in (1, 2)}, seen
        np.testing.assert_array_equal(env.ring.done_return.cpu().numpy().astype(np.float64), tr["done_return"])
        np.testing.assert_array_equal(env.ring.done_episodes.cpu().numpy(), tr["done_episodes"])


# ---- 6. an unknown game id in one block ---------------------------------------------------------------------------------------------
def test_an_unknown_game_in_one_block_stops_only_its_actors():
    """Block 1 of three names no game: through every entry the actors of task 1 write nothing, not even the statistics;
    the actors of the other blocks step and match their models."""
    from unreal_amd import ops
    case = 1
    tr = MM.run_trace(case)
    mix, B = MM.trace_mix(case), MM.TRACE_CASES[case][1]
    from unreal_amd.environment.arcade_environment import BatchedArcadeEnvironment
    env = BatchedArcadeEnvironment(B, MM.TRACE_H1 - 1, DEV, config=mix, seed=MM.TRACE_SEEDS[case][0])     # episode 0
    ring = env.ring
    block = env.arcade[0].clone()
    block[24] = 2
    broken = (block, 0, 3)
    dead = np.arange(B) % 3 == 1
    ring.frames.zero_()
    ring.r_pc.zero_()
    ring.frames.view(B, -1)[_dev(dead, torch.bool)] = 0x5A
    per_actor = {n: getattr(ring, n).clone().view(B, -1) for n in ARRAYS + STATS}
    ops.arcade_reset(ring, None, arcade=broken)                    # the sound blocks: episode 1, as the trace
    st = _rollout_state(B, XLD)
    st["t"].fill_(-7); st["r"].fill_(-7.5)
    for s in range(30):
        acts, active = _dev(tr["acts"][s], torch.int32), _dev(tr["active"][s], torch.int32)
        if s % 2:
            st["active"].copy_(active); st["te"].zero_(); st["n"].zero_(); st["log"].fill_(-3); st["idx"].fill_(-3)
            ops.arcade_rollout_step(ring, acts, st["r"], st["t"], st["active"], st["log"], st["n"], st["te"],
                                    next_idx=st["idx"], arcade=broken)
            assert (st["log"].cpu().numpy()[dead] == -3).all() and (st["idx"].cpu().numpy()[dead] == -3).all()
            assert (st["log"].cpu().numpy()[~dead] == tr["active"][s][~dead]).all()
        else:
            ops.arcade_step(ring, acts, active, st["r"], st["t"], reset_on_terminal=True, track_score=True, arcade=broken)
        what = "step %d" % s
        live = ~dead & (tr["active"][s] != 0)
        np.testing.assert_array_equal(st["r"].cpu().numpy()[live], tr["reward"][s][live], err_msg=what)
        np.testing.assert_array_equal(st["t"].cpu().numpy()[live], tr["terminal"][s][live], err_msg=what)
        assert (st["r"].cpu().numpy()[dead] == -7.5).all() and (st["t"].cpu().numpy()[dead] == -7).all(), what
        np.testing.assert_array_equal(env.current_records()[~dead], tr["records"][s][~dead], err_msg=what)
        np.testing.assert_array_equal(_current_frames(ring)[~dead], tr["frames"][s][~dead], err_msg=what)
    torch.cuda.synchronize()
    for n, t in per_actor.items():
        now = getattr(ring, n).view(B, -1)
        assert torch.equal(now[_dev(dead, torch.bool)], t[_dev(dead, torch.bool)]), n
    assert (ring.count.cpu().numpy()[dead] == 0).all() and (ring.episode.cpu().numpy()[dead] == 0).all()
    assert int(ring.done_episodes.cpu().numpy()[~dead].sum()) > 0


# ---- 7. the trainer against the oracle ---------------------------------------------------------------------------------------------
def _register_mix(name, settings=MM.MIX3):
    from unreal_amd.environment.environment import Environment
    Environment.register_arcade_mix(name, [dict(s) for s in settings])
    return Environment.ARCADE_CONFIG[name]


@pytest.mark.parametrize("use_lstm,aux", [(True, True), (False, False)])
def test_process_on_a_mixture_matches_oracle(use_lstm, aux):
    """Trainer.process against OracleTrainer with one host model per actor, every actor another game, as
    tests/test_arcade_gpu.py's test_process_on_the_arcade_matches_oracle and at its bars."""
    from unreal_amd.environment.environment import Environment
    from oracle.trainer import OracleTrainer, ExplicitDraws
    name = "mix_short_%d%d" % (use_lstm, aux)
    mix = _register_mix(name)
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(use_lstm, aux, H, T)
        cfg["initial_learning_rate"] = 7.0711e-4
        net, applier, tr, draws = _build(cfg, B, seed=3, env_type="arcade", env_name=name)
        assert tr.action_size == 4 and not net.lar_bounded and tr.rp_mode == 0 and tr.objective_size == 0
        assert tr.environment.config is mix and tr.environment.arcade[2] == 3
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = MM.host_batch(mix, B, seed=tr.seed)
        orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=hosts)
        while not tr._full:
            tr.process(None, 0)
        for step_u in draws.log:
            for b in range(B):
                edraws[b].action_u.append(float(step_u[b]))
        orc.fill()
        np.testing.assert_array_equal(tr.ring.count.cpu().numpy(), [a.exp.count for a in orc.actors])
        np.testing.assert_array_equal(tr.environment.current_records(), [h.record() for h in hosts])
        n_term = 0
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
        assert n_term > 0
        scores = tr.task_scores()
        assert [s["game"] for s in scores] == ["breakout", "duel", "invaders"] and sum(s["episodes"] for s in scores) == n_term
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


def test_grouped_process_on_a_mixture_is_the_reference_algorithm():
    """groups = B: one process() call = B sequential single-actor passes, each a one-actor view whose task is its global
    index, against OracleTrainer.process_async (tests/test_arcade_gpu.py's grouped test, at its bars)."""
    from unreal_amd.environment.environment import Environment
    from oracle.trainer import OracleTrainer, ExplicitDraws
    name = "mix_short_grouped"
    mix = _register_mix(name)
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(True, True, H, T)
        cfg["initial_learning_rate"] = 7.0711e-4
        net, applier, tr, draws = _build(cfg, B, seed=13, env_type="arcade", env_name=name, groups=B)
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = MM.host_batch(mix, B, seed=tr.seed)
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
        assert sum(s["episodes"] for s in tr.task_scores()) == n_scores
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


# ---- 8. Evaluate ---------------------------------------------------------------------------------------------------------------------
def test_evaluate_reports_every_task():
    """Evaluate(arcade=mixture), 12 actors, one episode per actor: every step's reward and terminal are the models'
    replaying the device's actions, and the overall keys and every task's keys are the models' first-episode statistics."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.evaluate import Evaluate
    name = "mix_eval"
    mix = _register_mix(name)
    try:
        cfg = _cfg(True, False, 40, 20)
        net, _, _, _ = _build(cfg, 1, seed=31, env_type="arcade", env_name=name)
        B, seed, K = 12, 0x5EED, 3
        ev = Evaluate(net, batch_size=B, device=DEV, seed=seed, arcade=name)
        assert not net.lar_bounded
        log = []
        inner = ev.env.process

        def recording(actions, active, out_reward, out_terminal, **kw):
            inner(actions, active, out_reward, out_terminal, **kw)
            log.append((actions.cpu().numpy().copy(), out_reward.cpu().numpy().copy(), out_terminal.cpu().numpy().copy()))
        ev.env.process = recording
        res = ev.process(0, one_episode_per_actor=True)
        hosts = MM.host_batch(mix, B, seed=seed)
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
                        first[b] = (ret[b], h.ep_steps, h.totals[0] - start[b][0], h.totals[1] - start[b][1],
                                    bool(h.success))
                    ret[b], start[b] = 0, list(h.totals)
                    h.reset()
        assert None not in first

        def stats(conf, eps):
            col = lambda i: np.array([e[i] for e in eps], np.float64)
            n = len(eps)
            want = dict(episodes=n, success_rate=col(4).mean(), mean_return=col(0).mean(), return_std=col(0).std(),
                        mean_length=col(1).mean())
            if conf is None:
                return want
            if conf.game == "duel":
                losses = sum(1 for e in eps if not e[4] and e[3] >= conf.points)
                want.update(timeouts=n - int(col(4).sum()) - losses, losses=losses, points_won_per_episode=col(2).mean(),
                            points_lost_per_episode=col(3).mean())
            else:
                first_key = "aliens_per_episode" if conf.game == "invaders" else "bricks_per_episode"
                want.update({"timeouts": n - int(col(4).sum()), first_key: col(2).mean(), "lives_lost_per_episode": col(3).mean()})
            return want

        def same(got, want, what):
            assert set(got) == set(want), (what, sorted(got), sorted(want))
            for key, v in want.items():
                assert abs(got[key] - v) < 1e-9, (what, key, got[key], v)

        tasks = [stats(conf, [first[b] for b in range(B) if b % K == k]) for k, conf in enumerate(mix.tasks)]
        overall = dict(stats(None, first), timeouts=sum(t["timeouts"] for t in tasks))
        assert len(res["tasks"]) == K
        same({k: v for k, v in res.items() if k != "tasks"}, overall, "overall")
        for k in range(K):
            assert res["tasks"][k]["episodes"] == 4
            same(res["tasks"][k], tasks[k], "task %d" % k)
        assert len({f[1] for f in first}) > 2, first
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


# ---- 9. training options ----------------------------------------------------------------------------------------------------------
def _build_options(env_name, Bn, T, Hn, groups=1, adam=None, aux=True, **options):
    """tests/test_minibatch_gpu.py's trainer, handed back before the replay fills (the caller hooks it first)."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.train.adam_applier import AdamApplier
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer
    Environment.action_size = -1
    net = UnrealModel(Environment.get_action_size("arcade", env_name), 0, -1, True, aux, aux, aux, 0.05, 0.001, DEV, seed=4)
    applier = AdamApplier(None, device=DEV, **adam) if adam is not None else \
        RMSPropApplier(None, decay=0.99, momentum=0.0, epsilon=0.1, clip_norm=40.0, device=DEV)
    tr = Trainer(0, net, 7.0711e-4, None, applier, "arcade", env_name, True, aux, aux, aux, 0.05, 0.001, T, T, 0.99, 0.9, Hn,
                 10 ** 6, DEV, batch_size=Bn, groups=groups, seed=21, **options)
    tr.prepare()
    return net, applier, tr


def test_training_options_on_a_mixture():
    """Full UNREAL on 8 actors of a three-task mixture with groups = 2, reuse_epochs = 2, reuse_minibatches = 2, Adam, the
    exploration bonus, GAE(0.95) and time-limit bootstrapping, three calls: finite losses and parameters, 8 updates a
    call, env steps the rollouts' own count, the records those of the models fed the logged actions, and task_scores()
    the models' finished episodes."""
    from unreal_amd.environment.environment import Environment
    name = "mix_options"
    mix = _register_mix(name, tuple(dict(s, max_episode_steps=m) for s, m in zip(MM.MIX3, (9, 7, 8))))
    try:
        G, E, M, Bn, T, K = 2, 2, 2, 8, 5, 3
        adam = dict(beta1=0.9, beta2=0.999, epsilon=1e-8, weight_decay=0.01, clip_norm=40.0)
        net, applier, tr = _build_options(name, Bn, T, 50, groups=G, adam=adam, reuse_epochs=E, reuse_minibatches=M,
                                          explore_beta=0.0625, gae_lambda=0.95, bootstrap_timeouts=True)
        Bg = Bn // G
        assert tr.full_ring.final_obs is not None and tr.full_ring.done_return is not None
        hosts = MM.host_batch(mix, Bn, seed=tr.seed)
        ret = np.zeros(Bn, np.int64)
        done = [[] for _ in range(K)]                              # per task: the returns of the episodes the rollouts finished
        rolled, n_term = [], [0]
        fill, roll = tr._fill_group, tr.compute_gradients

        def filling():
            fill()
            acts = tr.actions[:Bg].cpu().numpy()
            for j in range(Bg):
                h = hosts[tr.group * Bg + j]
                if h.process(acts[j])[2]:
                    h.reset()

        def rolling():
            roll()
            acts = tr.actions.cpu().numpy().reshape(T, Bg)
            n = tr.n_steps.cpu().numpy()
            for j in range(Bg):
                b = tr.group * Bg + j
                for t in range(n[j]):
                    _, r, term, _ = hosts[b].process(acts[t, j])
                    ret[b] += r
                    if term:
                        assert t == n[j] - 1
                        done[b % K].append(int(ret[b]))
                        ret[b] = 0
                        n_term[0] += 1
                        hosts[b].reset()
            rolled.append(int(n.sum()))
        tr._fill_group, tr.compute_gradients = filling, rolling
        while not tr._full:
            tr.process(None, 0)
        for h in hosts:                                            # the trainer resets every actor when the replay is full
            h.reset()
        np.testing.assert_array_equal(tr.full_environment.current_records(), [h.record() for h in hosts])
        assert not tr.full_ring.done_episodes.any()                # the fill tracks no score
        for call in range(3):
            del rolled[:]
            steps, _ = tr.process(None, call * 40)
            assert len(rolled) == G and steps == sum(rolled) and 0 < steps <= Bn * T, (steps, rolled)
            l = tr.last_losses
            assert all(np.isfinite(v) for v in l.values()), l
            assert l["updates"] == 8 and applier.t == (call + 1) * 8
            np.testing.assert_array_equal(tr.full_environment.current_records(), [h.record() for h in hosts])
        assert bool(torch.isfinite(net.params.flat).all()) and bool(torch.isfinite(applier.m).all())
        scores = tr.task_scores(reset=False)
        assert len(scores) == K and [s["game"] for s in scores] == ["breakout", "duel", "invaders"]
        assert [s["name"] for s in scores] == list(mix.task_names)
        assert sum(s["episodes"] for s in scores) == n_term[0] > 0
        for k, s in enumerate(scores):
            assert s["episodes"] == len(done[k]) > 0, (k, s, done)
            assert s["mean_return"] == sum(done[k]) / float(len(done[k])), (k, s, done[k])
        assert tr.task_scores() == scores                          # ... and zeroed by the read that asks for it
        assert all(s["episodes"] == 0 and s["mean_return"] is None for s in tr.task_scores())
    finally:
        Environment.ARCADE_CONFIG.pop(name, None)


# ---- 10. the option off -----------------------------------------------------------------------------------------------------------
def test_a_single_game_calls_no_mix_entry():
    """A trainer on a plain arcade config allocates no statistics and launches no _mix entry, and its parameters after two
    calls at one actor repeat bit for bit (the same trainer built twice, as tests/test_minibatch_gpu.py compares runs)."""
    from unreal_amd import ops
    from unreal_amd.environment.environment import Environment
    name = "mix_off"
    Environment.register_arcade_config(name, **dict(MM.MIX3[0], max_episode_steps=9))
    called = []
    inner = ops._call
    try:
        ops._call = lambda n, *a: (called.append(n), inner(n, *a))[1]
        flats = []
        for _ in range(3):                                         # (the first run only warms the process up)
            net, applier, tr = _build_options(name, 1, 5, 16, aux=False)
            while not tr._full:
                tr.process(None, 0)
            assert tr.full_ring.done_return is None and tr.full_ring.done_episodes is None
            assert len(tr.environment.arcade) == 2
            with pytest.raises(ValueError, match="mixture"):
                tr.task_scores()
            for it in range(2):
                steps, _ = tr.process(None, 0)
                assert steps > 0
            flats.append(net.params.flat.cpu().numpy().copy())
            del net, applier, tr
        np.testing.assert_array_equal(flats[1].view(np.uint32), flats[2].view(np.uint32))
    finally:
        ops._call = inner
        Environment.ARCADE_CONFIG.pop(name, None)
    arcade = {n for n in called if n.startswith("unreal_arcade")}
    assert arcade and not any("_mix" in n for n in arcade), arcade
