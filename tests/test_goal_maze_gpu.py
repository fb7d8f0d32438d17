"""Goal-sense first-person mazes on the device (maze.hip, a block with flag 64), bit for bit against the host
model of tests/goal_maze_model.py: the breadth-first search at every reset, record words 5..7, the shaped reward, the
objective launch, the fused paths on views, OracleTrainer, Evaluate and the batch-1 environment."""
import numpy as np
import pytest
import torch

try:
    import maze_model as MM
    import goal_maze_model as GOAL
except ImportError:            # imported as tests.<module>
    from tests import maze_model as MM
    from tests import goal_maze_model as GOAL
try:
    from test_maze_config_gpu import RING_ARRAYS, CFG_ARRAYS
    from test_fp_maze_gpu import _env, _current_frames, _rollout_state
    # the bars, room and rewards of the navigation process tests
    from test_nav_maze_gpu import (_cfg, _build, _feed_draws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL, NAV_ROOM, NAV_KW,
                                   _register)
except ImportError:
    from tests.test_maze_config_gpu import RING_ARRAYS, CFG_ARRAYS
    from tests.test_fp_maze_gpu import _env, _current_frames, _rollout_state
    from tests.test_nav_maze_gpu import (_cfg, _build, _feed_draws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL, NAV_ROOM,
                                         NAV_KW, _register)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB, PC = 21168, 400
SIZES = (7, 12, 14, 21)
STYLES = [(200, 100, 50, 0xAA), (0, 255, 0, 0x00), (10, 20, 250, 0x0F)]
APPLES = {7: 6, 12: 20, 14: 30, 21: 64}
SENTINEL = -7.5


def _static(N, L=7, seed=0, apples=True, **kw):
    from unreal_amd.environment.maze_environment import MazeConfig
    rs = np.random.RandomState(seed + N)
    marks = kw.pop("marks", "") + ("A" * APPLES[N] if apples else "")
    return MazeConfig([MM.random_layout(N, rs, marks=marks) for _ in range(L)], view="first_person", **kw)


def _generated(N, styled=False, **kw):
    from unreal_amd.environment.maze_environment import MazeConfig
    if styled:
        kw = dict(kw, wall_styles=STYLES, gen_landmark_density=64)
    return MazeConfig(None, random_start=True, random_goal=True, view="first_person", generate=N, **kw)


def _hosts(cfg, B, seed, frames=True):
    """Host models of an environment built by _env: its constructor and _env each reset once (episode 1)."""
    models = GOAL.host_batch(cfg, B, seed=seed, frames=frames)
    for m in models:
        m.reset()
    return models


def _records(ring):
    return ring.actor_records.cpu().numpy()


def _objectives(ring):
    return ring.r_objective.cpu().numpy().reshape(ring.B, ring.H1, 3)


def _check_state(env, models, what, count=None):
    """Count, cells, headings, goals, episode counters, last action / reward, the whole per-actor record (words 5..7 and
    the distance field with it), current_distances() and, unless the models render none, the current frames."""
    ring, B = env.ring, len(models)
    if count is not None:
        np.testing.assert_array_equal(ring.count.cpu().numpy(), count, err_msg=what)
    rec = _records(ring)
    want = np.stack([m.actor_record() for m in models])
    assert rec.shape == want.shape == (B, env.config.record_words), (rec.shape, want.shape)
    bad = np.flatnonzero((rec != want).any(1))
    assert not len(bad), "%s: records of actors %s differ (first words %s)" % (
        what, bad[:8], np.flatnonzero(rec[bad[0]] != want[bad[0]])[:8])
    np.testing.assert_array_equal(env.current_distances(), np.stack([m.distance_field() for m in models]), err_msg=what)
    np.testing.assert_array_equal(ring.pos.cpu().numpy().reshape(B, 2), [(m.x, m.y) for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.heading.cpu().numpy(), [m.h for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.goal.cpu().numpy().reshape(B, 2), [(m.gx, m.gy) for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.ep_steps.cpu().numpy(), [m.ep_steps for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.episode.cpu().numpy(), [m.episode for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.last_action.cpu().numpy(), [m.last_action for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.last_reward.cpu().numpy(), np.array([m.last_reward for m in models], np.float32),
                                  err_msg=what)
    if models[0].frames:
        got = _current_frames(ring)
        want = np.stack([m.frame.reshape(-1) for m in models])
        bad = np.flatnonzero((got != want).any(1))
        assert not len(bad), "%s: frames of actors %s differ" % (what, bad[:8])


def _check_current_objective(ring, models, what, others=None):
    """The slot count % H1 of every actor holds its model's objective; `others`: what every other slot must hold."""
    obj = _objectives(ring)
    slot = ring.count.cpu().numpy() % ring.H1
    want = np.stack([m.objective() for m in models]).astype(np.float32)
    np.testing.assert_array_equal(obj[np.arange(ring.B), slot], want, err_msg=what)
    if others is not None:
        rest = np.ones(obj.shape[:2], dtype=bool)
        rest[np.arange(ring.B), slot] = False
        assert (obj[rest] == others).all(), what


# ---- 1. reset ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["static", "generated"])
@pytest.mark.parametrize("N,B", [(N, B) for N in SIZES for B in (3, 64)])
def test_reset_fields_and_objectives_match_the_host_model(N, B, kind):
    """Static (7 layouts, random start and goal) and generated + styled: the first frames, record words 5..7, the whole
    distance field and r_objective at slot count % H1 are the model's, at counts that use every slot; then a masked reset:
    the other actors' records keep their fields, and no slot but the current ones is written."""
    seed = 0x60A1 + N + B
    if kind == "static":
        cfg = _static(N, L=7, seed=B, random_start=True, random_goal=True, show_goal=True, goal_sense=True,
                      progress_reward=1)
    else:
        cfg = _generated(N, styled=True, gen_loops=2, gen_apples=5, show_goal=True, goal_sense=True)
    env = _env(B, 2, cfg, seed=seed)
    ring = env.ring
    assert ring.objective_size == 3 and env.objective_size == 3 and ring.record_words == cfg.record_words
    models = _hosts(cfg, B, seed)
    _check_state(env, models, "reset")
    _check_current_objective(ring, models, "reset")
    count = (np.arange(B) % 5).astype(np.int32)              # slots 0, 1, 2 of H1 = 3
    ring.count.copy_(torch.from_numpy(count))
    ring.r_objective.fill_(SENTINEL)
    env.reset()
    for m in models:
        m.reset()
    _check_state(env, models, "second reset", count)
    _check_current_objective(ring, models, "second reset", others=SENTINEL)
    assert all(m.distance() >= 1 for m in models) and len(set(m.distance() for m in models)) > 1
    mask = np.random.RandomState(B).uniform(size=B) < 0.5
    before = _records(ring).copy()
    ring.r_objective.fill_(SENTINEL)
    env.reset(torch.from_numpy(mask.astype(np.int32)).to(DEV))
    for b in np.flatnonzero(mask):
        models[b].reset()
    np.testing.assert_array_equal(_records(ring)[~mask], before[~mask])
    _check_state(env, models, "masked reset", count)
    _check_current_objective(ring, models, "masked reset", others=SENTINEL)


# ---- 2. the long case ------------------------------------------------------------------------------------------------------
def test_serpentine_field_and_progress_rewards():
    """N = 21, one corridor of 240 moves from S to G (more than a byte holds; the search runs 241 passes), heading along
    it, progress_reward 2: the field is the model's, and 30 steps forward and back pay +2 and -2."""
    from unreal_amd.environment.maze_environment import MazeConfig
    B = 3
    cfg = MazeConfig([GOAL.serpentine_layout(21)], view="first_person", start_heading=0, goal_sense=True,
                     progress_reward=2, hit_reward=-5)
    env = _env(B, 3, cfg, seed=1)
    models = _hosts(cfg, B, 1)
    _check_state(env, models, "reset")
    field = env.current_distances()
    assert field.dtype == np.uint16 and field.shape == (B, 21, 21)
    assert field[0, 0, 0] == 240 and field[0, 20, 20] == 0 and field[0, 1, 0] == GOAL.NO_PATH
    assert list(_records(env.ring)[0, 5:8]) == [20, 20, 240]
    out_r = torch.zeros(B, dtype=torch.float32, device=DEV)
    out_t = torch.zeros(B, dtype=torch.int32, device=DEV)
    plan = [2] * 10 + [3] * 5 + [2] * 10 + [3] * 5               # cells 0 -> 10 -> 5 -> 15 -> 10 of the first row
    for step, a in enumerate(plan):
        env.process(torch.full((B,), a, dtype=torch.int32, device=DEV), None, out_r, out_t)
        for m in models:
            _, r, t, _ = m.process(a)
            assert r == (2 if a == 2 else -2) and not t
        assert out_r.cpu().tolist() == [2.0 if a == 2 else -2.0] * B and not out_t.any(), step
        _check_current_objective(env.ring, models, "step %d" % step)
    _check_state(env, models, "after the walk")
    assert list(_records(env.ring)[0, 5:8]) == [10, 20, 230]


# ---- 3. random steps -------------------------------------------------------------------------------------------------------
# (N, kind, action set, goal_respawn, progress_reward)
STEP_CASES = [(7, "static", "lab", True, 3), (7, "generated", "turn", False, 0), (21, "static", "turn", False, 3),
              (21, "generated", "lab", True, 3)]


@pytest.mark.parametrize("N,kind,action_set,respawn,p", STEP_CASES)
def test_random_steps_match_the_host_model(N, kind, action_set, respawn, p):
    """200 actors (static: over 7 layouts), a step limit of 23, 120 random actions under an `active` mask, a masked
    reset half way: rewards, terminals, cells, records (with the field, so every reset's search is checked) and the
    objective of the committed and of the new slot at every step.  Goals, time-outs, resets and distances rising and
    falling all happen.  (The frames of these blocks are compared at the resets above, against the same block without
    the option below and through the oracle; here the models render none, which keeps the case to a few seconds.)"""
    B, H, steps, seed = 200, 3, 120, 0x60A2 + N
    H1 = H + 1
    kw = dict(show_goal=True, max_episode_steps=23, goal_reward=10, apple_reward=1, hit_reward=-2, goal_respawn=respawn,
              action_set=action_set, goal_sense=True, progress_reward=p)
    if kind == "static":
        cfg = _static(N, L=7, seed=N, random_start=True, random_goal=True, **kw)
    else:
        cfg = _generated(N, styled=N == 21, gen_loops=3, gen_apples=APPLES[N] // 2, **kw)
    A = cfg.action_size
    env = _env(B, H, cfg, seed=seed)
    ring = env.ring
    models = _hosts(cfg, B, seed, frames=False)
    if kind == "static":
        assert len(set(ring.layout.cpu().numpy())) == 7
    rs = np.random.RandomState(N)
    out_r = torch.zeros(B, dtype=torch.float32, device=DEV)
    out_t = torch.zeros(B, dtype=torch.int32, device=DEV)
    committed_terminal = np.zeros(B, dtype=bool)
    count = np.zeros(B, dtype=np.int64)
    n = dict(goal=0, timeout=0, reset=0, up=0, down=0, respawn=0, idle=0)
    _check_state(env, models, "after reset", count)
    _check_current_objective(ring, models, "after reset")
    for step in range(steps):
        acts = rs.randint(0, A, B).astype(np.int32)
        active = rs.uniform(size=B) < 0.9
        prev_obj = np.stack([m.objective() for m in models]).astype(np.float32)
        out_r.fill_(SENTINEL); out_t.fill_(-1)
        env.process(torch.from_numpy(acts).to(DEV), torch.from_numpy(active.astype(np.int32)).to(DEV), out_r, out_t,
                    reset_on_terminal=True, track_score=True)
        want_r, term = np.full(B, SENTINEL, dtype=np.float32), np.zeros(B, dtype=bool)
        for b in np.flatnonzero(active):
            m = models[b]
            _, r, t, _ = m.process(acts[b])
            want_r[b], term[b] = r, t
            n["goal"] += m.at_goal
            n["timeout"] += m.timed_out
            n["up"] += m.d_after > m.d_before
            n["down"] += m.d_after < m.d_before
            n["respawn"] += m.respawned
            if t:
                m.reset()
                n["reset"] += 1
        n["idle"] += int((~active).sum())
        np.testing.assert_array_equal(out_r.cpu().numpy(), want_r, err_msg=str(step))
        np.testing.assert_array_equal(out_t.cpu().numpy(), np.where(active, term, -1).astype(np.int32), err_msg=str(step))
        old = count.copy()
        discard = term & (old > 0) & committed_terminal
        count = np.where(active & ~discard, old + 1, old)
        committed_terminal = np.where(active & ~discard, term, committed_terminal)
        _check_state(env, models, "step %d" % step, count)
        _check_current_objective(ring, models, "step %d" % step)
        moved_on = np.flatnonzero(count % H1 != old % H1)       # the committed slot keeps the objective of its state
        np.testing.assert_array_equal(_objectives(ring)[moved_on, old[moved_on] % H1], prev_obj[moved_on], err_msg=str(step))
        if step == steps // 2:
            mask = rs.uniform(size=B) < 0.5
            env.reset(torch.from_numpy(mask.astype(np.int32)).to(DEV))
            for b in np.flatnonzero(mask):
                models[b].reset()
            _check_state(env, models, "masked reset", count)
            _check_current_objective(ring, models, "masked reset")
    assert n["goal"] > 0 and n["timeout"] > 0 and n["reset"] > 0 and n["up"] > 0 and n["down"] > 0 and n["idle"] > 0, n
    assert n["respawn"] > 0 or not respawn, n


# ---- 4. the option observes, it does not act --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["static", "generated"])
def test_goal_sense_without_a_progress_reward_changes_nothing_else(kind):
    """goal_sense with progress_reward 0 against the same config without the option, 60 steps through resets: frames,
    pixel change, rewards, terminals, cells and record words 0..4 are identical."""
    B, H = 64, 3
    kw = dict(show_goal=True, max_episode_steps=9, goal_reward=10, hit_reward=-2, action_set="lab")
    if kind == "static":
        make = lambda **o: _static(12, L=5, random_start=True, random_goal=True, **dict(kw, **o))
    else:
        make = lambda **o: _generated(12, gen_loops=2, gen_apples=7, **dict(kw, **o))
    plain, sense = _env(B, H, make(), seed=5), _env(B, H, make(goal_sense=True), seed=5)
    assert plain.ring.r_objective is None and plain.ring.record_words + 72 == sense.ring.record_words
    rs = np.random.RandomState(4)
    z = lambda dt: torch.zeros(B, dtype=dt, device=DEV)
    r0, t0, r1, t1 = z(torch.float32), z(torch.int32), z(torch.float32), z(torch.int32)
    for step in range(60):
        a = torch.from_numpy(rs.randint(0, 6, B).astype(np.int32)).to(DEV)
        plain.process(a, None, r0, t0, track_score=True)
        sense.process(a, None, r1, t1, track_score=True)
        assert torch.equal(r0, r1) and torch.equal(t0, t1), step
        for name in RING_ARRAYS + CFG_ARRAYS:
            if name != "heading":
                assert torch.equal(getattr(plain.ring, name), getattr(sense.ring, name)), (step, name)
        width = plain.ring.record_words                      # (generated: the layout and apple records too)
        a_rec, b_rec = plain.ring.actor_records, sense.ring.actor_records[:, :width]
        assert torch.equal(a_rec[:, :5], b_rec[:, :5]) and torch.equal(a_rec[:, 8:], b_rec[:, 8:]), step
        assert not a_rec[:, 5:8].any()
    assert int(plain.ring.episode.min()) >= 3 and sense.ring.actor_records[:, 7].any()


# ---- 5. the entry on synthetic records --------------------------------------------------------------------------------------
@pytest.mark.parametrize("words", [8 + 25, 8 + 18 + 441 + 65 + 56 + 221])
@pytest.mark.parametrize("B", [1, 3, 257])
def test_objective_entry_on_synthetic_records(B, words):
    """unreal_maze_objective alone: H1 = 3 with counts 0, 2, 3, 7 (the wrap), negative offsets, with and without the
    LSTM-input rows; every other slot, column and record word keeps its sentinel."""
    from unreal_amd import _lib
    from unreal_amd._lib import ptr
    H1, ld, col0 = 3, 272, 263
    rs = np.random.RandomState(B + words)
    rec = rs.randint(-2 ** 31, 2 ** 31 - 1, (B, words)).astype(np.int32)
    rec[:, 5:7] = rs.randint(-20, 21, (B, 2))
    rec[:, 7] = rs.randint(0, 441, B)
    rec[0, 5:8] = [-20, 20, 440]
    count = np.array([0, 2, 3, 7], dtype=np.int32)[np.arange(B) % 4]
    want = rec[:, 5:8].astype(np.float32) / np.array([32, 32, 512], dtype=np.float32)
    assert (np.abs(want) < 1).all() and (want[:, :2] < 0).any()
    d_rec, d_count = torch.from_numpy(rec).to(DEV), torch.from_numpy(count).to(DEV)
    for with_lar in (False, True):
        obj = torch.full((B * H1 * 3,), SENTINEL, device=DEV)
        lar = torch.full((B * ld,), SENTINEL, device=DEV)
        _lib.lib().call("unreal_maze_objective", B, H1, ptr(d_count), ptr(d_rec), words, ptr(obj),
                        ptr(lar) if with_lar else None, ld, col0, None)
        torch.cuda.synchronize()
        got = obj.cpu().numpy().reshape(B, H1, 3)
        slot = count % H1
        np.testing.assert_array_equal(got[np.arange(B), slot], want)
        rest = np.ones((B, H1), dtype=bool)
        rest[np.arange(B), slot] = False
        assert (got[rest] == SENTINEL).all()
        rows = lar.cpu().numpy().reshape(B, ld)
        if with_lar:
            np.testing.assert_array_equal(rows[:, col0:col0 + 3], want)
            assert (rows[:, :col0] == SENTINEL).all() and (rows[:, col0 + 3:] == SENTINEL).all()
        else:
            assert (rows == SENTINEL).all()
        assert torch.equal(d_rec, torch.from_numpy(rec).to(DEV)) and torch.equal(d_count, torch.from_numpy(count).to(DEV))


# ---- 6. fused paths on views ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,kind", [(64, "static"), (300, "generated")])
def test_fused_rollout_steps_are_the_two_launch_paths(B, kind):
    """On two views of each environment (index_parent): rollout_step == process + rollout_advance (+ cur_idx) and
    policy_rollout_step == policy_step + rollout_step, array for array with records and r_objective; the next rows'
    objective columns are what ops.objective_fill reads from the ring at next_idx."""
    from unreal_amd import ops
    H, A, xld = 4, 6, 272
    col0 = 256 + A + 1
    rs = np.random.RandomState(B)
    dev = lambda a, dt: torch.from_numpy(np.asarray(a)).to(DEV, dt)
    Wp = dev(rs.uniform(-.3, .3, 256 * A), torch.float32); bp = dev(rs.uniform(-.1, .1, A), torch.float32)
    Wv = dev(rs.uniform(-.3, .3, 256), torch.float32); bv = dev(rs.uniform(-.1, .1, 1), torch.float32)
    kw = dict(show_goal=True, max_episode_steps=5, goal_reward=10, hit_reward=0, goal_respawn=True, action_set="lab",
              goal_sense=True, progress_reward=2)
    if kind == "static":
        cfg = _static(7, L=3, random_start=True, random_goal=True, **kw)
    else:
        cfg = _generated(7, styled=True, gen_apples=4, **kw)
    arrays = RING_ARRAYS + CFG_ARRAYS + ("r_objective", "gen" if kind == "generated" else "nav")
    envs = [_env(B, H, cfg, seed=9) for _ in range(3)]
    cut = B // 3
    views = [[e.view(0, cut), e.view(cut, B)] for e in envs]
    assert views[0][1].ring.record_words == cfg.record_words and views[0][1].ring.actor_records.shape[0] == B - cut
    st = [_rollout_state(B, xld) for _ in envs]
    for s in st:
        s["pi"] = torch.zeros(B * A, dtype=torch.float32, device=DEV)
        s["lar"].fill_(SENTINEL)
    n_term, n_rew = 0, set()
    for step in range(10):
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
        for name in arrays:
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
        # the next rows: [one-hot last action | last reward | objective], the objective as objective_fill reads it
        want = torch.full((B * xld,), SENTINEL, device=DEV)
        ops.lar_fill(B, A, envs[0].ring.last_action, envs[0].ring.last_reward, None, want, xld)
        ops.objective_fill(envs[0].ring, B, st[0]["idx"], want, xld, col0)
        rows, got = want.view(B, xld), st[1]["lar"].view(B, xld)
        assert torch.equal(got[:, 256:col0 + 3], rows[:, 256:col0 + 3]), step
        assert (got[:, :256] == SENTINEL).all() and (got[:, col0 + 3:] == SENTINEL).all()     # nothing else is written
        rec = _records(envs[0].ring)[:, 5:8].astype(np.float32) / np.array([32, 32, 512], dtype=np.float32)
        np.testing.assert_array_equal(rows[:, col0:col0 + 3].cpu().numpy(), rec, err_msg=str(step))
        n_term += int(st[0]["te"].sum())
        n_rew |= set(st[0]["r"][live].cpu().numpy().tolist())
        if step in (4, 8):
            for s in st:
                s["active"].fill_(1); s["te"].zero_(); s["n"].zero_()
    assert n_term > 0 and {2.0, -2.0} <= n_rew, (n_term, n_rew)
    assert int(envs[0].ring.episode.min()) >= 2


# ---- 7. the trainer ---------------------------------------------------------------------------------------------------------
GOAL_KW = dict(NAV_KW, goal_sense=True, progress_reward=1, max_episode_steps=7)


def _oracle_pair(name, cfg, B, seed, groups=1):
    from oracle.trainer import OracleTrainer, ExplicitDraws
    from unreal_amd.environment.environment import Environment
    conf = Environment.MAZE_CONFIG[name]
    cfg["action_size"] = 6
    cfg["objective_size"] = 3
    cfg["initial_learning_rate"] = 7.0711e-4
    net, applier, tr, draws = _build(cfg, B, seed=seed, env_name=name, groups=groups)
    assert tr.objective_size == 3 and net._objective_size == 3 and tr.full_ring.objective_size == 3
    params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
    edraws = [ExplicitDraws() for _ in range(B)]
    hosts = GOAL.host_batch(conf, B, seed=tr.seed)
    orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=hosts)
    return net, applier, tr, draws, edraws, hosts, orc


@pytest.mark.parametrize("use_lstm,aux", [(True, True), (False, False)])
def test_process_on_a_goal_sense_maze_matches_oracle(use_lstm, aux):
    """Trainer.process against OracleTrainer(objective_size=3) with one host model per actor, at the bars of the navigation
    process tests: full UNREAL with the LSTM (the objective in its input), and feed-forward without auxiliary tasks
    (where, as in the reference, the objective is carried but unused)."""
    from unreal_amd.environment.environment import Environment
    name = "goal_room_%d%d" % (use_lstm, aux)
    _register(name, **GOAL_KW)
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(use_lstm, aux, H, T)
        net, applier, tr, draws, edraws, hosts, orc = _oracle_pair(name, cfg, B, 3)
        assert not net.lar_bounded                      # goal 10
        while not tr._full:
            tr.process(None, 0)
        for step_u in draws.log:
            for b in range(B):
                edraws[b].action_u.append(float(step_u[b]))
        orc.fill()
        np.testing.assert_array_equal(tr.ring.count.cpu().numpy(), [a.exp.count for a in orc.actors])
        np.testing.assert_array_equal(_records(tr.ring), np.stack([h.actor_record() for h in hosts]))
        rewards, objectives = set(), set()
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
                objectives.add(tuple(hosts[b].last_state["objective"]))
            for key in ("policy_loss", "value_loss", "pc_loss", "vr_loss", "rp_loss", "total_loss"):
                if key not in losses_dev or key not in losses_o[0]:
                    continue
                want = np.mean([l[key] for l in losses_o])
                assert abs(losses_dev[key] - want) <= LOSS_ATOL + LOSS_RTOL * abs(want), (it, key, losses_dev[key], want)
            for (pname, _), gref in zip(orc.params.items(), mean_g):
                gr = gref.numpy().reshape(-1)
                assert np.abs(g_dev[pname] - gr).max() <= GRAD_ATOL + GRAD_REL * np.abs(gr).max(), (it, pname)
            assert abs(float(tr.last_grad_norm.cpu()[0]) - norm_o) <= 1e-4 * max(1.0, norm_o)
            np.testing.assert_array_equal(_records(tr.ring), np.stack([h.actor_record() for h in hosts]))
            _check_current_objective(tr.ring, hosts, "call %d" % it)
        assert all(h.episode >= 2 for h in hosts)                       # the oracle saw resets ...
        assert len(objectives) > 1 and all(any(o) for o in objectives)   # ... and objectives that are not zero
        assert {1.0, -1.0} & rewards                                    # the progress reward was paid
    finally:
        Environment.MAZE_CONFIG.pop(name, None)


def test_grouped_process_on_a_goal_sense_maze_is_the_reference_algorithm():
    """groups = B: one process() call = B sequential single-actor passes through ring views, against
    OracleTrainer.process_async."""
    from unreal_amd.environment.environment import Environment
    name = "goal_room_grouped"
    _register(name, **dict(GOAL_KW, max_episode_steps=5))
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(True, True, H, T)
        net, applier, tr, draws, edraws, hosts, orc = _oracle_pair(name, cfg, B, 13, groups=B)
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
            np.testing.assert_array_equal(_records(tr.full_ring), np.stack([h.actor_record() for h in hosts]))
            _check_current_objective(tr.full_ring, hosts, "call %d" % it)
            global_t += steps_dev
        assert n_scores > 0
    finally:
        Environment.MAZE_CONFIG.pop(name, None)


def test_trainer_refuses_a_network_without_the_objective_columns():
    from unreal_amd.environment.environment import Environment
    from unreal_amd.model.model import UnrealModel
    from unreal_amd.train.rmsprop_applier import RMSPropApplier
    from unreal_amd.train.trainer import Trainer
    name = "goal_room_mismatch"
    _register(name, **GOAL_KW)
    try:
        assert Environment.get_objective_size("maze", name) == 3
        net = UnrealModel(6, 0, -1, True, True, True, True, 0.05, 0.001, DEV)
        applier = RMSPropApplier(None, decay=0.99, momentum=0.0, epsilon=0.1, clip_norm=40.0, device=DEV)
        with pytest.raises(ValueError, match="objective_size"):
            Trainer(0, net, 7e-4, None, applier, "maze", name, True, True, True, True, 0.05, 0.001, 20, 20, 0.99, 0.9, 40,
                    10 ** 6, DEV, batch_size=3)
    finally:
        Environment.MAZE_CONFIG.pop(name, None)


# ---- 8. Evaluate and the batch-1 environment ---------------------------------------------------------------------------------
def test_evaluate_reports_start_distance_and_spl():
    """Evaluate(maze=name) on a goal-sense config without goal_respawn: start_distance and spl are those of the host model
    replaying the device's actions (first episodes; every action counts as a step)."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.evaluate import Evaluate
    name = "goal_room_eval"
    lay = NAV_ROOM                                   # nine free cells: an untrained policy finds some goals in 12 steps
    conf = _register(name, lay, random_goal=True, random_start=True, **dict(GOAL_KW, max_episode_steps=12))
    try:
        cfg = _cfg(True, False, 40, 20)
        cfg["action_size"] = 6
        net, _, _, _ = _build(cfg, 1, seed=31, env_name=name)
        B, seed = 32, 0x5EED
        ev = Evaluate(net, batch_size=B, device=DEV, seed=seed, maze=name)
        log = []
        inner = ev.env.process

        def recording(actions, active, out_reward, out_terminal, **kw):
            inner(actions, active, out_reward, out_terminal, **kw)
            log.append((actions.cpu().numpy().copy(), out_reward.cpu().numpy().copy(), out_terminal.cpu().numpy().copy()))
        ev.env.process = recording
        res = ev.process(0, one_episode_per_actor=True)
        hosts = GOAL.host_batch(conf, B, seed=seed)
        for h in hosts:
            h.reset()
        d0 = [h.distance() for h in hosts]
        first = [None] * B
        for step, (acts, rew, term) in enumerate(log):
            for b, h in enumerate(hosts):
                _, r, t, _ = h.process(acts[b])
                assert (float(r), int(t)) == (float(rew[b]), int(term[b])), (step, b)
                if t:
                    if first[b] is None:
                        first[b] = (d0[b], h.ep_steps, h.at_goal)
                    h.reset()
        assert None not in first and all(d >= 1 for d, _, _ in first)
        spl = [d / float(max(d, n)) if ok else 0.0 for d, n, ok in first]
        assert res["episodes"] == B
        assert abs(res["start_distance"] - np.mean([d for d, _, _ in first])) < 1e-12
        assert abs(res["spl"] - np.mean(spl)) < 1e-12
        assert abs(res["success_rate"] - np.mean([ok for _, _, ok in first])) < 1e-12
        assert 0 < res["spl"] < 1, res
        # with goal_respawn (or without goal_sense) the two keys are absent
        _register(name + "_r", lay, random_goal=True, random_start=True, **dict(GOAL_KW, max_episode_steps=6,
                                                                                    goal_respawn=True))
        res = Evaluate(net, batch_size=4, device=DEV, seed=seed, maze=name + "_r").process(0, one_episode_per_actor=True)
        assert "spl" not in res and "start_distance" not in res
    finally:
        Environment.MAZE_CONFIG.pop(name, None)
        Environment.MAZE_CONFIG.pop(name + "_r", None)


def test_batch1_environment_hands_out_the_objective():
    """Environment.create_environment('maze', name): last_state['objective'] is the model's float64 [3] at the reset and
    over 30 steps (the caller resets at a terminal)."""
    from unreal_amd.environment.environment import Environment
    name = "goal_room_batch1"
    lay = ["-------", "--A-A--", "-A+++A-", "---A---", "-A+-+A-", "--A-A--", "-------"]
    conf = _register(name, lay, random_goal=True, random_start=True, **dict(GOAL_KW, max_episode_steps=9))
    try:
        env = Environment.create_environment("maze", name)
        host = GOAL.HostGoalMaze(conf, 0, 1, seed=0)
        host.reset()
        rs = np.random.RandomState(2)
        seen = set()
        for step in range(30):
            obj = env.last_state["objective"]
            assert obj.dtype == np.float64 and obj.shape == (3,)
            np.testing.assert_array_equal(obj, host.last_state["objective"], err_msg=str(step))
            np.testing.assert_array_equal(env.last_state["image"], host.last_state["image"], err_msg=str(step))
            seen.add(tuple(obj))
            a = int(rs.randint(0, 6))
            image, reward, terminal, pc = env.process(a)
            _, r, t, pc_h = host.process(a)
            assert (reward, terminal) == (r, t), step
            if terminal:
                env.reset()
                host.reset()
        assert len(seen) > 5
    finally:
        Environment.MAZE_CONFIG.pop(name, None)
