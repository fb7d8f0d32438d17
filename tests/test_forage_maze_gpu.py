"""Foraging first-person mazes on the device (maze.hip, a block with flag 128, views 5 and 6), bit for bit
against the host model of tests/forage_maze_model.py: resets, pickup kinds in the frames, ending pickups, goal-less
episodes, generated pickups, the fused paths on views, OracleTrainer, Evaluate and the batch-1 environment."""
import numpy as np
import pytest
import torch

try:
    import maze_model as MM
    import nav_maze_model as NM
    import forage_maze_model as FM
except ImportError:            # imported as tests.<module>
    from tests import maze_model as MM
    from tests import nav_maze_model as NM
    from tests import forage_maze_model as FM
try:
    from test_maze_config_gpu import RING_ARRAYS, CFG_ARRAYS
    from test_fp_maze_gpu import _env, _current_frames, _rollout_state
    from test_nav_maze_gpu import _cfg, _build, _feed_draws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL, _register
except ImportError:
    from tests.test_maze_config_gpu import RING_ARRAYS, CFG_ARRAYS
    from tests.test_fp_maze_gpu import _env, _current_frames, _rollout_state
    from tests.test_nav_maze_gpu import _cfg, _build, _feed_draws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL, _register

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB, PC = 21168, 400
SIZES = (7, 12, 14, 21)
STYLES = [(200, 100, 50, 0xAA), (0, 255, 0, 0x00), (10, 20, 250, 0x0F)]
YELLOW, PINK, CYAN = (255, 255, 0), (255, 0, 255), (0, 255, 255)
# B: a lemon; C: a small good one; D: the melon, which ends the episode
KINDS = [(-1, YELLOW, False), (5, CYAN, False), (20, PINK, True)]
# pickups per static layout as marks of MM.random_layout (N = 21: 64, the most an actor has bits for)
MARKS = {7: "AABBCD", 12: "A" * 6 + "B" * 6 + "C" * 4 + "D" * 4, 14: "A" * 10 + "B" * 10 + "C" * 5 + "D" * 5,
         21: "A" * 24 + "B" * 20 + "C" * 12 + "D" * 8}
SENTINEL = -7.5


def _static(N, L=7, seed=0, marks=None, **kw):
    from unreal_amd.environment.maze_environment import MazeConfig
    rs = np.random.RandomState(seed + N)
    marks = MARKS[N] if marks is None else marks
    if not kw.get("no_goal"):
        marks = "G" + marks
    kw.setdefault("pickups", KINDS)
    return MazeConfig([MM.random_layout(N, rs, marks="S" + marks) for _ in range(L)], view="first_person", **kw)


def _generated(N, styled=False, **kw):
    from unreal_amd.environment.maze_environment import MazeConfig
    if styled:
        kw = dict(kw, wall_styles=STYLES, gen_landmark_density=64)
    kw.setdefault("pickups", KINDS)
    return MazeConfig(None, random_start=True, random_goal=not kw.get("no_goal"), view="first_person", generate=N, **kw)


def _hosts(cfg, B, seed, frames=True):
    """Host models of an environment built by _env: its constructor and _env each reset once (episode 1)."""
    models = FM.host_batch(cfg, B, seed=seed, frames=frames)
    for m in models:
        m.reset()
    return models


def _records(ring):
    return ring.actor_records.cpu().numpy()


def _check_state(env, models, what, count=None):
    """Count, cells, headings, goals, episode counters, last action / reward, the whole per-actor record (a generated
    maze's layout, pickup and style words with it) and the current frames of the models that render."""
    ring, B = env.ring, len(models)
    if count is not None:
        np.testing.assert_array_equal(ring.count.cpu().numpy(), count, err_msg=what)
    rec = _records(ring)
    want = np.stack([m.actor_record() for m in models])
    assert rec.shape == want.shape == (B, env.config.record_words), (rec.shape, want.shape)
    bad = np.flatnonzero((rec != want).any(1))
    assert not len(bad), "%s: records of actors %s differ (first words %s: %s, want %s)" % (
        what, bad[:8], np.flatnonzero(rec[bad[0]] != want[bad[0]])[:8], rec[bad[0]][:8], want[bad[0]][:8])
    np.testing.assert_array_equal(ring.pos.cpu().numpy().reshape(B, 2), [(m.x, m.y) for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.heading.cpu().numpy(), [m.h for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.goal.cpu().numpy().reshape(B, 2), [(m.gx, m.gy) for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.ep_steps.cpu().numpy(), [m.ep_steps for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.episode.cpu().numpy(), [m.episode for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.last_action.cpu().numpy(), [m.last_action for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.last_reward.cpu().numpy(), np.array([m.last_reward for m in models], np.float32),
                                  err_msg=what)
    seeing = [b for b, m in enumerate(models) if m.frames]
    if seeing:
        got = _current_frames(ring)[seeing]
        want = np.stack([models[b].frame.reshape(-1) for b in seeing])
        bad = np.flatnonzero((got != want).any(1))
        assert not len(bad), "%s: frames of actors %s differ" % (what, [seeing[i] for i in bad[:8]])


def _colours_seen(models):
    """The kinds whose floor colour shows in some model's current frame."""
    table = FM.kind_table(models[0]._base_config())
    return set(k for k, (_, colour, _) in enumerate(table) for m in models
               if m.frames and (m.frame == np.array(colour, np.uint8)).all(2).any())


# ---- 1. reset ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no_goal", [False, True])
@pytest.mark.parametrize("kind", ["static", "generated"])
@pytest.mark.parametrize("N,B", [(N, B) for N in SIZES for B in (3, 64)])
def test_reset_matches_the_host_model(N, B, kind, no_goal):
    """Static (7 layouts) and generated + styled, with a goal and without: frames with every kind's colour, records,
    cells, headings and ring.goal ((-1, -1) without a goal) are the model's; then a reset under a mask over slots filled
    with a sentinel: the other actors' records and frames keep theirs."""
    seed = 0xF0A1 + N + B
    kw = dict(max_episode_steps=30, no_goal=no_goal)
    if not no_goal:
        kw.update(show_goal=True, random_goal=True)
    if kind == "static":
        cfg = _static(N, L=7, seed=B, random_start=True, **kw)
    else:
        kw.pop("random_goal", None)
        R = (N + 1) // 2
        cfg = _generated(N, styled=True, gen_loops=2, gen_apples=R, gen_pickups=(R, R, R), **kw)
    assert cfg.forage and cfg.nav and cfg.flags & 128
    env = _env(B, 2, cfg, seed=seed)
    ring = env.ring
    assert env.maze[0] == (5 if kind == "static" else 6) and ring.record_words == cfg.record_words
    models = _hosts(cfg, B, seed)
    _check_state(env, models, "reset")
    if no_goal:
        assert (ring.goal.cpu().numpy() == -1).all()
    if B == 64:
        assert _colours_seen(models) == {0, 1, 2, 3}
    count = (np.arange(B) % 5).astype(np.int32)              # slots 0, 1, 2 of H1 = 3
    ring.count.copy_(torch.from_numpy(count))
    ring.frames.fill_(0x5A)
    mask = np.random.RandomState(B).uniform(size=B) < 0.5
    before = _records(ring).copy()
    env.reset(torch.from_numpy(mask.astype(np.int32)).to(DEV))
    for b in np.flatnonzero(mask):
        models[b].reset()
    np.testing.assert_array_equal(_records(ring)[~mask], before[~mask])
    frames = ring.frames.view(B, 3, FB).cpu().numpy()
    slot = count % 3
    for b in range(B):
        for s in range(3):
            if mask[b] and s == slot[b]:
                np.testing.assert_array_equal(frames[b, s], models[b].frame.reshape(-1), err_msg=str(b))
            else:
                assert (frames[b, s] == 0x5A).all(), (b, s)
    if kind == "generated":
        walls, cells, letters = env.current_layouts()
        for b, m in enumerate(models):
            assert list(cells[b]) == m._pickups()[0]
            assert [letters[b][c] for c in cells[b]] == [FM.LETTERS[k] for k in m._pickups()[1]]
            assert letters[b] == "".join(ch if ch in "+ABCD" else "-" for ch in
                                         cfg.generated_layout(seed, b, m.episode).translate({ord(d): "+" for d in "1234567"}))


# ---- 2. random steps -------------------------------------------------------------------------------------------------------
# (N, kind, action set, goal mode): both sizes static and generated, both action sets, every goal mode
STEP_CASES = [(7, "static", "turn", "respawn"), (7, "generated", "lab", "none"), (7, "static", "lab", "terminal"),
              (21, "static", "lab", "none"), (21, "generated", "turn", "respawn"), (21, "generated", "lab", "terminal")]
STEPS, STEP_B, SEEING = 120, 200, 6


def _step_config(N, kind, action_set, goal):
    """The config and the seed of a step case.  N = 7: two kinds (a lemon at -1, a melon at +20 that ends the episode);
    N = 21: three (a +5 between them).  The most pickups an actor can hold: 64 at N = 21 static, one in each of the 16 rooms
    of a generated N = 7."""
    kinds = [KINDS[0], KINDS[2]] if N == 7 else KINDS
    kw = dict(max_episode_steps=23, apple_reward=1, hit_reward=-2, action_set=action_set, pickups=kinds,
              no_goal=goal == "none")
    if goal != "none":
        kw.update(show_goal=True, goal_reward=10, goal_respawn=goal == "respawn")
    if kind == "static":
        if goal != "none":
            kw.update(random_goal=True)
        marks = "AAABBBCC" if N == 7 else MARKS[21]
        cfg = _static(N, L=7, seed=N, marks=marks, random_start=True, **kw)
    elif N == 7:
        cfg = _generated(7, gen_loops=4, gen_apples=6, gen_pickups=(6, 4), **kw)
    else:
        cfg = _generated(21, gen_loops=12, gen_apples=24, gen_pickups=(20, 12, 8), **kw)
    return cfg, 0xF0A2 + N + len(kind) + len(goal)


def run_step_case(N, kind, action_set, goal, env=None):
    """Drives the host models of a step case through STEPS random steps under an `active` mask with a masked reset half
    way and, with `env` (the device environment of the same config and seed), checks the device against them at every
    step.  -> the counters of what the models' trace contained."""
    cfg, seed = _step_config(N, kind, action_set, goal)
    B, H1, A = STEP_B, 4, cfg.action_size
    K = len(cfg.pickups)
    models = _hosts(cfg, B, seed, frames=SEEING)
    rs = np.random.RandomState(N)
    n = dict(picked=[0] * 4, ended=0, timeout=0, goal=0, respawn=0, on_pickup=0, idle=0, high_bit=0, hit=0)
    committed_terminal = np.zeros(B, dtype=bool)
    count = np.zeros(B, dtype=np.int64)
    if env is not None:
        ring = env.ring
        out_r = torch.zeros(B, dtype=torch.float32, device=DEV)
        out_t = torch.zeros(B, dtype=torch.int32, device=DEV)
        _check_state(env, models, "after reset", count)
    for step in range(STEPS):
        acts = rs.randint(0, A, B).astype(np.int32)
        active = rs.uniform(size=B) < 0.9
        if env is not None:
            out_r.fill_(SENTINEL); out_t.fill_(-1)
            env.process(torch.from_numpy(acts).to(DEV), torch.from_numpy(active.astype(np.int32)).to(DEV), out_r, out_t,
                        reset_on_terminal=True, track_score=True)
        want_r, term = np.full(B, SENTINEL, dtype=np.float32), np.zeros(B, dtype=bool)
        want_pc = {}
        for b in np.flatnonzero(active):
            m = models[b]
            _, r, t, pc = m.process(acts[b])
            want_r[b], term[b] = r, t
            if m.frames:
                want_pc[b] = pc
            if m.picked >= 0:
                n["picked"][m.picked] += 1
            n["ended"] += m.ended_by_pickup
            n["timeout"] += m.timed_out
            n["goal"] += m.at_goal
            n["respawn"] += m.respawned
            n["on_pickup"] += m.on_pickup
            n["hit"] += m.hit
            n["high_bit"] += (m.collected >> 32) != 0
            if t:
                m.reset()
                n["on_pickup"] += m.starts_on_pickup()
        n["idle"] += int((~active).sum())
        old = count.copy()
        discard = term & (old > 0) & committed_terminal
        count = np.where(active & ~discard, old + 1, old)
        committed_terminal = np.where(active & ~discard, term, committed_terminal)
        if env is not None:
            np.testing.assert_array_equal(out_r.cpu().numpy(), want_r, err_msg=str(step))
            np.testing.assert_array_equal(out_t.cpu().numpy(), np.where(active, term, -1).astype(np.int32), err_msg=str(step))
            _check_state(env, models, "step %d" % step, count)
            r_pc = ring.r_pc.view(B, H1, PC).cpu().numpy()
            for b, pc in want_pc.items():
                np.testing.assert_array_equal(r_pc[b, old[b] % H1], pc.reshape(-1), err_msg="%d %d" % (step, b))
        if step == STEPS // 2:
            mask = rs.uniform(size=B) < 0.5
            for b in np.flatnonzero(mask):
                models[b].reset()
                n["on_pickup"] += models[b].starts_on_pickup()
            if env is not None:
                env.reset(torch.from_numpy(mask.astype(np.int32)).to(DEV))
                _check_state(env, models, "masked reset", count)
    n["kinds"] = K
    return n


def check_trace(n, N, kind, goal):
    """What every step case's trace must contain (of the host model alone)."""
    assert all(c > 0 for c in n["picked"][:1 + n["kinds"]]), n           # every configured kind was collected
    assert n["ended"] > 0 and n["timeout"] > 0 and n["on_pickup"] > 0 and n["idle"] > 0 and n["hit"] > 0, n
    assert (n["goal"] > 0) == (goal != "none") and (n["respawn"] > 0) == (goal == "respawn"), n
    if N == 21 and kind == "static":
        assert n["high_bit"] > 0, n                                      # bits 32..63 of the collected mask


@pytest.mark.parametrize("N,kind,action_set,goal", STEP_CASES)
def test_random_steps_match_the_host_model(N, kind, action_set, goal):
    """200 actors (static: over 7 layouts), a step limit of 23, 120 random actions under an `active` mask, a masked reset
    half way: rewards, terminals, counts, cells, the whole records and, for the first actors, frames and pixel change
    (the other models render none, which keeps a case to a few seconds).  Every kind is collected, pickups end episodes,
    episodes time out, and resets or respawns land on pickup cells."""
    cfg, seed = _step_config(N, kind, action_set, goal)
    env = _env(STEP_B, 3, cfg, seed=seed)
    if kind == "static":
        assert len(set(env.ring.layout.cpu().numpy())) == 7
        assert max(len(c) for c in cfg.pickup_cells) == (64 if N == 21 else 8)
    n = run_step_case(N, kind, action_set, goal, env)
    check_trace(n, N, kind, goal)
    totals = _records(env.ring)[:, 4:8].sum(0)
    assert list(totals[:1 + n["kinds"]]) == n["picked"][:1 + n["kinds"]] and not totals[1 + n["kinds"]:].any()


def test_sixteen_rooms_of_a_generated_maze_all_hold_a_pickup():
    """generate=7 with gen_apples + gen_pickups = 16: every room holds one, the records and frames are the model's."""
    cfg = _generated(7, gen_loops=9, gen_apples=4, gen_pickups=(4, 4, 4), no_goal=True, max_episode_steps=9)
    env = _env(64, 2, cfg, seed=3)
    models = _hosts(cfg, 64, 3)
    _check_state(env, models, "reset")
    rec = _records(env.ring)
    arec = rec[:, 8 + 18 + 49:8 + 18 + 49 + 65]
    assert (arec[:, 0] == 16).all()
    rooms = [2 * j * 7 + 2 * i for j in range(4) for i in range(4)]
    assert all(list(a[1:17] & 0xFFFF) == rooms and sorted(a[1:17] >> 16) == [0] * 4 + [1] * 4 + [2] * 4 + [3] * 4
               for a in arec)


# ---- 3. the fused entries -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,A,kind", [(64, 4, "static"), (300, 6, "static"), (64, 6, "generated"), (300, 4, "generated")])
def test_fused_rollout_steps_are_the_two_launch_paths(B, A, kind):
    """On two views of each environment (index_parent): rollout_step == process + rollout_advance (+ cur_idx and the
    LSTM-input columns), and policy_rollout_step == policy_step + rollout_step, bit for bit, with pickups of every
    reward and episodes ended by pickups and time-outs."""
    from unreal_amd import ops
    H, xld = 4, 264
    rs = np.random.RandomState(B)
    dev = lambda a, dt: torch.from_numpy(np.asarray(a)).to(DEV, dt)
    Wp = dev(rs.uniform(-.3, .3, 256 * A), torch.float32); bp = dev(rs.uniform(-.1, .1, A), torch.float32)
    Wv = dev(rs.uniform(-.3, .3, 256), torch.float32); bv = dev(rs.uniform(-.1, .1, 1), torch.float32)
    kw = dict(max_episode_steps=6, hit_reward=0, action_set="lab" if A == 6 else "turn", no_goal=True)
    if kind == "static":
        cfg = _static(7, L=3, marks="AAAABBBBCCCDDD", random_start=True, **kw)
    else:
        cfg = _generated(7, gen_loops=9, gen_apples=4, gen_pickups=(4, 3, 3), **kw)
    arrays = RING_ARRAYS + CFG_ARRAYS + (("nav",) if kind == "static" else ("gen",))
    envs = [_env(B, H, cfg, seed=9) for _ in range(3)]
    cut = B // 3
    views = [[e.view(0, cut), e.view(cut, B)] for e in envs]
    st = [_rollout_state(B, xld) for _ in envs]
    for s in st:
        s["pi"] = torch.zeros(B * A, dtype=torch.float32, device=DEV)
    n_term, n_rew = 0, set()
    for step in range(12):
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
        lar = st[1]["lar"].view(B, xld)[:, 256:256 + A + 1].cpu().numpy()
        la, lr = envs[0].ring.last_action.cpu().numpy(), envs[0].ring.last_reward.cpu().numpy()
        np.testing.assert_array_equal(lar[:, :A], np.eye(A, dtype=np.float32)[la], err_msg=str(step))
        np.testing.assert_array_equal(lar[:, A], lr, err_msg=str(step))
        n_term += int(st[0]["te"].sum())
        n_rew |= set(st[0]["r"][live].cpu().numpy().tolist())
        if step in (4, 8):
            for s in st:
                s["active"].fill_(1); s["te"].zero_(); s["n"].zero_()
    assert n_term > 0 and {1.0, -1.0, 5.0, 20.0} <= n_rew, (n_term, n_rew)
    assert (envs[0].ring.actor_records[:, 4:8].sum(0) > 0).all()


# ---- 4. other blocks keep their kernels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["static", "generated"])
def test_a_navigation_config_without_the_options_keeps_its_view(kind):
    """Apples and none of the new options through Environment: view 1 (static) or 2 (generated), a block without flag 128
    and a 60-step trace equal to the navigation host model's."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.maze_environment import batched_maze_environment
    try:
        import gen_maze_model as GM
    except ImportError:
        from tests import gen_maze_model as GM
    name = "forage_plain_nav_" + kind
    kw = dict(view="first_person", random_start=True, random_goal=True, max_episode_steps=11, goal_reward=10, hit_reward=-2,
              show_goal=True)
    if kind == "static":
        rs = np.random.RandomState(5)
        Environment.register_maze_config(name, [MM.random_layout(7, rs, marks="AAAAAA") for _ in range(3)], **kw)
    else:
        Environment.register_maze_config(name, None, generate=7, gen_loops=3, gen_apples=5, **kw)
    try:
        conf = Environment.MAZE_CONFIG[name]
        assert conf.nav and not conf.forage and not conf.flags & 128
        B = 32
        env = batched_maze_environment(B, 3, DEV, config=conf, seed=4)
        assert env.maze[0] == (1 if kind == "static" else 2)
        env.ring.frames.zero_()
        env.reset()
        models = (NM if kind == "static" else GM).host_batch(conf, B, seed=4)
        for m in models:
            m.reset()
        rs = np.random.RandomState(6)
        out_r = torch.zeros(B, dtype=torch.float32, device=DEV)
        out_t = torch.zeros(B, dtype=torch.int32, device=DEV)
        n_apple = n_term = 0
        for step in range(60):
            acts = rs.randint(0, 4, B).astype(np.int32)
            env.process(torch.from_numpy(acts).to(DEV), None, out_r, out_t, reset_on_terminal=True)
            want = [m.process(a)[1:3] for m, a in zip(models, acts)]
            n_apple += sum(m.apple for m in models)
            for m, (_, t) in zip(models, want):
                if t:
                    m.reset()
                    n_term += 1
            assert out_r.cpu().tolist() == [float(r) for r, _ in want], step
            assert out_t.cpu().tolist() == [int(t) for _, t in want], step
            np.testing.assert_array_equal(_records(env.ring)[:, :8], [m.record() for m in models], err_msg=str(step))
            np.testing.assert_array_equal(_current_frames(env.ring), np.stack([m.frame.reshape(-1) for m in models]))
        assert n_apple > 0 and n_term > 0
    finally:
        Environment.MAZE_CONFIG.pop(name, None)


def test_a_forage_block_in_another_views_kernel_writes_nothing_and_the_reverse():
    """View 1 on a forage block and view 5 on a navigation block (and 2 / 6 on generated ones): reset and step return
    before any store."""
    from unreal_amd import ops
    B = 8
    z = lambda dt: torch.zeros(B, dtype=dt, device=DEV)
    pairs = [(_static(7, L=1, random_start=True, no_goal=True, max_episode_steps=5), 1),
             (_static(7, L=1, marks="AAA", random_start=True, random_goal=True, pickups=None), 5),
             (_generated(7, gen_apples=3, gen_pickups=(2, 2, 2), no_goal=True, max_episode_steps=5), 2),
             (_generated(7, gen_apples=3, pickups=None), 6)]
    for cfg, wrong in pairs:
        env = _env(B, 2, cfg, seed=1)
        names = RING_ARRAYS + CFG_ARRAYS + (("nav",) if cfg.generate is None else ("gen",))
        before = {n: getattr(env.ring, n).clone() for n in names}
        maze = (wrong,) + env.maze[1:]
        ops.maze_reset(env.ring, None, maze=maze)
        ops.maze_step(env.ring, z(torch.int32) + 2, None, z(torch.float32), z(torch.int32), maze=maze)
        torch.cuda.synchronize()
        for n, t in before.items():
            assert torch.equal(getattr(env.ring, n), t), (wrong, n)


# ---- 5. trainer, evaluation, batch 1 -----------------------------------------------------------------------------------------
# no goal: apples, lemons (B, -1) and a melon (C, +20, ends the episode) around S
FORAGE_ROOM = ["+++++++",
               "+++++++",
               "++ABA++",
               "++-SB++",
               "++A-C++",
               "+++++++",
               "+++++++"]
FORAGE_KW = dict(no_goal=True, apple_reward=1, hit_reward=0, action_set="lab",
                 pickups=[(-1, YELLOW, False), (20, PINK, True)])


@pytest.mark.parametrize("use_lstm,aux", [(True, True), (False, False)])
def test_process_on_a_forage_maze_matches_oracle(use_lstm, aux):
    """Trainer.process against OracleTrainer with one host model per actor on a no_goal config with a -1 kind and an
    ending kind (the LSTM input's reward column unbounded), at the bars of test_nav_maze_gpu."""
    from unreal_amd.environment.environment import Environment
    from oracle.trainer import OracleTrainer, ExplicitDraws
    name = "forage_room_%d%d" % (use_lstm, aux)
    conf = _register(name, FORAGE_ROOM, max_episode_steps=7, **FORAGE_KW)
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(use_lstm, aux, H, T)
        cfg["action_size"] = 6
        cfg["initial_learning_rate"] = 7.0711e-4
        net, applier, tr, draws = _build(cfg, B, seed=3, env_name=name)
        assert tr.action_size == 6 and not net.lar_bounded and conf.reward_bound == 20
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = FM.host_batch(conf, B, seed=tr.seed)
        orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=hosts)
        while not tr._full:
            tr.process(None, 0)
        for step_u in draws.log:
            for b in range(B):
                edraws[b].action_u.append(float(step_u[b]))
        orc.fill()
        np.testing.assert_array_equal(tr.ring.count.cpu().numpy(), [a.exp.count for a in orc.actors])
        np.testing.assert_array_equal(tr.ring.nav.cpu().numpy().reshape(B, 8), [h.record() for h in hosts])
        rewards = set()
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
            for key in ("policy_loss", "value_loss", "pc_loss", "vr_loss", "rp_loss", "total_loss"):
                if key not in losses_dev or key not in losses_o[0]:
                    continue
                want = np.mean([l[key] for l in losses_o])
                assert abs(losses_dev[key] - want) <= LOSS_ATOL + LOSS_RTOL * abs(want), (it, key, losses_dev[key], want)
            for (pname, _), gref in zip(orc.params.items(), mean_g):
                gr = gref.numpy().reshape(-1)
                assert np.abs(g_dev[pname] - gr).max() <= GRAD_ATOL + GRAD_REL * np.abs(gr).max(), (it, pname)
            assert abs(float(tr.last_grad_norm.cpu()[0]) - norm_o) <= 1e-4 * max(1.0, norm_o)
            np.testing.assert_array_equal(tr.ring.pos.cpu().numpy().reshape(B, 2), [(h.x, h.y) for h in hosts])
            np.testing.assert_array_equal(tr.ring.nav.cpu().numpy().reshape(B, 8), [h.record() for h in hosts])
        totals = np.sum([h.totals for h in hosts], 0)
        assert (totals[:3] > 0).all() and {1.0, -1.0, 20.0} <= rewards, (totals, rewards)
    finally:
        Environment.MAZE_CONFIG.pop(name, None)


def test_grouped_process_on_a_forage_maze_is_the_reference_algorithm():
    """groups = B: one process() call = B sequential single-actor passes, against OracleTrainer.process_async."""
    from unreal_amd.environment.environment import Environment
    from oracle.trainer import OracleTrainer, ExplicitDraws
    name = "forage_room_grouped"
    conf = _register(name, FORAGE_ROOM, max_episode_steps=5, **FORAGE_KW)
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(True, True, H, T)
        cfg["action_size"] = 6
        cfg["initial_learning_rate"] = 7.0711e-4
        net, applier, tr, draws = _build(cfg, B, seed=13, env_name=name, groups=B)
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = FM.host_batch(conf, B, seed=tr.seed)
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
            np.testing.assert_array_equal(tr.full_ring.nav.cpu().numpy().reshape(B, 8), [h.record() for h in hosts])
            global_t += steps_dev
        assert n_scores > 0
    finally:
        Environment.MAZE_CONFIG.pop(name, None)


def test_evaluate_on_a_forage_maze_matches_the_host_model():
    """Evaluate(maze=name) on a no_goal config: rewards / terminals of every step agree with the host model replaying the
    device's actions; pickups_per_episode is the mean of the first episodes' collections per kind, and success is a first
    episode whose last step collected the melon."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.evaluate import Evaluate
    name = "forage_eval"
    lay = ["-------", "--A-B--", "-C---A-", "---S---", "-B---C-", "--A-B--", "-------"]
    conf = _register(name, lay, random_start=True, max_episode_steps=12, **FORAGE_KW)
    try:
        cfg = _cfg(True, False, 40, 20)
        cfg["action_size"] = 6
        net, _, _, _ = _build(cfg, 1, seed=31, env_name=name)
        B, seed = 32, 0x5EED
        ev = Evaluate(net, batch_size=B, device=DEV, seed=seed, maze=name)
        assert not net.lar_bounded
        log = []
        inner = ev.env.process

        def recording(actions, active, out_reward, out_terminal, **kw):
            inner(actions, active, out_reward, out_terminal, **kw)
            log.append((actions.cpu().numpy().copy(), out_reward.cpu().numpy().copy(), out_terminal.cpu().numpy().copy()))
        ev.env.process = recording
        res = ev.process(0, one_episode_per_actor=True)
        hosts = FM.host_batch(conf, B, seed=seed)
        for h in hosts:
            h.reset()
        first = [None] * B
        start = [list(h.totals) for h in hosts]
        for step, (acts, rew, term) in enumerate(log):
            for b, h in enumerate(hosts):
                _, r, t, _ = h.process(acts[b])
                assert (float(r), int(t)) == (float(rew[b]), int(term[b])), (step, b)
                if t:
                    assert h.ended_by_pickup == (h.picked == 2) and (h.ended_by_pickup or h.ep_steps == 12)
                    if first[b] is None:
                        first[b] = ([now - was for now, was in zip(h.totals, start[b])], h.picked == 2)
                    start[b] = list(h.totals)
                    h.reset()
        assert None not in first
        n_succ = sum(won for _, won in first)
        assert res["episodes"] == B and res["timeouts"] == B - n_succ
        assert abs(res["success_rate"] - n_succ / float(B)) < 1e-12
        want = np.mean([k for k, _ in first], 0)
        assert len(res["pickups_per_episode"]) == 4 and np.abs(np.array(res["pickups_per_episode"]) - want).max() < 1e-12
        assert abs(res["apples_per_episode"] - want[0]) < 1e-12 and res["goals_per_episode"] == 0
        assert 0 < n_succ < B and (want[:3] > 0).all() and want[3] == 0, first
    finally:
        Environment.MAZE_CONFIG.pop(name, None)


def test_batch1_environment_on_a_forage_maze():
    """Environment.create_environment('maze', name) on a forage config with a goal: images, rewards, terminals and pixel
    change of the host model (no reset on terminal: the caller resets)."""
    from unreal_amd.environment.environment import Environment
    name = "forage_batch1"
    lay = ["-------", "--A-B--", "-C---A-", "---G---", "-B---C-", "--A-B--", "-------"]
    kw = dict(FORAGE_KW, no_goal=False)
    conf = _register(name, lay, random_start=True, max_episode_steps=15, goal_respawn=True, goal_reward=10,
                     show_goal=True, **kw)
    try:
        env = Environment.create_environment("maze", name)
        host = FM.HostForageMaze(conf, 0, 1, seed=0)
        host.reset()
        np.testing.assert_array_equal(env.last_state["image"], host.last_state["image"])
        rs = np.random.RandomState(2)
        n_term, picked = 0, set()
        for step in range(150):
            a = int(rs.randint(0, 6))
            image, reward, terminal, pc = env.process(a)
            _, r, t, pc_h = host.process(a)
            np.testing.assert_array_equal(image, host.last_state["image"], err_msg=str(step))
            assert (reward, terminal) == (r, t), step
            np.testing.assert_array_equal(pc, pc_h, err_msg=str(step))
            picked.add(host.picked)
            if terminal:
                n_term += 1
                env.reset()
                host.reset()
                np.testing.assert_array_equal(env.last_state["image"], host.last_state["image"])
        assert n_term > 0 and picked >= {0, 1, 2}
    finally:
        Environment.MAZE_CONFIG.pop(name, None)
