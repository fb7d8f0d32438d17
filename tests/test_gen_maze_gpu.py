"""Generated first-person mazes on the device (maze.hip, a block with the GENERATED flag), bit for bit
against the host model of tests/gen_maze_model.py: records, frames, steps through many resets, views, the fused paths, a
launch with the wrong view, OracleTrainer, Evaluate and the batch-1 environment."""
import numpy as np
import pytest
import torch

try:
    import gen_maze_model as GM
    import maze_model as MM
except ImportError:            # imported as tests.<module>
    from tests import gen_maze_model as GM
    from tests import maze_model as MM
try:
    from test_trainer_gpu import _cfg, _build, _feed_draws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL
    from test_maze_config_gpu import RING_ARRAYS, CFG_ARRAYS
    from test_fp_maze_gpu import _env, _current_frames, _rollout_state
except ImportError:
    from tests.test_trainer_gpu import _cfg, _build, _feed_draws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL
    from tests.test_maze_config_gpu import RING_ARRAYS, CFG_ARRAYS
    from tests.test_fp_maze_gpu import _env, _current_frames, _rollout_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB, PC = 21168, 400
GEN_ARRAYS = RING_ARRAYS + CFG_ARRAYS + ("gen",)
SIZES = (7, 12, 14, 21)


def _config(N, **kw):
    from unreal_amd.environment.maze_environment import MazeConfig
    return MazeConfig(None, random_start=True, random_goal=True, view="first_person", generate=N, **kw)


def _hosts(cfg, B, seed, **kw):
    """Host models of an environment built by _env: its constructor and _env each reset once (episode 1)."""
    models = GM.host_batch(cfg, B, seed=seed, **kw)
    for m in models:
        m.reset()
    return models


def _words(N):
    return 8 + 18 + N * N + 65


def _check_state(env, models, what, count=None):
    ring, B, N = env.ring, len(models), env.config.N
    if count is not None:
        np.testing.assert_array_equal(ring.count.cpu().numpy(), count, err_msg=what)
    rec = ring.gen.cpu().numpy().reshape(B, _words(N))
    want = np.stack([m.actor_record() for m in models])
    bad = np.flatnonzero((rec != want).any(1))
    assert not len(bad), "%s: records of actors %s differ (first words %s)" % (
        what, bad[:8], np.flatnonzero(rec[bad[0]] != want[bad[0]])[:8])
    np.testing.assert_array_equal(ring.pos.cpu().numpy().reshape(B, 2), [(m.x, m.y) for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.heading.cpu().numpy(), [m.h for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.goal.cpu().numpy().reshape(B, 2), [(m.gx, m.gy) for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.ep_steps.cpu().numpy(), [m.ep_steps for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.episode.cpu().numpy(), [m.episode for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.last_action.cpu().numpy(), [m.last_action for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.last_reward.cpu().numpy(), np.array([m.last_reward for m in models], np.float32),
                                  err_msg=what)
    got = _current_frames(ring)
    want = np.stack([m.frame.reshape(-1) for m in models])
    bad = np.flatnonzero((got != want).any(1))
    assert not len(bad), "%s: frames of actors %s differ" % (what, bad[:8])


# every N at every batch size; loops and apples, fixed and drawn headings, the goal shown or not
RESET_CASES = [(N, B) for N in SIZES for B in (3, 64, 512, 4096)]
RESET_KW = {7: dict(gen_loops=2, gen_apples=5, show_goal=True), 12: dict(show_goal=True, start_heading=1),
            14: dict(gen_loops=9, gen_apples=30, apple_reward=3), 21: dict(gen_loops=5, gen_apples=64, show_goal=True)}


@pytest.mark.parametrize("N,B", RESET_CASES)
def test_reset_records_and_frames_match_the_host_model(N, B):
    """The record (walls, free list, apples) and the first observation of every actor, with cell, heading and goal; then
    a masked reset, which regenerates the masked actors only; current_layouts reads the records back."""
    seed = 0x6E4 + N + B
    cfg = _config(N, **RESET_KW[N])
    env = _env(B, 2, cfg, seed=seed)
    models = _hosts(cfg, B, seed)
    _check_state(env, models, "reset")
    before = env.ring.gen.clone().view(B, -1)
    mask = np.random.RandomState(B).uniform(size=B) < 0.5
    env.reset(torch.from_numpy(mask.astype(np.int32)).to(DEV))
    for b in np.flatnonzero(mask):
        models[b].reset()
    _check_state(env, models, "masked reset")
    after = env.ring.gen.view(B, -1)
    keep = torch.from_numpy(~mask).to(DEV)
    assert torch.equal(before[keep], after[keep])
    walls, apples = env.current_layouts()
    assert walls.shape == (B, N, N) and walls.dtype == bool
    for b in (0, B // 2, B - 1):
        np.testing.assert_array_equal(walls[b].reshape(-1), models[b].config.walls[0])
        np.testing.assert_array_equal(apples[b], models[b].config.apples[0])
        assert cfg.generated_layout(seed, b, models[b].episode) == GM.layout_string(models[b].config.walls[0],
                                                                                   models[b].config.apples[0])


# (plain: no navigation option) and navigation with both action sets, both reward sets, respawn on and off
STEP_MODES = {"plain": dict(gen_loops=1),
              "nav_lab": dict(gen_loops=3, gen_apples=12, goal_reward=10, apple_reward=1, hit_reward=0, goal_respawn=True,
                              action_set="lab"),
              "nav_turn": dict(gen_apples=9, apple_reward=2)}
STEP_CASES = [(7, "plain"), (7, "nav_lab"), (12, "plain"), (12, "nav_turn"), (14, "plain"), (14, "nav_lab"),
              (21, "plain"), (21, "nav_lab"), (21, "nav_turn")]


@pytest.mark.parametrize("N,mode", STEP_CASES)
def test_random_steps_through_many_resets_match_the_host_model(N, mode):
    """200 actors, a step limit of 17, 120 random actions with a masked reset half way: every actor passes through at
    least six resets.  Frames, pixel change, rewards, terminals, cells, headings, counters and the whole per-actor
    record at every step; a layout changes at a reset and at nothing else (respawns included)."""
    B, H, steps, seed = 200, 3, 120, 0x9E4 + N
    H1 = H + 1
    kw = dict(STEP_MODES[mode])
    cfg = _config(N, show_goal=True, max_episode_steps=17, **kw)
    A = cfg.action_size
    env = _env(B, H, cfg, seed=seed)
    ring = env.ring
    models = _hosts(cfg, B, seed)
    rs = np.random.RandomState(N)
    out_r = torch.zeros(B, dtype=torch.float32, device=DEV)
    out_t = torch.zeros(B, dtype=torch.int32, device=DEV)
    committed_terminal = np.zeros(B, dtype=bool)
    count = np.zeros(B, dtype=np.int64)
    n = dict(goal=0, timeout=0, hit=0, apple=0, respawn=0, resets=0, changed=0)
    resets = np.zeros(B, dtype=np.int64)
    _check_state(env, models, "after reset", count)
    for step in range(steps):
        acts = rs.randint(0, A, B).astype(np.int32)
        layouts = [m.config.walls[0] for m in models]
        env.process(torch.from_numpy(acts).to(DEV), None, out_r, out_t, reset_on_terminal=True, track_score=True)
        want_r, want_t, want_pc = [], [], []
        for b, m in enumerate(models):
            _, r, t, pc = m.process(acts[b])
            want_r.append(r); want_t.append(t); want_pc.append(pc)
            n["goal"] += getattr(m, "at_goal", bool(t and not m.timed_out))
            n["timeout"] += m.timed_out
            n["hit"] += getattr(m, "hit", r < 0)
            n["apple"] += getattr(m, "apple", False)
            n["respawn"] += getattr(m, "respawned", False)
            assert m.config.walls[0] is layouts[b]
            if t:
                m.reset()
                resets[b] += 1
                n["resets"] += 1
                n["changed"] += not np.array_equal(m.config.walls[0], layouts[b])
        np.testing.assert_array_equal(out_r.cpu().numpy(), np.array(want_r, dtype=np.float32), err_msg=str(step))
        term = np.array(want_t, dtype=bool)
        np.testing.assert_array_equal(out_t.cpu().numpy(), term.astype(np.int32), err_msg=str(step))
        old = count.copy()
        discard = term & (old > 0) & committed_terminal
        count = np.where(discard, old, old + 1)
        committed_terminal = np.where(discard, committed_terminal, term)
        _check_state(env, models, "step %d" % step, count)
        base = np.arange(B) * H1 + old % H1
        pc_dev = ring.r_pc.view(-1, PC)[torch.from_numpy(base).to(DEV)].cpu().numpy()
        np.testing.assert_array_equal(pc_dev, np.stack(want_pc).reshape(B, PC), err_msg=str(step))
        if step == steps // 2:
            mask = rs.uniform(size=B) < 0.5
            env.reset(torch.from_numpy(mask.astype(np.int32)).to(DEV))
            for b in np.flatnonzero(mask):
                models[b].reset()
            _check_state(env, models, "masked reset", count)
    assert resets.min() >= 6, resets.min()
    assert n["goal"] > 0 and n["timeout"] > 0 and n["hit"] > 0, n
    if cfg.nav:
        assert n["apple"] > 0, n
    assert n["respawn"] > 0 or not cfg.goal_respawn, n
    # (at N = 7 two episodes of an actor can draw the same of ~10^5 trees; above, never in a run of this size)
    assert n["changed"] == n["resets"] if N > 7 else n["changed"] > 0.97 * n["resets"], n


@pytest.mark.parametrize("N", [7, 21])
def test_two_half_batch_views_equal_the_whole_batch(N):
    """view(0, cut) and view(cut, B) of one environment stepped one after the other == another environment stepped
    whole, array for array, through resets (the views' records are slices of the ring's)."""
    B, H, cut = 130, 3, 47
    cfg = _config(N, gen_loops=2, gen_apples=6, show_goal=True, max_episode_steps=6, action_set="lab")
    whole, split = _env(B, H, cfg, seed=21), _env(B, H, cfg, seed=21)
    views = [split.view(0, cut), split.view(cut, B)]
    assert views[1].ring.gen.data_ptr() == split.ring.gen.data_ptr() + 4 * cut * _words(N)
    for v in views:                       # a masked reset through the views
        m = torch.ones(v.B, dtype=torch.int32, device=DEV)
        v.reset(m)
    whole.reset()
    rs = np.random.RandomState(N)
    z = lambda dt: torch.zeros(B, dtype=dt, device=DEV)
    r0, t0, r1, t1 = z(torch.float32), z(torch.int32), z(torch.float32), z(torch.int32)
    for step in range(25):
        a = torch.from_numpy(rs.randint(0, 6, B).astype(np.int32)).to(DEV)
        whole.process(a, None, r0, t0, track_score=True)
        for v, (b0, b1) in zip(views, ((0, cut), (cut, B))):
            v.process(a[b0:b1], None, r1[b0:b1], t1[b0:b1], track_score=True)
        assert torch.equal(r0, r1) and torch.equal(t0, t1), step
        for name in GEN_ARRAYS:
            assert torch.equal(getattr(whole.ring, name), getattr(split.ring, name)), (step, name)
    assert int(whole.ring.episode.min()) >= 4


@pytest.mark.parametrize("B,A", [(64, 4), (300, 6)])
def test_fused_rollout_steps_are_the_two_launch_paths(B, A):
    """On two views of each environment: rollout_step == process + rollout_advance (+ cur_idx and the LSTM-input
    columns), and policy_rollout_step == policy_step + rollout_step, bit for bit, at A = 4 and A = 6, with resets
    regenerating layouts on the way."""
    from unreal_amd import ops
    H, xld = 4, 264
    rs = np.random.RandomState(B)
    dev = lambda a, dt: torch.from_numpy(np.asarray(a)).to(DEV, dt)
    Wp = dev(rs.uniform(-.3, .3, 256 * A), torch.float32); bp = dev(rs.uniform(-.1, .1, A), torch.float32)
    Wv = dev(rs.uniform(-.3, .3, 256), torch.float32); bv = dev(rs.uniform(-.1, .1, 1), torch.float32)
    kw = dict(gen_apples=8, goal_reward=10, hit_reward=0, goal_respawn=True, action_set="lab") if A == 6 else \
        dict(gen_loops=2)
    cfg = _config(12 if A == 6 else 7, show_goal=True, max_episode_steps=5, **kw)
    assert cfg.action_size == A
    envs = [_env(B, H, cfg, seed=9) for _ in range(3)]
    cut = B // 3
    views = [[e.view(0, cut), e.view(cut, B)] for e in envs]
    st = [_rollout_state(B, xld) for _ in envs]
    for s in st:
        s["pi"] = torch.zeros(B * A, dtype=torch.float32, device=DEV)
    n_term = 0
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
        for name in GEN_ARRAYS:
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
        n_term += int(st[0]["te"].sum())
        if step in (4, 8):
            for s in st:
                s["active"].fill_(1); s["te"].zero_(); s["n"].zero_()
    assert n_term > 0 and int(envs[0].ring.episode.max()) >= 2
    assert set(st[0]["a"].cpu().numpy().tolist()) >= set(range(A))


def test_a_launch_with_the_wrong_view_writes_nothing():
    """A first-person or top-down launch on a generated block, and a generated launch on a static block: the kernels
    return before any store, as for a block of another grid size."""
    from unreal_amd import ops
    from unreal_amd.environment.maze_environment import MazeConfig
    B, H, N = 16, 2, 7
    dev = torch.device(DEV)
    gen_block = torch.from_numpy(_config(N, gen_loops=1).block(3)).to(dev)
    static = MazeConfig([MM.random_layout(N, np.random.RandomState(1))], True, True, view="first_person")
    static_block = torch.from_numpy(static.block(3)).to(dev)
    cases = [(ops.MAZE_FIRST_PERSON, gen_block, 0), (ops.MAZE_TOP_DOWN, gen_block, 0),
             (ops.MAZE_FIRST_PERSON_GENERATED, static_block, N)]
    for view, block, gen in cases:
        ring = ops.Ring(B, H, dev, maze_state=True, gen=gen)
        ring.frames.fill_(7); ring.r_pc.fill_(-1.0); ring.pos.fill_(1); ring.goal.fill_(2)
        if gen:
            ring.gen.fill_(5)
        names = RING_ARRAYS + CFG_ARRAYS + ("heading",) + (("gen",) if gen else ())
        before = {n: getattr(ring, n).clone() for n in names}
        maze = (view, N, block, 0)
        acts = torch.ones(B, dtype=torch.int32, device=dev)
        out_r = torch.full((B,), -5.0, device=dev)
        out_t = torch.full((B,), -5, dtype=torch.int32, device=dev)
        ops.maze_reset(ring, None, maze=maze)
        ops.maze_step(ring, acts, None, out_r, out_t, True, True, maze=maze)
        torch.cuda.synchronize()
        for n, t in before.items():
            assert torch.equal(getattr(ring, n), t), (view, n)
        assert (out_r == -5.0).all() and (out_t == -5).all()
    ring = ops.Ring(B, H, dev, maze_state=True)                 # no per-actor records: refused before the launch
    with pytest.raises(ValueError):
        ops.maze_reset(ring, None, maze=(ops.MAZE_FIRST_PERSON_GENERATED, N, gen_block, 0))


def _register(name, N, **kw):
    from unreal_amd.environment.environment import Environment
    Environment.register_maze_config(name, None, random_start=True, random_goal=True, view="first_person", generate=N,
                                     **kw)
    return Environment.MAZE_CONFIG[name]


# full UNREAL at A = 4 without navigation options; FF at A = 6 on a navigation maze (rewards 10 / 1 / 0, respawn)
TRAINER_CASES = [(True, True, 4, dict(gen_loops=2, show_goal=True, max_episode_steps=7)),
                 (True, True, 6, dict(gen_apples=6, goal_reward=10, apple_reward=1, hit_reward=0, action_set="lab",
                                      goal_respawn=True, show_goal=True, max_episode_steps=7)),
                 (False, False, 6, dict(gen_apples=6, action_set="lab", max_episode_steps=5))]


@pytest.mark.parametrize("use_lstm,aux,A,kw", TRAINER_CASES)
def test_process_on_a_generated_maze_matches_oracle(use_lstm, aux, A, kw):
    """Trainer.process against OracleTrainer with one host model per actor, at the bars of
    test_process_on_a_first_person_maze_matches_oracle: every actor meets new layouts during the run."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.maze_environment import FirstPersonMazeEnvironment
    from oracle.trainer import OracleTrainer, ExplicitDraws
    name = "gen_train_%d%d%d" % (use_lstm, aux, A)
    conf = _register(name, 7, **kw)
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(use_lstm, aux, H, T)
        cfg["action_size"] = A
        cfg["initial_learning_rate"] = 7.0711e-4
        net, applier, tr, draws = _build(cfg, B, seed=3, env_name=name)
        assert isinstance(tr.environment, FirstPersonMazeEnvironment) and tr.action_size == A
        assert tr.environment.maze[0] == 2
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = GM.host_batch(conf, B, seed=tr.seed)
        orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=hosts)
        while not tr._full:
            tr.process(None, 0)
        for step_u in draws.log:
            for b in range(B):
                edraws[b].action_u.append(float(step_u[b]))
        orc.fill()
        records = lambda: tr.ring.gen.cpu().numpy().reshape(B, -1)
        np.testing.assert_array_equal(tr.ring.count.cpu().numpy(), [a.exp.count for a in orc.actors])
        np.testing.assert_array_equal(records(), [h.actor_record() for h in hosts])
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
            np.testing.assert_array_equal(records(), [h.actor_record() for h in hosts])
        assert min(h.episode for h in hosts) >= 3
    finally:
        Environment.MAZE_CONFIG.pop(name, None)
        Environment.action_size = -1


def _evaluate(name, conf, net, B, seed):
    from unreal_amd.evaluate import Evaluate
    ev = Evaluate(net, batch_size=B, device=DEV, seed=seed, maze=name)
    log = []
    inner = ev.env.process

    def recording(actions, active, out_reward, out_terminal, **kw):
        inner(actions, active, out_reward, out_terminal, **kw)
        log.append((actions.cpu().numpy().copy(), out_reward.cpu().numpy().copy(), out_terminal.cpu().numpy().copy()))
    ev.env.process = recording
    first_layouts = None

    inner_reset = ev.env.reset

    def reset(mask=None):
        nonlocal first_layouts
        inner_reset(mask)
        if first_layouts is None:
            first_layouts = ev.env.current_layouts()[0].copy()
    ev.env.reset = reset
    res = ev.process(0, one_episode_per_actor=True)
    hosts = GM.host_batch(conf, B, seed=seed)
    for h in hosts:
        h.reset()                  # Evaluate.process: self.env.reset()
    np.testing.assert_array_equal(first_layouts.reshape(B, -1), [h.config.walls[0] for h in hosts])
    first = [None] * B
    for step, (acts, rew, term) in enumerate(log):
        for b, h in enumerate(hosts):
            g0, a0 = h.goals_total, h.apples_total
            _, r, t, _ = h.process(acts[b])
            assert (float(r), int(t)) == (float(rew[b]), int(term[b])), (step, b)
            h.ep_goals = getattr(h, "ep_goals", 0) + h.goals_total - g0
            h.ep_apples = getattr(h, "ep_apples", 0) + h.apples_total - a0
            if t:
                if first[b] is None:
                    first[b] = (h.ep_goals, h.ep_apples)
                h.ep_goals = h.ep_apples = 0
                h.reset()
    assert None not in first
    goals = [g for g, _ in first]
    apples = [a for _, a in first]
    n_succ = sum(g > 0 for g in goals)
    assert res["episodes"] == B and res["timeouts"] == B - n_succ
    assert abs(res["success_rate"] - n_succ / float(B)) < 1e-12
    assert abs(res["goals_per_episode"] - np.mean(goals)) < 1e-12
    assert abs(res["apples_per_episode"] - np.mean(apples)) < 1e-12
    return first_layouts, first


def test_evaluate_with_two_seeds_sees_different_layouts_and_matches_the_host_model():
    """Evaluate(maze=name, seed=...) on a generated navigation maze: per-actor rewards / terminals of every step and the
    first episodes' outcomes are the host model's, for two seeds whose layouts differ."""
    from unreal_amd.environment.environment import Environment
    name = "gen_eval"
    conf = _register(name, 7, gen_loops=4, gen_apples=8, goal_reward=10, apple_reward=1, hit_reward=0,
                     action_set="lab", goal_respawn=True, show_goal=True, max_episode_steps=30)
    try:
        cfg = _cfg(True, False, 40, 20)
        cfg["action_size"] = 6
        net, _, _, _ = _build(cfg, 1, seed=31, env_name=name)
        B = 32
        lay_a, first_a = _evaluate(name, conf, net, B, 0x5EED)
        lay_b, first_b = _evaluate(name, conf, net, B, 0x5EED + 1)
        assert all(not np.array_equal(lay_a[b], lay_b[b]) for b in range(B))
        assert sum(a for _, a in first_a + first_b) > 0, (first_a, first_b)
    finally:
        Environment.MAZE_CONFIG.pop(name, None)
        Environment.action_size = -1


def test_batch1_environment_on_a_generated_maze():
    """Environment.create_environment('maze', name) on a generated config: images, rewards, terminals and pixel change
    of the host model (no reset on terminal: the caller resets, and gets a new layout)."""
    from unreal_amd.environment.environment import Environment
    name = "gen_batch1"
    conf = _register(name, 12, gen_loops=3, gen_apples=10, goal_reward=10, hit_reward=0, action_set="lab",
                     goal_respawn=True, show_goal=True, max_episode_steps=15)
    try:
        assert Environment.get_action_size("maze", name) == 6
        env = Environment.create_environment("maze", name)
        host = GM.host_batch(conf, 1, seed=0)[0]
        host.reset()                   # (MazeEnvironment's constructor resets twice: its batched environment's, its own)
        np.testing.assert_array_equal(env.last_state["image"], host.last_state["image"])
        rs = np.random.RandomState(2)
        n_term = 0
        layouts = set()
        for step in range(150):
            a = int(rs.randint(0, 6))
            image, reward, terminal, pc = env.process(a)
            _, r, t, pc_h = host.process(a)
            np.testing.assert_array_equal(image, host.last_state["image"], err_msg=str(step))
            assert (reward, terminal) == (r, t), step
            np.testing.assert_array_equal(pc, pc_h, err_msg=str(step))
            if terminal:
                n_term += 1
                env.reset()
                host.reset()
                np.testing.assert_array_equal(env.last_state["image"], host.last_state["image"])
                layouts.add(env._env.current_layouts()[0].tobytes())
        assert n_term == 10 and len(layouts) == 10
    finally:
        Environment.MAZE_CONFIG.pop(name, None)
        Environment.action_size = -1
