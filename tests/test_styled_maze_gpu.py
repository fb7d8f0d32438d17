"""Styled first-person walls and landmarks on the device (maze.hip, a block with the STYLED flag), bit for
bit against the host model of tests/styled_maze_model.py: reset frames and style ids, steps through many resets, the
fused paths, views, OracleTrainer, Evaluate and the batch-1 environment, on static and generated configs."""
import numpy as np
import pytest
import torch

try:
    import maze_model as MM
    import styled_maze_model as SM
except ImportError:            # imported as tests.<module>
    from tests import maze_model as MM
    from tests import styled_maze_model as SM
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
SIZES = (7, 12, 14, 21)
# all seven styles; the patterns none, all, alternating, half; a colour whose bytes are the plain floor's
STYLES = [(200, 100, 50, 0xAA), (0, 255, 0, 0x00), (255, 255, 255, 0xFF), (10, 20, 250, 0x0F), (40, 40, 40, 0x81),
          (255, 0, 255, 0x3C), (1, 2, 3, 0x55)]
APPLES = {7: 6, 12: 20, 14: 30, 21: 64}


def _layout(N, rs, marks=""):
    """A random layout most of whose wall cells carry a digit 1..7."""
    cells = list(MM.random_layout(N, rs, marks=marks))
    for c, ch in enumerate(cells):
        k = rs.randint(0, 10)
        if ch == "+" and 1 <= k <= 7:
            cells[c] = str(k)
    return "".join(cells)


def _static(N, L=7, seed=0, nav=False, **kw):
    from unreal_amd.environment.maze_environment import MazeConfig
    rs = np.random.RandomState(seed + N)
    marks = kw.pop("marks", "") + ("A" * APPLES[N] if nav else "")
    lays = [_layout(N, rs, marks=marks) for _ in range(L)]
    return MazeConfig(lays, view="first_person", wall_styles=STYLES, **kw)


def _generated(N, density=64, styles=STYLES, **kw):
    from unreal_amd.environment.maze_environment import MazeConfig
    return MazeConfig(None, random_start=True, random_goal=True, view="first_person", generate=N, wall_styles=styles,
                      gen_landmark_density=density, **kw)


def _hosts(cfg, B, seed, **kw):
    """Host models of an environment built by _env: its constructor and _env each reset once (episode 1)."""
    models = SM.host_batch(cfg, B, seed=seed, **kw)
    for m in models:
        m.reset()
    return models


def _arrays(cfg):
    return RING_ARRAYS + CFG_ARRAYS + (("gen",) if cfg.generate is not None else ("nav",) if cfg.nav else ("heading",))


def _check_state(env, models, what, count=None):
    ring, B, cfg = env.ring, len(models), env.config
    if count is not None:
        np.testing.assert_array_equal(ring.count.cpu().numpy(), count, err_msg=what)
    if cfg.generate is not None:
        rec = ring.gen.cpu().numpy().reshape(B, -1)
        want = np.stack([m.actor_record() for m in models])
        assert rec.shape == want.shape
        bad = np.flatnonzero((rec != want).any(1))
        assert not len(bad), "%s: records of actors %s differ (first words %s)" % (
            what, bad[:8], np.flatnonzero(rec[bad[0]] != want[bad[0]])[:8])
    elif cfg.nav:
        np.testing.assert_array_equal(ring.nav.cpu().numpy().reshape(B, 8), [m.record() for m in models], err_msg=what)
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


def _check_styles(env, models):
    N = env.config.N
    ids = env.current_styles()
    assert ids.shape == (len(models), N, N) and ids.dtype == np.uint8
    np.testing.assert_array_equal(ids.reshape(len(models), -1), np.stack([m.style_ids() for m in models]))


RESET_KW = {7: dict(gen_loops=2, gen_apples=5, show_goal=True), 12: dict(show_goal=True, start_heading=1),
            14: dict(gen_loops=9, gen_apples=30, apple_reward=3), 21: dict(gen_loops=5, gen_apples=64, show_goal=True)}


@pytest.mark.parametrize("kind", ["static", "generated"])
@pytest.mark.parametrize("N,B", [(N, B) for N in SIZES for B in (3, 64, 512)])
def test_reset_frames_and_styles_match_the_host_model(N, B, kind):
    """The first observation of every actor and current_styles(), then a masked reset.  Static: 7 layouts with digits,
    all 7 styles; generated: landmark density 64, and 256 (every wall cell a landmark) at B = 64.  N = 14 and 21 end in a
    partly filled nibble word."""
    seed = 0x57E + N + B
    if kind == "static":
        cfg = _static(N, L=7, seed=B, marks="SG", random_start=B != 64, random_goal=True, show_goal=True,
                      start_heading=None if N != 12 else 2)
    else:
        cfg = _generated(N, density=256 if B == 64 else 64, **RESET_KW[N])
    env = _env(B, 2, cfg, seed=seed)
    models = _hosts(cfg, B, seed)
    _check_state(env, models, "reset")
    _check_styles(env, models)
    styled = sum(int(m.style_ids().any()) for m in models)
    assert styled == B if kind == "static" or B == 64 or N > 7 else styled > 0
    mask = np.random.RandomState(B).uniform(size=B) < 0.5
    env.reset(torch.from_numpy(mask.astype(np.int32)).to(DEV))
    for b in np.flatnonzero(mask):
        models[b].reset()
    _check_state(env, models, "masked reset")
    _check_styles(env, models)
    if kind == "generated":
        walls, _ = env.current_layouts()                 # (unchanged by the longer record)
        np.testing.assert_array_equal(walls.reshape(B, -1), np.stack([m.config.walls[0] for m in models]))
        lay = cfg.generated_layout(seed, B - 1, models[-1].episode)
        assert lay == SM.layout_string(models[-1].config.walls[0], models[-1].config.apples[0], models[-1].style_ids())


NAV_KW = dict(goal_reward=10, apple_reward=1, hit_reward=0, goal_respawn=True, action_set="lab")


def _step_config(N, mode):
    kw = dict(random_start=True, random_goal=True, show_goal=True, max_episode_steps=17)
    if mode == "plain":
        return _static(N, L=7, seed=N, **kw)
    if mode == "nav":
        return _static(N, L=7, seed=N, nav=True, **dict(kw, **NAV_KW))
    return _generated(N, density=96, gen_loops=3, gen_apples=APPLES[N] // 2, show_goal=True, max_episode_steps=17,
                      **NAV_KW)


@pytest.mark.parametrize("mode", ["plain", "nav", "generated"])
@pytest.mark.parametrize("N", SIZES)
def test_random_steps_match_the_host_model(N, mode):
    """200 actors, a step limit of 17, 120 random actions with a masked reset half way: frames, pixel change (bit for
    bit, and equal to unreal_pixel_change_u8 on the two stored frames), rewards, terminals, cells, headings, counters
    and records at every step, on a plain static config, a navigation config (Lab's actions, respawn, apples) and a
    generated one with loops and apples."""
    from unreal_amd import ops
    B, H, steps, seed = 200, 3, 120, 0x57E9 + N
    H1 = H + 1
    cfg = _step_config(N, mode)
    A = cfg.action_size
    env = _env(B, H, cfg, seed=seed)
    ring = env.ring
    models = _hosts(cfg, B, seed)
    rs = np.random.RandomState(N)
    out_r = torch.zeros(B, dtype=torch.float32, device=DEV)
    out_t = torch.zeros(B, dtype=torch.int32, device=DEV)
    pc_u8 = torch.zeros(B * PC, dtype=torch.float32, device=DEV)
    committed_terminal = np.zeros(B, dtype=bool)
    count = np.zeros(B, dtype=np.int64)
    n = dict(goal=0, timeout=0, hit=0, apple=0, respawn=0, styled=0)
    _check_state(env, models, "after reset", count)
    for step in range(steps):
        acts = rs.randint(0, A, B).astype(np.int32)
        env.process(torch.from_numpy(acts).to(DEV), None, out_r, out_t, reset_on_terminal=True, track_score=True)
        want_r, want_t, want_pc = [], [], []
        for b, m in enumerate(models):
            plain_frame = super(SM._Styled, m)._render
            _, r, t, pc = m.process(acts[b])
            want_r.append(r); want_t.append(t); want_pc.append(pc)
            n["goal"] += getattr(m, "at_goal", bool(t and not m.timed_out))
            n["timeout"] += m.timed_out
            n["hit"] += getattr(m, "hit", r < 0)
            n["apple"] += getattr(m, "apple", False)
            n["respawn"] += getattr(m, "respawned", False)
            n["styled"] += not np.array_equal(m.frame, plain_frame())
            if t:
                m.reset()
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
        live = np.flatnonzero(~term)
        if len(live):
            idx_new = torch.from_numpy((live * H1 + count[live] % H1).astype(np.int32)).to(DEV)
            idx_old = torch.from_numpy((live * H1 + old[live] % H1).astype(np.int32)).to(DEV)
            ops.pixel_change_u8(ring.frames, idx_new, idx_old, 48.0 * 255.0, pc_u8[:len(live) * PC])
            np.testing.assert_array_equal(pc_u8[:len(live) * PC].cpu().numpy().reshape(-1, PC), pc_dev[live])
        if step == steps // 2:
            mask = rs.uniform(size=B) < 0.5
            env.reset(torch.from_numpy(mask.astype(np.int32)).to(DEV))
            for b in np.flatnonzero(mask):
                models[b].reset()
            _check_state(env, models, "masked reset", count)
            _check_styles(env, models)
    assert n["goal"] > 0 and n["timeout"] > 0 and n["hit"] > 0, n
    assert n["styled"] > B * steps // 4, n               # the styled path was looked at
    if cfg.nav:
        assert n["apple"] > 0 and n["respawn"] > 0, n


@pytest.mark.parametrize("N,kind", [(7, "static"), (21, "generated")])
def test_two_half_batch_views_equal_the_whole_batch(N, kind):
    """view(0, cut) and view(cut, B) of one environment stepped one after the other == another environment stepped
    whole, array for array, through resets (a generated view's records are slices of the longer styled records)."""
    B, H, cut = 130, 3, 47
    if kind == "static":
        cfg = _static(N, L=5, nav=True, random_start=True, random_goal=True, show_goal=True, max_episode_steps=6,
                      action_set="lab")
    else:
        cfg = _generated(N, gen_loops=2, gen_apples=6, show_goal=True, max_episode_steps=6, action_set="lab")
    whole, split = _env(B, H, cfg, seed=21), _env(B, H, cfg, seed=21)
    views = [split.view(0, cut), split.view(cut, B)]
    if kind == "generated":
        words = 8 + 18 + N * N + 65 + (N * N + 7) // 8
        assert views[1].ring.gen.data_ptr() == split.ring.gen.data_ptr() + 4 * cut * words
    for v in views:                       # a masked reset through the views
        v.reset(torch.ones(v.B, dtype=torch.int32, device=DEV))
    whole.reset()
    np.testing.assert_array_equal(np.concatenate([v.current_styles() for v in views]), whole.current_styles())
    rs = np.random.RandomState(N)
    z = lambda dt: torch.zeros(B, dtype=dt, device=DEV)
    r0, t0, r1, t1 = z(torch.float32), z(torch.int32), z(torch.float32), z(torch.int32)
    for step in range(25):
        a = torch.from_numpy(rs.randint(0, 6, B).astype(np.int32)).to(DEV)
        whole.process(a, None, r0, t0, track_score=True)
        for v, (b0, b1) in zip(views, ((0, cut), (cut, B))):
            v.process(a[b0:b1], None, r1[b0:b1], t1[b0:b1], track_score=True)
        assert torch.equal(r0, r1) and torch.equal(t0, t1), step
        for name in _arrays(cfg):
            assert torch.equal(getattr(whole.ring, name), getattr(split.ring, name)), (step, name)
    assert int(whole.ring.episode.min()) >= 4


@pytest.mark.parametrize("B,A", [(64, 4), (300, 6)])
def test_fused_rollout_steps_are_the_two_launch_paths(B, A):
    """On two views of each environment: rollout_step == process + rollout_advance (+ cur_idx and the LSTM-input
    columns), and policy_rollout_step == policy_step + rollout_step, bit for bit: A = 4 on a styled generated config,
    A = 6 on a styled static navigation config."""
    from unreal_amd import ops
    H, xld = 4, 264
    rs = np.random.RandomState(B)
    dev = lambda a, dt: torch.from_numpy(np.asarray(a)).to(DEV, dt)
    Wp = dev(rs.uniform(-.3, .3, 256 * A), torch.float32); bp = dev(rs.uniform(-.1, .1, A), torch.float32)
    Wv = dev(rs.uniform(-.3, .3, 256), torch.float32); bv = dev(rs.uniform(-.1, .1, 1), torch.float32)
    if A == 4:
        cfg = _generated(7, density=128, gen_loops=2, show_goal=True, max_episode_steps=5)
    else:
        cfg = _static(12, L=3, nav=True, random_start=True, random_goal=True, show_goal=True, max_episode_steps=5,
                      **NAV_KW)
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
        for name in _arrays(cfg):
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


# a room whose walls carry four styles around the goal; apples and respawn at S as in the navigation tests
STYLED_ROOM = ["+++++++",
               "++123++",
               "+4A-G1+",
               "+3-SA2+",
               "+2A-A3+",
               "++412++",
               "+++++++"]


def _register(name, layouts, **kw):
    from unreal_amd.environment.environment import Environment
    Environment.register_maze_config(name, layouts, view="first_person", wall_styles=STYLES[:4], **kw)
    return Environment.MAZE_CONFIG[name]


# full UNREAL at A = 4 on a styled generated config; FF at A = 6 on a styled navigation config
TRAINER_CASES = [(True, True, 4, None, dict(random_start=True, random_goal=True, generate=7, gen_loops=2,
                                            gen_landmark_density=128, show_goal=True, max_episode_steps=7)),
                 (False, False, 6, [STYLED_ROOM], dict(goal_reward=10, apple_reward=1, hit_reward=0, action_set="lab",
                                                       goal_respawn=True, show_goal=True, max_episode_steps=7))]


@pytest.mark.parametrize("use_lstm,aux,A,layouts,kw", TRAINER_CASES)
def test_process_on_a_styled_maze_matches_oracle(use_lstm, aux, A, layouts, kw):
    """Trainer.process against OracleTrainer with one host model per actor, at the bars of
    test_process_on_a_generated_maze_matches_oracle."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.environment.maze_environment import FirstPersonMazeEnvironment
    from oracle.trainer import OracleTrainer, ExplicitDraws
    name = "styled_train_%d%d%d" % (use_lstm, aux, A)
    conf = _register(name, layouts, **kw)
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(use_lstm, aux, H, T)
        cfg["action_size"] = A
        cfg["initial_learning_rate"] = 7.0711e-4
        net, applier, tr, draws = _build(cfg, B, seed=3, env_name=name)
        assert isinstance(tr.environment, FirstPersonMazeEnvironment) and tr.action_size == A
        assert len(tr.environment.maze) == 5 and tr.environment.maze[0] == (2 if layouts is None else 1)
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = SM.host_batch(conf, B, seed=tr.seed)
        orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=hosts)
        while not tr._full:
            tr.process(None, 0)
        for step_u in draws.log:
            for b in range(B):
                edraws[b].action_u.append(float(step_u[b]))
        orc.fill()
        records = lambda: tr.ring.actor_records.cpu().numpy()
        want_records = lambda: [h.actor_record() if layouts is None else h.record() for h in hosts]
        np.testing.assert_array_equal(tr.ring.count.cpu().numpy(), [a.exp.count for a in orc.actors])
        np.testing.assert_array_equal(records(), want_records())
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
            np.testing.assert_array_equal(records(), want_records())
            np.testing.assert_array_equal(_current_frames(tr.ring), [h.frame.reshape(-1) for h in hosts])
        assert min(h.episode for h in hosts) >= 3
        np.testing.assert_array_equal(tr.environment.current_styles().reshape(B, -1), [h.style_ids() for h in hosts])
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
    first = {}
    inner_reset = ev.env.reset

    def reset(mask=None):
        inner_reset(mask)
        if not first:
            first["styles"] = ev.env.current_styles().copy()
            first["frames"] = _current_frames(ev.env.ring).copy()
    ev.env.reset = reset
    res = ev.process(0, one_episode_per_actor=True)
    hosts = SM.host_batch(conf, B, seed=seed)
    for h in hosts:
        h.reset()                  # Evaluate.process: self.env.reset()
    np.testing.assert_array_equal(first["styles"].reshape(B, -1), [h.style_ids() for h in hosts])
    np.testing.assert_array_equal(first["frames"], [h.frame.reshape(-1) for h in hosts])
    done = [None] * B
    for step, (acts, rew, term) in enumerate(log):
        for b, h in enumerate(hosts):
            g0 = h.goals_total
            _, r, t, _ = h.process(acts[b])
            assert (float(r), int(t)) == (float(rew[b]), int(term[b])), (step, b)
            h.ep_goals = getattr(h, "ep_goals", 0) + h.goals_total - g0
            if t:
                if done[b] is None:
                    done[b] = h.ep_goals
                h.ep_goals = 0
                h.reset()
    assert None not in done
    n_succ = sum(g > 0 for g in done)
    assert res["episodes"] == B and res["timeouts"] == B - n_succ
    assert abs(res["goals_per_episode"] - np.mean(done)) < 1e-12
    return first["styles"]


def test_evaluate_with_two_seeds_sees_different_landmarks_and_matches_the_host_model():
    """Evaluate(maze=name, seed=...) on a styled generated navigation maze: the first frames, the style ids and the
    rewards / terminals of every step are the host model's, for two seeds whose landmarks differ."""
    from unreal_amd.environment.environment import Environment
    name = "styled_eval"
    conf = _register(name, None, random_start=True, random_goal=True, generate=7, gen_loops=4, gen_apples=8,
                     gen_landmark_density=100, goal_reward=10, apple_reward=1, hit_reward=0, action_set="lab",
                     goal_respawn=True, show_goal=True, max_episode_steps=30)
    try:
        cfg = _cfg(True, False, 40, 20)
        cfg["action_size"] = 6
        net, _, _, _ = _build(cfg, 1, seed=31, env_name=name)
        B = 32
        a = _evaluate(name, conf, net, B, 0x5EED)
        b = _evaluate(name, conf, net, B, 0x5EED + 1)
        assert all(not np.array_equal(a[k], b[k]) for k in range(B))
    finally:
        Environment.MAZE_CONFIG.pop(name, None)
        Environment.action_size = -1


@pytest.mark.parametrize("generated", [False, True])
def test_batch1_environment_on_a_styled_maze(generated):
    """Environment.create_environment('maze', name) on a styled config: images, rewards, terminals and pixel change of
    the host model."""
    from unreal_amd.environment.environment import Environment
    name = "styled_batch1"
    kw = dict(goal_reward=10, hit_reward=0, action_set="lab", goal_respawn=True, show_goal=True, max_episode_steps=15)
    if generated:
        conf = _register(name, None, random_start=True, random_goal=True, generate=12, gen_loops=3, gen_apples=10,
                         gen_landmark_density=160, **kw)
    else:
        conf = _register(name, [STYLED_ROOM], **kw)
    try:
        assert Environment.get_action_size("maze", name) == 6
        env = Environment.create_environment("maze", name)
        host = SM.host_batch(conf, 1, seed=0)[0]
        host.reset()                   # (MazeEnvironment's constructor resets twice: its batched environment's, its own)
        np.testing.assert_array_equal(env.last_state["image"], host.last_state["image"])
        rs = np.random.RandomState(2)
        n_term = 0
        for step in range(90):
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
                np.testing.assert_array_equal(env._env.current_styles()[0].reshape(-1), host.style_ids())
        assert n_term == 6
    finally:
        Environment.MAZE_CONFIG.pop(name, None)
        Environment.action_size = -1
