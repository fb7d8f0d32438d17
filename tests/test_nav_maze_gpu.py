"""First-person navigation mazes on the device (maze.hip, a block with the NAV flag) against the host model of
tests/nav_maze_model.py, the two-launch paths, OracleTrainer, Evaluate and the batch-1 environment."""
import numpy as np
import pytest
import torch

try:
    import maze_model as MM
    import nav_maze_model as NM
except ImportError:            # imported as tests.<module>
    from tests import maze_model as MM
    from tests import nav_maze_model as NM
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
NAV_ARRAYS = RING_ARRAYS + CFG_ARRAYS + ("nav",)
APPLES = {7: 6, 12: 20, 14: 30, 21: 64}          # apples per layout


def _config(N, L=5, seed=0, marks="", **kw):
    from unreal_amd.environment.maze_environment import MazeConfig
    rs = np.random.RandomState(seed + N)
    return MazeConfig([MM.random_layout(N, rs, marks=marks + "A" * APPLES[N]) for _ in range(L)], view="first_person",
                      **kw)


def _hosts(cfg, B, seed):
    """Host models of an environment built by _env: its constructor and _env each reset once (episode 1)."""
    models = NM.host_batch(cfg, B, seed=seed)
    for m in models:
        m.reset()
    return models


def _check_state(ring, models, what, count=None):
    B = len(models)
    if count is not None:
        np.testing.assert_array_equal(ring.count.cpu().numpy(), count, err_msg=what)
    np.testing.assert_array_equal(ring.pos.cpu().numpy().reshape(B, 2), [(m.x, m.y) for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.heading.cpu().numpy(), [m.h for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.nav.cpu().numpy().reshape(B, 8), [m.record() for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.goal.cpu().numpy().reshape(B, 2), [(m.gx, m.gy) for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.ep_steps.cpu().numpy(), [m.ep_steps for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.episode.cpu().numpy(), [m.episode for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.last_action.cpu().numpy(), [m.last_action for m in models], err_msg=what)
    np.testing.assert_array_equal(ring.last_reward.cpu().numpy(), np.array([m.last_reward for m in models], np.float32),
                                  err_msg=what)
    want = np.stack([m.frame.reshape(-1) for m in models])
    got = _current_frames(ring)
    bad = np.flatnonzero((got != want).any(1))
    assert not len(bad), "%s: frames of actors %s differ" % (what, bad[:8])


# (N, B, flags, start_heading): every N and every batch size, random / fixed cells, fixed / drawn headings
RESET_CASES = [(7, 4096, "goal show", None), (12, 512, "start goal show", 1), (14, 64, "start", None),
               (21, 3, "start goal show", None), (21, 4096, "", 3), (7, 64, "start goal", None), (12, 3, "", 0),
               (14, 4096, "start goal", 2)]


@pytest.mark.parametrize("N,B,flags,heading", RESET_CASES)
def test_reset_frames_match_the_host_model(N, B, flags, heading):
    """The first observation of every actor with its apples, byte for byte, with cell, heading, goal and record; then a
    masked reset."""
    seed = 0xA11E + N + B
    cfg = _config(N, L=7, seed=B, marks="SG", random_start="start" in flags, random_goal="goal" in flags,
                  show_goal="show" in flags, start_heading=heading, apple_reward=3)
    assert cfg.nav
    env = _env(B, 2, cfg, seed=seed)
    models = _hosts(cfg, B, seed)
    _check_state(env.ring, models, "reset")
    green = sum(int((m.frame == NM.APPLE_FLOOR).all(2).any()) for m in models)
    assert green > 0
    mask = np.random.RandomState(B).uniform(size=B) < 0.5
    env.reset(torch.from_numpy(mask.astype(np.int32)).to(DEV))
    for b in np.flatnonzero(mask):
        models[b].reset()
    _check_state(env.ring, models, "masked reset")


# (action set, (goal, apple, hit) rewards, goal_respawn)
STEP_MODES = [("lab", (10, 1, 0), True), ("turn", (1, 1, -1), False), ("lab", (1, 1, -1), False),
              ("turn", (10, 1, 0), True)]
# every N runs both action sets, both reward sets, and goal_respawn on and off
STEP_CASES = [(7, 0), (7, 1), (12, 2), (12, 3), (14, 0), (14, 1), (21, 2), (21, 3)]


@pytest.mark.parametrize("N,mode", STEP_CASES)
def test_random_steps_match_the_host_model(N, mode):
    """Seven layouts with apples over 200 actors, random start / goal, the goal shown, a step limit of 37, 120 random
    actions with a masked reset half way: frames, pixel change (bit for bit, and equal to unreal_pixel_change_u8 on the
    two stored frames), rewards, terminals, records, counts, cells, headings, episode steps / indices.  Apples, hits,
    time-outs, goals and (with goal_respawn) respawns all happen."""
    _steps(N, *STEP_MODES[mode])


def _steps(N, action_set, rewards, respawn):
    from unreal_amd import ops
    B, H, steps, seed = 200, 3, 120, 0xBEEF + N
    H1 = H + 1
    A = 6 if action_set == "lab" else 4
    cfg = _config(N, L=7, seed=N, random_start=True, random_goal=True, show_goal=True, max_episode_steps=37,
                  goal_reward=rewards[0], apple_reward=rewards[1], hit_reward=rewards[2], goal_respawn=respawn,
                  action_set=action_set)
    env = _env(B, H, cfg, seed=seed)
    ring = env.ring
    models = _hosts(cfg, B, seed)
    assert len(set(ring.layout.cpu().numpy())) == 7
    rs = np.random.RandomState(N)
    out_r = torch.zeros(B, dtype=torch.float32, device=DEV)
    out_t = torch.zeros(B, dtype=torch.int32, device=DEV)
    pc_u8 = torch.zeros(B * PC, dtype=torch.float32, device=DEV)
    committed_terminal = np.zeros(B, dtype=bool)
    count = np.zeros(B, dtype=np.int64)
    n = dict(goal=0, timeout=0, hit=0, apple=0, respawn=0)
    _check_state(ring, models, "after reset", count)
    for step in range(steps):
        acts = rs.randint(0, A, B).astype(np.int32)
        env.process(torch.from_numpy(acts).to(DEV), None, out_r, out_t, reset_on_terminal=True, track_score=True)
        want_r, want_t, want_pc = [], [], []
        for b, m in enumerate(models):
            _, r, t, pc = m.process(acts[b])
            want_r.append(r); want_t.append(t); want_pc.append(pc)
            n["goal"] += m.at_goal
            n["timeout"] += m.timed_out
            n["hit"] += m.hit
            n["apple"] += m.apple
            n["respawn"] += m.respawned
            if t:
                m.reset()
        np.testing.assert_array_equal(out_r.cpu().numpy(), np.array(want_r, dtype=np.float32), err_msg=str(step))
        term = np.array(want_t, dtype=bool)
        np.testing.assert_array_equal(out_t.cpu().numpy(), term.astype(np.int32), err_msg=str(step))
        old = count.copy()
        discard = term & (old > 0) & committed_terminal
        count = np.where(discard, old, old + 1)
        committed_terminal = np.where(discard, committed_terminal, term)
        _check_state(ring, models, "step %d" % step, count)
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
            _check_state(ring, models, "masked reset", count)
    assert n["goal"] > 0 and n["timeout"] > 0 and n["apple"] > 0 and n["hit"] > 0, n
    assert n["respawn"] > 0 or not respawn, n
    return n


@pytest.mark.parametrize("B", [64, 300])
def test_fused_rollout_steps_are_the_two_launch_paths_at_six_actions(B):
    """A = 6 on a navigation block, on two views of each environment: rollout_step == process + rollout_advance (+ cur_idx
    and the LSTM-input columns), and policy_rollout_step == policy_step + rollout_step, bit for bit, with goals (respawns),
    apples and time-outs."""
    from unreal_amd import ops
    H, A, xld = 4, 6, 264
    rs = np.random.RandomState(B)
    dev = lambda a, dt: torch.from_numpy(np.asarray(a)).to(DEV, dt)
    Wp = dev(rs.uniform(-.3, .3, 256 * A), torch.float32); bp = dev(rs.uniform(-.1, .1, A), torch.float32)
    Wv = dev(rs.uniform(-.3, .3, 256), torch.float32); bv = dev(rs.uniform(-.1, .1, 1), torch.float32)
    cfg = _config(7, L=3, random_goal=True, random_start=True, show_goal=True, max_episode_steps=5, goal_reward=10,
                  apple_reward=1, hit_reward=0, goal_respawn=True, action_set="lab")
    envs = [_env(B, H, cfg, seed=9) for _ in range(3)]
    cut = B // 3
    views = [[e.view(0, cut), e.view(cut, B)] for e in envs]
    st = [_rollout_state(B, xld) for _ in envs]
    for s in st:
        s["pi"] = torch.zeros(B * A, dtype=torch.float32, device=DEV)
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
        for name in NAV_ARRAYS:
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
    assert n_term > 0 and {10.0, 1.0} <= n_rew, (n_term, n_rew)
    assert int(envs[0].ring.nav.view(B, 8)[:, 3].sum()) > 0 and int(envs[0].ring.nav.view(B, 8)[:, 4].sum()) > 0
    assert set(st[0]["a"].cpu().numpy().tolist()) >= {4, 5}


def test_a_policy_step_whose_A_is_not_the_blocks_action_count_writes_nothing():
    """A = 6 on a navigation block with the turn set (and A = 4 on one with Lab's set): the kernel returns before any
    store, like a block of another grid size."""
    from unreal_amd import ops
    for action_set, A in (("turn", 6), ("lab", 4)):
        cfg = _config(7, L=1, random_goal=True, random_start=True, apple_reward=2, action_set=action_set)
        env = _env(8, 2, cfg, seed=1)
        z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=DEV)
        before = {n: getattr(env.ring, n).clone() for n in NAV_ARRAYS}
        acts, pi, active = z(8, torch.int32) - 1, z(8 * A) - 1, z(8, torch.int32) + 1
        ops.maze_policy_rollout_step(env.ring, z(8 * 256) + 1, 256, z(256 * A) + 1, z(A), z(256), z(1),
                                     z(8, torch.float64) + 0.5, pi, z(8), acts, z(8), z(8, torch.int32), active,
                                     z(8, torch.int32), z(8, torch.int32), z(8, torch.int32), A=A, maze=env.maze)
        torch.cuda.synchronize()
        assert (acts == -1).all() and (pi == -1).all() and (active == 1).all()
        for n, t in before.items():
            assert torch.equal(getattr(env.ring, n), t), (action_set, n)


# the goal two cells from the start (no episode ends on its first step); apples around; respawn at S
NAV_ROOM = ["+++++++",
            "+++++++",
            "++A-G++",
            "++-SA++",
            "++A-A++",
            "+++++++",
            "+++++++"]


def _register(name, layout=NAV_ROOM, **kw):
    from unreal_amd.environment.environment import Environment
    Environment.register_maze_config(name, [layout], view="first_person", **kw)
    return Environment.MAZE_CONFIG[name]


NAV_KW = dict(goal_reward=10, apple_reward=1, hit_reward=0, action_set="lab", show_goal=True)


@pytest.mark.parametrize("use_lstm,aux", [(True, True), (False, False)])
def test_process_on_a_navigation_maze_matches_oracle(use_lstm, aux):
    """Trainer.process against OracleTrainer with one host model per actor at A = 6 and rewards (10, 1, 0) (the LSTM
    input's reward column unbounded), at the bars of test_process_on_a_first_person_maze_matches_oracle."""
    from unreal_amd.environment.environment import Environment
    from oracle.trainer import OracleTrainer, ExplicitDraws
    name = "nav_room_%d%d" % (use_lstm, aux)
    conf = _register(name, goal_respawn=True, max_episode_steps=7, **NAV_KW)
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(use_lstm, aux, H, T)
        cfg["action_size"] = 6
        cfg["initial_learning_rate"] = 7.0711e-4
        net, applier, tr, draws = _build(cfg, B, seed=3, env_name=name)
        assert tr.action_size == 6 and not net.lar_bounded
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = NM.host_batch(conf, B, seed=tr.seed)
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
        assert sum(h.goals_total for h in hosts) > 0 and sum(h.apples_total for h in hosts) > 0
        assert 1.0 in rewards
    finally:
        Environment.MAZE_CONFIG.pop(name, None)


def test_grouped_process_on_a_navigation_maze_is_the_reference_algorithm():
    """groups = B at A = 6: one process() call = B sequential single-actor passes, against OracleTrainer.process_async."""
    from unreal_amd.environment.environment import Environment
    from oracle.trainer import OracleTrainer, ExplicitDraws
    name = "nav_room_grouped"
    conf = _register(name, goal_respawn=True, max_episode_steps=5, **NAV_KW)
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(True, True, H, T)
        cfg["action_size"] = 6
        cfg["initial_learning_rate"] = 7.0711e-4
        net, applier, tr, draws = _build(cfg, B, seed=13, env_name=name, groups=B)
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = NM.host_batch(conf, B, seed=tr.seed)
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


@pytest.mark.parametrize("respawn", [True, False])
def test_evaluate_on_a_navigation_maze_matches_the_host_model(respawn):
    """Evaluate(maze=name): per-actor rewards / terminals of every step agree with the host model replaying the device's
    actions; success_rate, goals_per_episode and apples_per_episode are those of the first episodes."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.evaluate import Evaluate
    name = "nav_room_eval_%d" % respawn
    lay = ["-------", "--A-A--", "-A---A-", "---A---", "-A---A-", "--A-A--", "-------"]
    conf = _register(name, lay, random_goal=True, random_start=True, max_episode_steps=12, goal_respawn=respawn,
                     **NAV_KW)
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
        hosts = NM.host_batch(conf, B, seed=seed)
        for h in hosts:
            h.reset()
        first = [None] * B
        for step, (acts, rew, term) in enumerate(log):
            for b, h in enumerate(hosts):
                g0, a0 = h.goals_total, h.apples_total
                _, r, t, _ = h.process(acts[b])
                assert (float(r), int(t)) == (float(rew[b]), int(term[b])), (step, b)
                h.ep_goals = getattr(h, "ep_goals", 0) + h.goals_total - g0
                h.ep_apples = getattr(h, "ep_apples", 0) + h.apples_total - a0
                if t:
                    assert h.ep_steps == 12 or not respawn          # with goal_respawn only the time-out ends one
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
        assert n_succ > 0 and sum(apples) > 0, first
    finally:
        Environment.MAZE_CONFIG.pop(name, None)


def test_batch1_environment_on_a_navigation_maze():
    """Environment.create_environment('maze', name) on a navigation config: images, rewards, terminals and pixel change
    of the host model (no reset on terminal: the caller resets)."""
    from unreal_amd.environment.environment import Environment
    name = "nav_room_batch1"
    lay = ["-------", "--A-A--", "-A---A-", "---A---", "-A---A-", "--A-A--", "-------"]
    conf = _register(name, lay, random_goal=True, random_start=True, max_episode_steps=15, goal_respawn=True, **NAV_KW)
    try:
        env = Environment.create_environment("maze", name)
        host = NM.HostNavMaze(conf, 0, 1, seed=0)
        host.reset()
        np.testing.assert_array_equal(env.last_state["image"], host.last_state["image"])
        rs = np.random.RandomState(2)
        n_term = n_apple = 0
        for step in range(150):
            a = int(rs.randint(0, 6))
            image, reward, terminal, pc = env.process(a)
            _, r, t, pc_h = host.process(a)
            np.testing.assert_array_equal(image, host.last_state["image"], err_msg=str(step))
            assert (reward, terminal) == (r, t), step
            np.testing.assert_array_equal(pc, pc_h, err_msg=str(step))
            n_apple += host.apple
            if terminal:
                n_term += 1
                env.reset()
                host.reset()
                np.testing.assert_array_equal(env.last_state["image"], host.last_state["image"])
        assert n_term > 0 and n_apple > 0
    finally:
        Environment.MAZE_CONFIG.pop(name, None)
