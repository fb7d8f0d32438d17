"""Configured mazes on the device (Environment.register_maze_config: a config block in the unreal_maze_* entries) against
the reference map's null-config path and the host model of tests/maze_model.py."""
import numpy as np
import pytest
import torch

try:
    import maze_model as MM
except ImportError:            # imported as tests.<module>
    from tests import maze_model as MM
try:
    from test_trainer_gpu import _cfg, _build, _feed_draws, RecordingDraws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL
except ImportError:
    from tests.test_trainer_gpu import _cfg, _build, _feed_draws, RecordingDraws, LOSS_ATOL, LOSS_RTOL, GRAD_ATOL, GRAD_REL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FB, PC = 21168, 400
RING_ARRAYS = ("frames", "r_reward", "r_action", "r_terminal", "r_last_action", "r_last_reward", "r_pc", "pos", "count",
               "last_action", "last_reward", "episode_reward", "score_out", "score_valid")
CFG_ARRAYS = ("goal", "layout", "ep_steps", "episode")


def _env(B, H, config=None, seed=0, **kw):
    from unreal_amd.environment.maze_environment import BatchedMazeEnvironment
    env = BatchedMazeEnvironment(B, H, DEV, config=config, seed=seed, **kw)
    env.ring.frames.zero_()           # (torch.empty: slots no step has written would hold stale allocator bytes)
    env.ring.r_pc.zero_()
    return env


def _config(N, L=5, seed=0, marks="", **kw):
    from unreal_amd.environment.maze_environment import MazeConfig
    rs = np.random.RandomState(seed + N)
    return MazeConfig([MM.random_layout(N, rs, marks=marks) for _ in range(L)], **kw)


def _current_frames(ring):
    idx = ring.cur_idx().long()
    return ring.frames.view(-1, FB)[idx].cpu().numpy()


@pytest.mark.parametrize("B", [3, 64, 512, 4096])
def test_reference_map_through_the_cfg_path_is_the_default(B):
    """The reference's map registered as a config (a config block in device memory) steps and renders bit for bit like
    the null-config kernels, at every actors-per-workgroup tier."""
    from unreal_amd import ops
    from unreal_amd.environment.maze_environment import MazeConfig
    H = 3
    envs = [_env(B, H), _env(B, H, MazeConfig.reference(), seed=5)]
    rs = np.random.RandomState(B)
    pos = envs[0].ring.pos.cpu()
    pos[0:2 * (B // 2):2], pos[1:2 * (B // 2):2] = 5, 0          # one RIGHT from the goal: episodes end inside the test
    for e in envs:
        e.reset()
        e.ring.pos.copy_(pos)
    z = lambda dt: torch.zeros(B, dtype=dt, device=DEV)
    outs = [(z(torch.float32), z(torch.int32)) for _ in envs]
    n_term = 0
    for step in range(12):
        a = torch.from_numpy(rs.randint(0, 4, B).astype(np.int32)).to(DEV)
        for e, (r, t) in zip(envs, outs):
            e.process(a, None, r, t, reset_on_terminal=step % 3 != 2, track_score=True)
        if step == 6:
            m = torch.from_numpy((rs.uniform(size=B) < 0.3).astype(np.int32)).to(DEV)
            for e in envs:
                e.reset(m)
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), step
        for name in RING_ARRAYS:
            assert torch.equal(getattr(envs[0].ring, name), getattr(envs[1].ring, name)), (step, name)
        n_term += int(outs[0][1].sum())
    assert n_term > 0                  # goals reached, with and without the reset on terminal
    assert ops.last_launch() == "maze_step " + ("tiny" if B <= 64 else "apg2" if B <= 1024 else "big")
    g = envs[1].ring.goal.cpu().numpy().reshape(B, 2)
    assert (g == (6, 0)).all()


def _straddles(layout, apg):
    """Whether some workgroup of `apg` actors holds actors of two layouts (the wall-image rebuild inside a workgroup)."""
    pad = -len(layout) % apg
    groups = np.concatenate([layout, np.repeat(layout[-1:], pad)]).reshape(-1, apg)
    return bool((groups != groups[:, :1]).any())


# (N, actors, steps, flags, marks): L = 7 layouts put layout boundaries inside workgroups of the step kernel (2 actors
# per workgroup at 200 actors, 8 at 1100) and of the reset kernel (8); the last case draws the start around a fixed G
HOST_MODEL_CASES = [(7, 200, 300, "start goal", ""), (12, 200, 300, "start goal", ""), (14, 200, 300, "start goal", ""),
                    (21, 200, 300, "start goal", ""), (21, 1100, 80, "start goal", ""), (7, 200, 300, "start", "G")]


@pytest.mark.parametrize("N,B,steps,random,marks", HOST_MODEL_CASES)
def test_configured_maze_matches_the_host_model(N, B, steps, random, marks):
    """Seven layouts, random start (and goal), the goal block shown, a step limit of 37: random-action steps and one
    masked reset, every frame byte, reward, terminal, position, goal, count, episode step / index and last action /
    reward exact against the host model; pixel change within 3e-7 of it, and equal to unreal_pixel_change_u8 on the two
    stored frames at non-reset steps."""
    from unreal_amd import ops
    H, seed = 3, 0xBEEF + N + B
    H1 = H + 1
    cfg = _config(N, L=7, seed=B, random_start="start" in random, random_goal="goal" in random, show_goal=True,
                  max_episode_steps=37, marks=marks)
    env = _env(B, H, cfg, seed=seed)
    env.reset()                        # (after the zeroing: the frames of slot 0 again)
    ring = env.ring
    models = MM.host_batch(cfg, B, seed=seed)
    for m in models:
        m.reset()
    layout = ring.layout.cpu().numpy()
    np.testing.assert_array_equal(layout, [m.layout for m in models])
    assert len(set(layout)) == 7
    assert _straddles(layout, 2 if B <= 1024 else 8) and _straddles(layout, 8)
    rs = np.random.RandomState(N + B)
    out_r = torch.zeros(B, dtype=torch.float32, device=DEV)
    out_t = torch.zeros(B, dtype=torch.int32, device=DEV)
    pc_u8 = torch.zeros(B * PC, dtype=torch.float32, device=DEV)
    committed_terminal = np.zeros(B, dtype=bool)
    count = np.zeros(B, dtype=np.int64)
    n_goal = n_timeout = 0

    def check_state(what):
        np.testing.assert_array_equal(ring.count.cpu().numpy(), count, err_msg=what)
        np.testing.assert_array_equal(ring.pos.cpu().numpy().reshape(B, 2), [(m.x, m.y) for m in models], err_msg=what)
        np.testing.assert_array_equal(ring.goal.cpu().numpy().reshape(B, 2), [(m.gx, m.gy) for m in models], err_msg=what)
        np.testing.assert_array_equal(ring.ep_steps.cpu().numpy(), [m.ep_steps for m in models], err_msg=what)
        np.testing.assert_array_equal(ring.episode.cpu().numpy(), [m.episode for m in models], err_msg=what)
        np.testing.assert_array_equal(ring.last_action.cpu().numpy(), [m.last_action for m in models], err_msg=what)
        np.testing.assert_array_equal(ring.last_reward.cpu().numpy(), np.array([m.last_reward for m in models], np.float32),
                                      err_msg=what)
        want = np.stack([m.last_state['image'].astype(np.uint8).reshape(-1) for m in models])
        np.testing.assert_array_equal(_current_frames(ring), want, err_msg="frames, " + what)

    check_state("after reset")
    for step in range(steps):
        acts = rs.randint(0, 4, B).astype(np.int32)
        env.process(torch.from_numpy(acts).to(DEV), None, out_r, out_t, reset_on_terminal=True, track_score=True)
        want_r, want_t, want_pc = [], [], []
        for b, m in enumerate(models):
            _, r, t, pc = m.process(acts[b])
            want_r.append(r); want_t.append(t); want_pc.append(pc)
            n_goal += t and not m.timed_out
            n_timeout += t and m.timed_out
            if t:
                m.reset()
        np.testing.assert_array_equal(out_r.cpu().numpy(), np.array(want_r, dtype=np.float32), err_msg=str(step))
        term = np.array(want_t, dtype=bool)
        np.testing.assert_array_equal(out_t.cpu().numpy(), term.astype(np.int32), err_msg=str(step))
        old = count.copy()
        discard = term & (old > 0) & committed_terminal
        count = np.where(discard, old, old + 1)
        committed_terminal = np.where(discard, committed_terminal, term)
        check_state("step %d" % step)
        base = np.arange(B) * H1 + old % H1
        pc_dev = ring.r_pc.view(-1, PC)[torch.from_numpy(base).to(DEV)].cpu().numpy()
        assert np.abs(pc_dev - np.stack(want_pc).reshape(B, PC)).max() <= 3e-7, step
        live = np.flatnonzero(~term)
        if len(live):
            idx_new = torch.from_numpy((live * H1 + count[live] % H1).astype(np.int32)).to(DEV)
            idx_old = torch.from_numpy((live * H1 + old[live] % H1).astype(np.int32)).to(DEV)
            ops.pixel_change_u8(ring.frames, idx_new, idx_old, 48.0, pc_u8[:len(live) * PC])
            np.testing.assert_array_equal(pc_u8[:len(live) * PC].cpu().numpy().reshape(-1, PC), pc_dev[live])
        if step == steps // 2:         # a masked reset (maze_reset_kernel) in the middle of the run
            mask = rs.uniform(size=B) < 0.5
            env.reset(torch.from_numpy(mask.astype(np.int32)).to(DEV))
            for b in np.flatnonzero(mask):
                models[b].reset()
            check_state("masked reset")
    assert n_goal > 0 and n_timeout > 0, (n_goal, n_timeout)


@pytest.mark.parametrize("B", [64, 1025])
def test_fused_policy_step_on_a_configured_maze_is_the_two_launch_path(B):
    """unreal_maze_policy_rollout_step == unreal_policy_step + unreal_maze_rollout_step on a configured maze, bit for
    bit, with time-outs and goals ending episodes on the way."""
    from unreal_amd import ops
    H, A, xld = 4, 4, 264
    rs = np.random.RandomState(B)
    dev = lambda a, dt: torch.from_numpy(np.asarray(a)).to(DEV, dt)
    Wp = dev(rs.uniform(-.3, .3, 256 * A), torch.float32); bp = dev(rs.uniform(-.1, .1, A), torch.float32)
    Wv = dev(rs.uniform(-.3, .3, 256), torch.float32); bv = dev(rs.uniform(-.1, .1, 1), torch.float32)
    cfg = _config(14, L=3, random_goal=True, random_start=True, show_goal=True, max_episode_steps=3)
    envs = [_env(B, H, cfg, seed=9), _env(B, H, cfg, seed=9)]
    z = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device=DEV)
    st = [dict(active=torch.ones(B, dtype=torch.int32, device=DEV), log=z(B), n=z(B), te=z(B), r=z(B, torch.float32),
               t=z(B), a=z(B), pi=z(B * A, torch.float32), v=z(B, torch.float32), idx=z(B),
               lar=torch.zeros(B * xld, device=DEV)) for _ in envs]
    n_term = 0
    for step in range(5):
        X = dev(rs.uniform(-1, 1, (B, 256)), torch.float32).view(-1)
        u = dev(rs.uniform(0, 1, B), torch.float64)
        (e0, e1), (s0, s1) = envs, st
        ops.policy_step(B, A, X, 256, Wp, bp, Wv, bv, u, s0["pi"], s0["v"], s0["a"])
        ops.maze_rollout_step(e0.ring, s0["a"], s0["r"], s0["t"], s0["active"], s0["log"], s0["n"], s0["te"],
                              next_idx=s0["idx"], next_lar=s0["lar"], lar_ld=xld, lar_col0=256, A=A, maze=e0.maze)
        ops.maze_policy_rollout_step(e1.ring, X, 256, Wp, bp, Wv, bv, u, s1["pi"], s1["v"], s1["a"], s1["r"], s1["t"],
                                     s1["active"], s1["log"], s1["n"], s1["te"], next_idx=s1["idx"], next_lar=s1["lar"],
                                     lar_ld=xld, lar_col0=256, A=A, maze=e1.maze)
        for k in s0:
            assert torch.equal(s0[k], s1[k]), (step, k)
        for name in RING_ARRAYS + CFG_ARRAYS:
            assert torch.equal(getattr(e0.ring, name), getattr(e1.ring, name)), (step, name)
        n_term += int(s0["t"].sum())
    assert n_term > 0


def test_two_views_are_the_whole_environment():
    """Two half-batch views (their own global actor base) step, reset and draw exactly like the whole environment."""
    B, H = 200, 3
    cfg = _config(21, L=64, random_goal=True, random_start=True, show_goal=True, max_episode_steps=11)
    whole, split = _env(B, H, cfg, seed=4), _env(B, H, cfg, seed=4)
    views = [split.view(0, 120), split.view(120, B)]
    rs = np.random.RandomState(1)
    out = [(torch.zeros(B, dtype=torch.float32, device=DEV), torch.zeros(B, dtype=torch.int32, device=DEV)) for _ in range(2)]
    for step in range(40):
        a = torch.from_numpy(rs.randint(0, 4, B).astype(np.int32)).to(DEV)
        whole.process(a, None, out[0][0], out[0][1], track_score=True)
        for v, (b0, b1) in zip(views, ((0, 120), (120, B))):
            v.process(a[b0:b1], None, out[1][0][b0:b1], out[1][1][b0:b1], track_score=True)
        if step == 20:
            m = torch.from_numpy((rs.uniform(size=B) < 0.5).astype(np.int32)).to(DEV)
            whole.reset(m)
            views[0].reset(m[:120])
            views[1].reset(m[120:])
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), step
        for name in RING_ARRAYS + CFG_ARRAYS:
            assert torch.equal(getattr(whole.ring, name), getattr(split.ring, name)), (step, name)
    assert int(whole.ring.episode.min()) >= 3


GOAL_ROOM = ["+++++++",
             "+++++++",
             "++---++",
             "++-S-++",
             "++---++",
             "+++++++",
             "+++++++"]


def test_process_on_a_configured_maze_matches_oracle():
    """Trainer.process, full UNREAL, on a configured maze with a random goal and a step limit against OracleTrainer with
    one host-model environment per actor: the bars and the draw replay of test_process_matches_oracle."""
    from unreal_amd.environment.environment import Environment
    from oracle.trainer import OracleTrainer, ExplicitDraws
    Environment.register_maze_config("goal_room", [GOAL_ROOM], random_goal=True, max_episode_steps=7)
    try:
        B, H, T = 3, 40, 20
        cfg = _cfg(True, True, H, T)
        cfg["initial_learning_rate"] = 7.0711e-4
        net, applier, tr, draws = _build(cfg, B, seed=3, env_name="goal_room")
        assert tr.environment.config is Environment.MAZE_CONFIG["goal_room"]
        params = {k: torch.tensor(v, dtype=torch.float64) for k, v in net.export_named().items()}
        edraws = [ExplicitDraws() for _ in range(B)]
        hosts = MM.host_batch(Environment.MAZE_CONFIG["goal_room"], B, seed=tr.seed)
        orc = OracleTrainer(cfg, n_actors=B, draws=edraws, dtype=torch.float64, params=params, envs=hosts)
        while not tr._full:
            tr.process(None, 0)
        for step_u in draws.log:
            for b in range(B):
                edraws[b].action_u.append(float(step_u[b]))
        orc.fill()
        np.testing.assert_array_equal(tr.ring.count.cpu().numpy(), [a.exp.count for a in orc.actors])
        np.testing.assert_array_equal(tr.ring.pos.cpu().numpy().reshape(B, 2), [(h.x, h.y) for h in hosts])
        np.testing.assert_array_equal(tr.ring.goal.cpu().numpy().reshape(B, 2), [(h.gx, h.gy) for h in hosts])
        goals = timeouts = 0
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
                if infos[b]["terminal_end"]:
                    goals += infos[b]["rewards"][-1] == 1
                    timeouts += infos[b]["rewards"][-1] != 1
            for key in ("policy_loss", "value_loss", "pc_loss", "vr_loss", "rp_loss", "total_loss"):
                want = np.mean([l[key] for l in losses_o])
                assert abs(losses_dev[key] - want) <= LOSS_ATOL + LOSS_RTOL * abs(want), (it, key, losses_dev[key], want)
            for (name, _), gref in zip(orc.params.items(), mean_g):
                gr = gref.numpy().reshape(-1)
                assert np.abs(g_dev[name] - gr).max() <= GRAD_ATOL + GRAD_REL * np.abs(gr).max(), (it, name)
            assert abs(float(tr.last_grad_norm.cpu()[0]) - norm_o) <= 1e-4 * max(1.0, norm_o)
            for b in range(B):
                assert tuple(tr.ring.pos.cpu().numpy()[2 * b:2 * b + 2]) == (hosts[b].x, hosts[b].y)
        assert goals > 0 and timeouts > 0, (goals, timeouts)
    finally:
        Environment.MAZE_CONFIG.pop("goal_room", None)


def test_evaluate_counts_goals_and_timeouts_of_the_configured_maze():
    """Evaluate(maze=...): success = the goal reached, time-outs = the environment's own.  The host model replays the
    device's actions from the same episode (Evaluate.process resets the environment first, so each host resets once
    too): every step's reward and terminal agree per actor, each actor's first episode ends the same way, and the
    evaluator's counts are those of the first episodes."""
    from unreal_amd.environment.environment import Environment
    from unreal_amd.evaluate import Evaluate
    Environment.register_maze_config("goal_room_eval", [GOAL_ROOM], random_goal=True, random_start=True,
                                     show_goal=True, max_episode_steps=6)
    try:
        cfg = _cfg(True, False, 40, 20)
        net, _, _, _ = _build(cfg, 1, seed=31)
        B, seed = 16, 0x5EED
        ev = Evaluate(net, batch_size=B, device=DEV, seed=seed, maze="goal_room_eval")
        log = []
        inner = ev.env.process

        def recording(actions, active, out_reward, out_terminal, **kw):
            inner(actions, active, out_reward, out_terminal, **kw)
            log.append((actions.cpu().numpy().copy(), out_reward.cpu().numpy().copy(), out_terminal.cpu().numpy().copy()))
        ev.env.process = recording
        res = ev.process(0, one_episode_per_actor=True)
        hosts = MM.host_batch(Environment.MAZE_CONFIG["goal_room_eval"], B, seed=seed)
        for h in hosts:
            h.reset()                  # Evaluate.process: self.env.reset()
        host_first, dev_first = [None] * B, [None] * B
        for step, (acts, rew, term) in enumerate(log):
            for b, h in enumerate(hosts):
                _, r, t, _ = h.process(acts[b])
                assert (float(r), int(t)) == (float(rew[b]), int(term[b])), (step, b)
                if t:
                    if host_first[b] is None:
                        host_first[b] = "timeout" if h.timed_out else "goal"
                        dev_first[b] = "goal" if rew[b] == 1.0 else "timeout"
                    h.reset()
        assert None not in host_first
        assert dev_first == host_first
        n_goal = host_first.count("goal")
        assert res["episodes"] == B and res["timeouts"] == B - n_goal
        assert abs(res["success_rate"] - n_goal / float(B)) < 1e-12
        assert 0 < n_goal < B, host_first
    finally:
        Environment.MAZE_CONFIG.pop("goal_room_eval", None)
